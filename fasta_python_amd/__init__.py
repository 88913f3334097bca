"""fasta_python_amd -- MI355X-native forward-backward splitting behind the fasta-python call surface.

    from fasta_python_amd import fasta, Convergence, linalg, proximal, stopping, losses

`fasta(A[, At], f, gradf, g, proxg, x0, ...)` keeps the reference's signature, options, defaults
and `Convergence` record (reference: fasta/__init__.py:38-53, :323-351); the work runs in
hand-written HIP kernels through the ctypes C ABI of include/fasta_hip.h.  The top-level `fasta`
package in this repository re-exports these names so `import fasta` keeps working.

Which loop runs is decided by the operand types: device-recognisable operands (matrix / sparse matrix / DenseMatrixMap / SparseMatrixMap / GradDivMap + tagged
loss + tagged prox) run the HIP loop and raise when the built `libfasta_hip.so` or a gfx950 GPU is missing -- no CPU fallback;
`A=None` with a tagged losses.Quadratic or losses.Factorization runs the HIP loop too (csrc/fh_quad.h, csrc/fh_bilinear.h), and so does `A=None` with one tagged
losses.LogisticLoss(B) / LeastSquares(B) and a 2-D x0 of B's shape (the identity operator, csrc/fh_nuclear.h: proximal.NuclearShrink / NuclearBall, observation weights); closures, callable pairs, any other `A=None` and host LinearMaps cannot execute inside a kernel and run the generic host loop
(`generic.py`, the reference's semantics).  `backend="hip"` / `backend="numpy"` force either.
"""

from . import certificates, generic, hip, linalg, losses, preprocess, proximal, regpath, stopping
from .certificates import Certificate, critical_mu, duality_gap
from .linalg import BilinearMap, ConvMap, DCTMap, DenseMatrixMap, GradDivMap, IdentityMap, LinearMap, LinearOperator, QuadraticMap, ShardedDenseMatrixMap, SparseMatrixMap
from .losses import Factorization, LeastSquares, LogisticLoss, Quadratic, SoftmaxLoss
from .preprocess import Standardization, standardize
from .proximal import Box, GroupShrink, L1Ball, LinfProx, NonNeg, NoProx, NuclearBall, NuclearShrink, RowBall, RowSplit, Shrink, TVDualBall
from .regpath import path
from .solver import EPSILON, Convergence, FBSolver, fasta
from .stopping import DualityGap

__all__ = ["fasta", "Convergence", "FBSolver", "EPSILON", "linalg", "proximal", "stopping", "losses", "hip", "certificates", "preprocess", "standardize", "Standardization", "path", "duality_gap", "critical_mu", "Certificate", "DualityGap",
           "LinearMap", "LinearOperator", "DenseMatrixMap", "ShardedDenseMatrixMap", "SparseMatrixMap", "GradDivMap", "DCTMap", "ConvMap", "QuadraticMap", "BilinearMap", "IdentityMap", "LeastSquares", "LogisticLoss", "SoftmaxLoss", "Quadratic", "Factorization",
           "Shrink", "NonNeg", "LinfProx", "L1Ball", "Box", "TVDualBall", "GroupShrink", "RowBall", "RowSplit", "NuclearShrink", "NuclearBall", "NoProx"]
