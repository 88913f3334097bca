"""Linear maps behind the reference's `fasta.linalg` names (fasta/linalg.py:13-160).

`LinearMap` keeps the reference's callable-pair contract (shape asserts, `.H`, algebra).  Two
subclasses are *recognised* by `fasta()` and run on the device:

  DenseMatrixMap  -- row-major float64 matrix, resident in HBM (from a host ndarray, or generated
                     on the device by the counter-based synthetic generator, optionally one row
                     block of a matrix sharded over GPUs, one process per GPU); with `rhs=L` it maps
                     (n, L) matrices to (m, L) matrices -- one A for L columns, read once per pass
                     (examples/mmv.py, multi-column LASSO / NNLS);
  ShardedDenseMatrixMap -- the same matrix split into contiguous row blocks over several devices
                     of THIS process (single call): `fasta(ShardedDenseMatrixMap(A,
                     devices=[0, 1, ...]), ls.f, ls.gradf, reg.g, reg.prox, x0)`;
  SparseMatrixMap -- a sparse design matrix (any scipy.sparse matrix / array, or CSR arrays), kept on the
                     device by rows and by columns; both directions are gathers (csrc/fh_sparse.h; with `rhs=L`
                     the unknown is an (n, L) matrix and every entry gathers a whole row of it, csrc/fh_spmulti.h);
  GradDivMap      -- the periodic div/grad stencil pair of examples/tv_denoising.py:26-63;
  DCTMap          -- the subsampled orthonormal DCT of examples/democratic_representation.py:80-82, an implicit fast transform (csrc/fh_dct.h); on an image shape (H, W) the separable
                     2-D transform `mask * dctn(x)` / `idctn(mask * w)` (csrc/fh_dct2.h);
  ConvMap         -- periodic convolution with a small kernel (a point-spread function) and its correlation adjoint, an implicit operator (csrc/fh_conv.h);
  QuadraticMap    -- the identity operator of a quadratic smooth term (losses.Quadratic): what `fasta(None, None, q.f, q.gradf, ...)` runs on;
  BilinearMap     -- the identity operator of a bilinear smooth term (losses.Factorization): what `fasta(None, None, fz.f, fz.gradf, ...)` runs on;
  IdentityMap     -- the identity operator on an (M, N) matrix unknown with an elementwise loss (losses.LeastSquares / LogisticLoss): what
                     `fasta(None, None, ll.f, ll.gradf, reg.g, reg.prox, X0)` runs on (examples/logistic_matrix_completion.py, csrc/fh_nuclear.h).

A DenseMatrixMap built from a host ndarray uploads LAZILY: it keeps a reference to the array (as the
closures of fasta/linalg.py:41 do) and copies it into HBM when the device loop first asks for its
context.  Called on a host array -- which is what the generic host loop, the reference's own loop or
user code do -- it applies `A @ x` / `A.T @ y` on the host, exactly the reference's expressions, so
`LinearMap.from_matrix(A)` together with Python closures (examples/lasso.py:42-47, :79) runs
bit-identically to the reference with or without a GPU.  Maps without a host copy (the synthetic
generator, GradDivMap) apply on the device (fh_apply); `device_apply` always does.
"""

from functools import reduce
from operator import mul

import numpy as np

from . import hip

Matrix = np.ndarray
Vector = np.ndarray

__all__ = ["LinearMap", "LinearOperator", "DenseMatrixMap", "ShardedDenseMatrixMap", "SparseMatrixMap", "GradDivMap", "DCTMap", "ConvMap", "QuadraticMap", "BilinearMap", "IdentityMap", "is_sparse_matrix", "Matrix", "Vector"]


class LinearMap:
    """Callable pair (map, adjoint) between array spaces V and W (fasta/linalg.py:13-69)."""

    def __init__(self, map_func, adj_func, Vshape, Wshape=None):
        # 3-argument form (map, adj, shape) = the old `LinearOperator` call used by
        # examples/democratic_representation.py:80-82: an endomorphism on `shape`.
        if Wshape is None:
            Wshape = Vshape
        self.map_func, self.adj_func = map_func, adj_func
        self.Vshape, self.Wshape = tuple(Vshape), tuple(Wshape)

    @staticmethod
    def from_matrix(A, device=0, storage="f64", devices=None):
        """fasta/linalg.py:37-41.  Returns a DenseMatrixMap: `A @ x` / `A.T @ y` on host arrays (the reference's closures), the
        device-resident operator once the device loop adopts it (storage="f32": opt-in float32 storage of the device copy;
        devices=[...]: row blocks over several devices of this process, i.e. a ShardedDenseMatrixMap)."""
        if is_sparse_matrix(A):                    # a scipy.sparse matrix: kept sparse on the device (one device, float64)
            if storage != "f64" or devices is not None:
                raise TypeError('storage="f32" and row sharding are not implemented for a sparse operator on the device')
            return SparseMatrixMap(A, device=device)
        assert A.ndim == 2
        if devices is not None:
            return ShardedDenseMatrixMap(A, devices=devices, storage=storage)
        return DenseMatrixMap(A, device=device, storage=storage)

    @staticmethod
    def identity(shape):
        return LinearMap(lambda x: x, lambda x: x, shape, shape)

    def __call__(self, v):
        assert v.shape == self.Vshape            # AssertionError like fasta/linalg.py:58
        w = self.map_func(v)
        assert w.shape == self.Wshape            # :60
        return w

    @property
    def H(self):
        return LinearMap(self.adj_func, self.map_func, self.Wshape, self.Vshape)

    # ---- algebra (host-side composition of callables; fasta/linalg.py:71-160) -------------------
    def __matmul__(self, B):
        assert isinstance(B, LinearMap) and self.Wshape == B.Vshape     # same check as :77
        return LinearMap(lambda x: self(B(x)), lambda y: B.H(self.H(y)), self.Vshape, B.Wshape)

    def __rmul__(self, k):
        assert np.isscalar(k)
        return LinearMap(lambda x: k * self(x), lambda y: k * self.H(y), self.Vshape, self.Wshape)

    __mul__ = __rmul__

    def __neg__(self):
        return -1 * self

    def __add__(self, B):
        assert isinstance(B, LinearMap) and (self.Vshape, self.Wshape) == (B.Vshape, B.Wshape)
        return LinearMap(lambda x: self(x) + B(x), lambda y: self.H(y) + B.H(y), self.Vshape, self.Wshape)

    def __sub__(self, B):
        return self + (-B)

    @property
    def is_operator(self):
        return self.Vshape == self.Wshape

    def __pow__(self, n, modulo=None):
        assert self.is_operator
        out = LinearMap.identity(self.Vshape)
        for _ in range(n):
            out = out @ self
        return out

    @property
    def _scipy(self):
        from scipy.sparse import linalg as sla
        M = reduce(mul, self.Vshape, 1)
        N = reduce(mul, self.Wshape, 1)
        return sla.LinearOperator((M, N), matvec=lambda x: np.ravel(self(x.reshape(self.Vshape))),
                                  rmatvec=lambda y: np.ravel(self.H(y.reshape(self.Wshape))))

    def eigs(self, k=1):
        from scipy.sparse import linalg as sla
        assert self.is_operator
        values, vectors = sla.eigs(self._scipy, k)
        return values, np.reshape(vectors.T, (k,) + self.Wshape)


LinearOperator = LinearMap      # name the reference's examples import (sparse_least_squares.py:12)


class _DeviceMap(LinearMap):
    """A LinearMap whose operator lives in a HipContext; `fasta()` runs the fused device loop on it."""

    def __init__(self, Vshape, Wshape, device, storage="f64", devices=None, lazy=False, rccl_shell=False):
        self._ctx = None
        self._ctx_args = (device, storage, devices, rccl_shell)
        self.device = device
        LinearMap.__init__(self, self._apply_fwd, self._apply_adj, Vshape, Wshape)
        if not lazy:
            self.ctx                                   # create the device context now (raises without a GPU)

    @property
    def ctx(self):
        """The device context; created -- and, for a map built from a host matrix, filled -- on first use."""
        if self._ctx is None:
            device, storage, devices, rccl_shell = self._ctx_args
            self._ctx = hip.HipContext(device, storage, devices=devices, rccl_shell=rccl_shell)
            try:
                self._on_context(self._ctx)
            except Exception:
                self._ctx.close()
                self._ctx = None
                raise
        return self._ctx

    @ctx.setter
    def ctx(self, value):                              # (test stand-ins install their own context object)
        self._ctx = value

    def _on_context(self, ctx):
        pass

    def device_apply(self, v, adjoint=False):
        """A v (or A^H v) computed by the device kernels on a host array (fh_apply)."""
        shape = self.Vshape if adjoint else self.Wshape
        return self.ctx.apply(np.asarray(v, dtype=np.float64), adjoint=adjoint).reshape(shape)

    def _apply_fwd(self, v):
        return self.device_apply(v, adjoint=False)

    def _apply_adj(self, w):
        return self.device_apply(w, adjoint=True)

    def close(self):
        if self._ctx is not None:
            self._ctx.close()

    def spectral_norm_squared(self, iters=50, rtol=1e-6, seed=None):
        """||A||_2^2 by power iteration on A^H A, the matvecs running on the device: each iteration is one
        `fh_gradient_at` with a zero target (the one-pass kernel reads a dense A once for both directions); the host only
        normalises the n-vector in between.  OPT-IN replacement for `LinearMap.eigs` (linalg.py:149-160) and for the
        four setup passes of fasta()'s random-probe estimate (fasta/__init__.py:100-113): for f = .5||Ax - b||^2 pass
        `L = op.spectral_norm_squared()` and `tau0 = (2 / L) / 10` to fasta().  A different L changes every iterate with
        respect to the reference's RNG-based estimate, so fasta() never calls this by itself.
        Overwrites the context's loss with a zero least-squares target; call it before fasta() (which sets its own)."""
        c = self.ctx
        n = int(np.prod(self.Vshape))
        m = int(np.prod(self.Wshape))
        rng = np.random.RandomState(seed)
        x = rng.randn(n)
        x /= np.linalg.norm(x)
        c.set_loss_lsq(np.zeros(m))
        lam = 0.0
        for _ in range(int(iters)):
            c.set_vector(hip.VEC_T0, x)
            c.gradient_at(hip.VEC_T0, hip.VEC_T1)                  # y = A^H (A x - 0)
            y = c.get_vector(hip.VEC_T1, n)
            new = float(np.dot(x, y))                              # Rayleigh quotient (||x|| = 1)
            ny = float(np.linalg.norm(y))
            if ny == 0.0:
                return 0.0
            x = y / ny
            if abs(new - lam) <= rtol * abs(new):
                lam = new
                break
            lam = new
        return lam


class DenseMatrixMap(_DeviceMap):
    """Dense float64 matrix held row-major in HBM (the operator of fasta/linalg.py:41).

    `rows` = (row0, m_total) describes a row block of a larger matrix when A is sharded across
    ranks (one process per GPU); the default is the whole matrix on one GPU.
    """

    def __init__(self, A=None, device=0, tuning=None, _defer=False, storage="f64", _devices=None, _rccl_shell=False, rhs=None):
        """rhs=L (1..16): the unknown is an (n, L) matrix and the data an (m, L) matrix (`Vshape = (n, L)`, `Wshape = (m, L)`): every
        device pass reads A once for all L columns (csrc/fh_multi.h).  float64 storage, one device.
        storage="f32" (opt-in): keep the device copy of A in float32 -- half the bytes per pass, ~2x the iterations/s on
        large matrices.  The solve is then the reference's solve on the ROUNDED matrix A.astype(float32) (all vectors and
        arithmetic stay float64), so iterates differ from the float64-matrix run by the effect of that rounding."""
        self.rows = None
        self.shape = None
        self.storage = storage
        self.rhs = None if rhs is None else int(rhs)
        if self.rhs is not None:
            if not 1 <= self.rhs <= hip.MAX_RHS:
                raise ValueError(f"rhs must be in 1..{hip.MAX_RHS} columns (got {rhs})")
            if storage != "f64" or _devices is not None:
                raise TypeError("a matrix unknown (rhs=L) needs float64 storage on a single device")
        self.matrix = None                 # host copy (a reference to the caller's array, like the closures of linalg.py:41)
        self._tuning = dict(tuning or {})
        if _defer:
            _DeviceMap.__init__(self, (0,), (0,), device, storage, _devices, rccl_shell=_rccl_shell)
        else:
            assert A is not None and A.ndim == 2
            self.matrix = A
            self.shape = tuple(A.shape)
            cols = () if self.rhs is None else (self.rhs,)
            _DeviceMap.__init__(self, (A.shape[1],) + cols, (A.shape[0],) + cols, device, storage, _devices, lazy=True, rccl_shell=_rccl_shell)

    def _on_context(self, ctx):
        """First use of the device context: tuning, then the one H2D copy of the host matrix."""
        for key, value in self._tuning.items():
            ctx.set_tuning(key, value)
        if self.matrix is not None:
            ctx.set_matrix(self.matrix)
            if self.rhs is not None:
                ctx.set_rhs(self.rhs)

    def _tune(self, tuning):
        self._tuning.update(tuning or {})
        for key, value in (tuning or {}).items():
            self.ctx.set_tuning(key, value)

    # host arrays in, host arrays out: with a host copy of A these ARE the reference's closures (linalg.py:41); a storage="f32"
    # map applies the rounded matrix, i.e. the operator its device copy holds
    def _host_matrix(self):
        if self.storage == "f32" and self.matrix.dtype != np.float32:
            if getattr(self, "_rounded", None) is None:
                self._rounded = self.matrix.astype(np.float32).astype(np.float64)
            return self._rounded
        return self.matrix

    def _apply_fwd(self, v):
        if self.matrix is None:
            return self.device_apply(v, adjoint=False)
        return self._host_matrix() @ v

    def _apply_adj(self, w):
        if self.matrix is None:
            return self.device_apply(w, adjoint=True)
        return self._host_matrix().T @ w

    @classmethod
    def synthetic(cls, m, n, seed, scale, row0=0, m_total=None, device=0, tuning=None, storage="f64", _devices=None, rhs=None):
        """Rows [row0, row0+m) of the counter-based synthetic matrix, generated in HBM; rhs=L as in the constructor."""
        from .synthetic import synth_coef
        self = cls(_defer=True, device=device, storage=storage, _devices=_devices, rhs=rhs)
        self._tune(tuning)
        self.ctx.generate_matrix(m, n, row0, seed, synth_coef(scale))
        cols = () if self.rhs is None else (self.rhs,)
        if self.rhs is not None:
            self.ctx.set_rhs(self.rhs)
        self.Vshape, self.Wshape = (n,) + cols, (m,) + cols
        self.shape = (m, n)
        self.rows = (row0, m if m_total is None else m_total)
        return self

    def take_columns(self, src, idx):
        """This map <- the columns idx (strictly increasing) of the dense map `src`, device to device on one device (fh_gather_columns); the
        column count of the unknown stays.  The map has no host copy afterwards: it applies its device copy."""
        self.ctx.gather_columns(src.ctx, idx)
        if self.rhs is not None:
            self.ctx.set_rhs(self.rhs)
        cols = () if self.rhs is None else (self.rhs,)
        m, n = src.shape[0], int(np.size(idx))
        self.matrix, self.shape = None, (m, n)
        self.Vshape, self.Wshape = (n,) + cols, (m,) + cols

    def standardize(self, center=True, scale=True):
        """The device copy rewritten in place as (a - mean) / scale per column (fh_standardize) -- (means, scales).  The caller's array is
        not what the context holds any more, so the map lets go of it and applies its device copy."""
        means, scales = self.ctx.standardize(center=center, scale=scale)
        self.matrix = None
        return means, scales

    def host_rows(self, row0, nrows):
        """Rows of the DEVICE copy of A pulled back to the host."""
        return self.ctx.get_matrix_rows(row0, nrows)

    @property
    def T(self):
        return self.H


class ShardedDenseMatrixMap(DenseMatrixMap):
    """Dense matrix split into contiguous ROW BLOCKS over several devices driven from this one process -- the single-call
    multi-GPU form of the operator of fasta/linalg.py:41:

        op = ShardedDenseMatrixMap(A, devices=[0, 1, 2, 3])            # or .synthetic(m, n, seed, scale, devices=[...])
        fasta(op, ls.f, ls.gradf, reg.g, reg.prox, x0)                 # b and z are split like the rows, x / g are replicated

    Each iteration is one local launch per device, ONE sum of the A_k^T r_k partials (with the loss sums riding along) and one
    host synchronisation (csrc/fasta_hip.hip:dense_step).  `devices` all different: one GPU per block, the sum is a grouped
    RCCL all-reduce over xGMI; all equal (e.g. [0] * 8): every block on that GPU, summed in block order by an in-library
    kernel -- the same arithmetic on a one-GPU box.  Results differ from the unsharded operator only by the order of the
    float64 sums (~1e-15 relative)."""

    def __init__(self, A=None, devices=(0, 0), tuning=None, storage="f64", _defer=False, _rccl_shell=False):
        """`_rccl_shell` (tests): with a single device id, still build the multi-device form -- one row block whose exchange is the
        grouped ncclAllReduce on a communicator from ncclCommInitAll (FH_CREATE_RCCL_SHELL)."""
        devices = [int(d) for d in devices]
        self.devices = devices
        DenseMatrixMap.__init__(self, A, device=devices[0], tuning=tuning, storage=storage, _defer=_defer, _devices=devices,
                                _rccl_shell=_rccl_shell)

    @classmethod
    def synthetic(cls, m, n, seed, scale, devices=(0, 0), tuning=None, storage="f64"):
        """The whole (m, n) counter-based synthetic matrix, every device generating its own row block in HBM."""
        from .synthetic import synth_coef
        self = cls(devices=devices, storage=storage, _defer=True)
        self._tune(tuning)
        self.ctx.generate_matrix(m, n, 0, seed, synth_coef(scale))
        self.Vshape, self.Wshape = (n,), (m,)
        self.shape = (m, n)
        self.rows = (0, m)
        return self

    def row_blocks(self):
        """[(row0, rows)] of every block, in device-list order."""
        return [self.ctx.shard(k)[1:] for k in range(self.ctx.shard_count())]


def is_sparse_matrix(A):
    """A scipy.sparse matrix or array, told by its interface (SciPy is not imported here)."""
    return not isinstance(A, np.ndarray) and callable(getattr(A, "tocsr", None)) and hasattr(A, "shape") and hasattr(A, "nnz")


def canonical_csr(A):
    """(data float64, indices int32, indptr int64, (m, n)) in canonical CSR -- rows in order, column indices strictly increasing, duplicates
    summed, explicit zeros kept -- from a scipy.sparse matrix / array of any format, or from a raw `((data, indices, indptr), shape)` tuple,
    which must already be canonical (ValueError otherwise: a raw triple is taken as it is, never silently re-sorted)."""
    if is_sparse_matrix(A):
        if len(A.shape) != 2:
            raise AssertionError("matrix operator must be 2-D")
        S = A.tocsr()
        if S is A or S.data is getattr(A, "data", None):
            S = S.copy()                                   # (sum_duplicates / sort_indices work in place: never on the caller's matrix)
        S.sum_duplicates()
        S.sort_indices()
        data, indices, indptr, shape = S.data, S.indices, S.indptr, S.shape
    else:
        try:
            (data, indices, indptr), shape = A
        except (TypeError, ValueError):
            raise TypeError("SparseMatrixMap takes a scipy.sparse matrix / array or a ((data, indices, indptr), shape) tuple") from None
    m, n = (int(k) for k in shape)
    if m < 1 or n < 1:
        raise ValueError(f"matrix must be non-empty (got {m} x {n})")
    if n >= 2 ** 31 or m >= 2 ** 31:
        raise ValueError("matrix dimension exceeds 2^31 - 1: column / row numbers are kept as 32-bit integers")
    data = np.ascontiguousarray(data, dtype=np.float64)
    indices = np.asarray(indices)
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    if indices.dtype.kind not in "iu":
        raise TypeError("CSR indices must be integers")
    if indices.size and (int(indices.min()) < 0 or int(indices.max()) >= n):
        raise ValueError(f"CSR column index out of range for {n} columns")
    indices = np.ascontiguousarray(indices, dtype=np.int32)           # (in range: the narrowing is exact)
    if indptr.shape != (m + 1,) or indices.shape != data.shape or data.ndim != 1:
        raise ValueError(f"CSR arrays do not fit shape {(m, n)}")
    if indptr[0] != 0 or indptr[-1] != data.size or np.any(np.diff(indptr) < 0):
        raise ValueError("CSR indptr must start at 0, be non-decreasing and end at nnz")
    if data.size > 1:
        step_ok = np.diff(indices.astype(np.int64)) > 0
        starts = indptr[1:-1]
        step_ok[starts[(starts > 0) & (starts < data.size)] - 1] = True    # (a row's first entry need not exceed the previous row's last)
        if not step_ok.all():
            bad = int(np.searchsorted(indptr, int(np.flatnonzero(~step_ok)[0]) + 1, side="right")) - 1
            raise ValueError(f"CSR column indices of row {bad} are not strictly increasing (sort them and sum duplicates)")
    return data, indices, indptr, (m, n)


class SparseMatrixMap(_DeviceMap):
    """Sparse matrix on the device (csrc/fh_sparse.h): `A` is any scipy.sparse matrix or array, or a `((data, indices, indptr), shape)`
    tuple of canonical CSR arrays.  It is canonicalised on the host (float64, duplicates summed, indices sorted, explicit zeros kept);
    the device keeps A by rows and A^T by rows and runs both directions as gathers -- no atomics, bitwise repeatable.

    Lazy like a DenseMatrixMap built from a host matrix: the upload happens when the device loop first asks for the context, and on
    host arrays the map is `S @ v` / `S.T @ w`, the closures the reference is given for such a matrix -- so `backend="numpy"` and the
    generic host loop are the reference bit for bit.  One device, float64; prox kinds Shrink / NonNeg / Box / none; both losses.

    rhs=L (1..16): the unknown is an (n, L) matrix and the data an (m, L) matrix (`Vshape = (n, L)`, `Wshape = (m, L)`; on host arrays
    `S @ X` / `S.T @ Y`).  On the device every stored entry then gathers a whole row of X and is paid once for all L columns
    (csrc/fh_spmulti.h); least squares only, prox kinds Shrink / NonNeg / Box / GroupShrink / none."""

    def __init__(self, A, device=0, tuning=None, rhs=None):
        self.rhs = None if rhs is None else int(rhs)
        if self.rhs is not None and not 1 <= self.rhs <= hip.MAX_RHS:
            raise ValueError(f"rhs must be in 1..{hip.MAX_RHS} columns (got {rhs})")
        self.storage = "f64"
        self._tuning = dict(tuning or {})
        self._ctx = None
        self.set_matrix(A)
        _DeviceMap.__init__(self, self.Vshape, self.Wshape, device, lazy=True)

    def set_matrix(self, A):
        """Replace the matrix (any form the constructor takes); the column count of the unknown stays.  Host copy, shapes and -- where the map
        has one -- the context, through the CSR setter it was filled by, hold the new matrix afterwards."""
        data, indices, indptr, shape = canonical_csr(A)
        self.csr = (data, indices, indptr)
        self.shape = shape
        from scipy.sparse import csr_matrix            # (SciPy is needed from here on, not at module import)
        self._host = csr_matrix((data, indices, indptr), shape=shape)
        cols = () if self.rhs is None else (self.rhs,)
        self.Vshape, self.Wshape = (shape[1],) + cols, (shape[0],) + cols
        if self._ctx is not None:
            self._on_context(self._ctx)

    def standardize(self, center=False, scale=True):
        """The device copy rescaled in place, a / scale per column (fh_standardize: a sparse operator is served with center=False) -- (means,
        scales).  The host copy the map applies takes the same division, so it holds the same bits."""
        means, scales = self.ctx.standardize(center=center, scale=scale)
        data, indices, indptr = self.csr
        self.csr = (data / scales[indices], indices, indptr)
        self._host = type(self._host)(self.csr, shape=self.shape)
        return means, scales

    @property
    def nnz(self):
        return int(self.csr[0].size)

    @property
    def matrix(self):
        """The canonical host matrix (scipy.sparse.csr_matrix)."""
        return self._host

    def _on_context(self, ctx):
        for key, value in self._tuning.items():
            ctx.set_tuning(key, value)
        data, indices, indptr = self.csr
        if self.rhs is None:
            ctx.set_matrix_csr(indptr, indices, data, self.shape)
        else:
            ctx.set_matrix_csr_rhs(indptr, indices, data, self.shape, self.rhs)

    def _apply_fwd(self, v):
        return self._host @ v

    def _apply_adj(self, w):
        return self._host.T @ w

    @property
    def T(self):
        return self.H


class QuadraticMap(_DeviceMap):
    """The operator of `fasta(None, None, q.f, q.gradf, g, prox, x0)` with q = losses.Quadratic(Q, c): the identity on x0's shape.  Its device
    context holds Q and c (fh_set_quadratic: operator and loss in one call, csrc/fh_quad.h) for an unknown of shape (n,) or (n, L), L <= 16.
    Lazy like a map built from a host matrix; on host arrays it is the identity, as `A = None` is in the reference (examples/svm.py:74)."""

    def __init__(self, loss, shape, device=0, tuning=None):
        shape = tuple(int(k) for k in shape)
        n = loss.Q.shape[0]
        if len(shape) not in (1, 2) or shape[0] != n or (len(shape) == 2 and not 1 <= shape[1] <= hip.MAX_RHS):
            raise ValueError(f"a quadratic loss on a {n} x {n} matrix takes an unknown of shape ({n},) or ({n}, L), L <= {hip.MAX_RHS} (got {shape})")
        if loss.c is not None and loss.c.shape != shape:
            raise ValueError(f"the linear term c has shape {loss.c.shape}, the unknown {shape}")
        self.loss = loss
        self.shape = (n, n)
        self.rhs = shape[1] if len(shape) == 2 else 1
        self.storage = "f64"
        self._tuning = dict(tuning or {})
        _DeviceMap.__init__(self, shape, shape, device, lazy=True)

    def _on_context(self, ctx):
        for key, value in self._tuning.items():
            ctx.set_tuning(key, value)
        ctx.set_quadratic(self.loss.Q, self.loss.c, self.rhs)

    def _apply_fwd(self, v):
        return v

    def _apply_adj(self, w):
        return w


class BilinearMap(_DeviceMap):
    """The operator of `fasta(None, None, fz.f, fz.gradf, g, prox, Z0)` with fz = losses.Factorization(S): the identity on Z0's shape
    (m + n, K), K <= 16.  Its device context holds S (fh_set_factorization: operator and loss in one call, csrc/fh_bilinear.h).  Lazy like a
    map built from a host matrix; on host arrays it is the identity, as `A = None` is in the reference (examples/nn_factorization.py:63)."""

    def __init__(self, loss, shape, device=0, tuning=None):
        shape = tuple(int(k) for k in shape)
        rows = loss.m + loss.n
        if len(shape) != 2 or shape[0] != rows or not 1 <= shape[1] <= hip.MAX_RHS:
            raise ValueError(f"a factorization of a {loss.m} x {loss.n} matrix takes an unknown of shape ({rows}, K), K <= {hip.MAX_RHS} (got {shape})")
        self.loss = loss
        self.shape = (rows, rows)
        self.rhs = shape[1]
        self.storage = "f64"
        self._tuning = dict(tuning or {})
        _DeviceMap.__init__(self, shape, shape, device, lazy=True)

    def _on_context(self, ctx):
        for key, value in self._tuning.items():
            ctx.set_tuning(key, value)
        ctx.set_factorization(self.loss.S, self.rhs)

    def _apply_fwd(self, v):
        return v

    def _apply_adj(self, w):
        return w


class IdentityMap(_DeviceMap):
    """The operator of `fasta(None, None, loss.f, loss.gradf, g, prox, X0)` with loss = losses.LogisticLoss(B) or losses.LeastSquares(B) and a
    2-D X0 of B's shape: the identity on (M, N) matrices.  Its device context keeps the unknown in the vector form's buffers (fh_set_identity,
    csrc/fh_nuclear.h) and serves proximal.NuclearShrink, NuclearBall, Shrink, NonNeg, Box or no prox, with or without observation weights on the loss
    (losses.LeastSquares / LogisticLoss(B, weights=W): fh_set_loss_weights).  Lazy like QuadraticMap; on host arrays it is the
    identity, as `A = None` is in the reference (examples/logistic_matrix_completion.py:47).
    tuning: {hip.TUNE_NUC_BLOCK_ROWS: 1 | 2 | 4 | 8} sets the rows per block of the nuclear-norm prox's Jacobi steps."""

    MAX_ENTRIES = 1 << 26
    MAX_NUCLEAR_RANK = 1024

    def __init__(self, shape, device=0, tuning=None):
        shape = tuple(int(k) for k in shape)
        if len(shape) != 2 or min(shape) < 1:
            raise ValueError(f"the identity operator takes a non-empty matrix unknown of shape (M, N) (got {shape})")
        if shape[0] * shape[1] > self.MAX_ENTRIES:
            raise ValueError(f"the identity operator serves at most 2^26 entries on the device (got {shape})")
        self.shape = (shape[0] * shape[1], shape[0] * shape[1])
        self.matrix_shape = shape
        self.rhs = None
        self.storage = "f64"
        self._tuning = dict(tuning or {})
        _DeviceMap.__init__(self, shape, shape, device, lazy=True)

    def _on_context(self, ctx):
        for key, value in self._tuning.items():
            ctx.set_tuning(key, value)
        ctx.set_identity(*self.matrix_shape)

    def _apply_fwd(self, v):
        return v

    def _apply_adj(self, w):
        return w


def _nd_grad(X):
    """Periodic discrete gradient of an N-d array -> (N+1)-d (examples/tv_denoising.py:26-40): roll(X, +1, axis) - X per axis."""
    out = np.zeros(X.shape + (X.ndim,))
    for axis in range(X.ndim):
        out[..., axis] = np.roll(X, 1, axis=axis) - X
    return out


def _nd_div(Y):
    """Adjoint of `_nd_grad` (examples/tv_denoising.py:43-63): sum over axes of roll(Y[..., axis], -1, axis) - Y[..., axis]."""
    out = np.zeros(Y.shape[:-1])
    for axis in range(Y.shape[-1]):
        comp = Y[..., axis]
        out += np.roll(comp, -1, axis=axis) - comp
    return out


class GradDivMap(_DeviceMap):
    """A = div and A^H = grad, periodic (examples/tv_denoising.py:26-63), of an image or a volume:
    (H, W):    div : (H, W, 2) -> (H, W), the 2-D stencil kernels (csrc/fh_tv.h);
    (D, H, W): div : (D, H, W, 3) -> (D, H, W), the 3-D stencil kernels (csrc/fh_tv3d.h).  Lazy like a map built from a host matrix: the
               device context is created when the device loop first asks for it, and on host arrays the map is the reference's N-d
               `div` / `grad` closures -- so `backend="numpy"` and the generic host loop are the reference bit for bit."""

    def __init__(self, image_shape, device=0):
        image_shape = tuple(int(k) for k in image_shape)
        if len(image_shape) == 3:
            self.image_shape = image_shape
            _DeviceMap.__init__(self, image_shape + (3,), image_shape, device, lazy=True)
            return
        if len(image_shape) != 2:
            raise ValueError(f"GradDivMap takes an image shape (H, W) or a volume shape (D, H, W); got {len(image_shape)} dimensions")
        H, W = image_shape
        self.image_shape = (H, W)                      # (before the context: _on_context reads it)
        _DeviceMap.__init__(self, (H, W, 2), (H, W), device)
        self.ctx.set_stencil(H, W)

    def _on_context(self, ctx):
        if len(self.image_shape) == 3:
            ctx.set_stencil3d(*self.image_shape)

    def _apply_fwd(self, v):
        if len(self.image_shape) == 3:
            return _nd_div(v)
        return self.device_apply(v, adjoint=False)

    def _apply_adj(self, w):
        if len(self.image_shape) == 3:
            return _nd_grad(w)
        return self.device_apply(w, adjoint=True)


class DCTMap(_DeviceMap):
    """A = mask * DCT and A^H = IDCT(mask * .), the orthonormal DCT-II / DCT-III of length N (examples/democratic_representation.py:80-82):
    an implicit operator -- no matrix is stored, the device runs the transform itself (fh_set_dct, csrc/fh_dct.h), so N = 2^16 ... 2^22 is in
    reach where a dense N x N matrix is not.  `mask`: any float64 vector of length N (the reference's is 0/1), None = all ones.
    On host arrays the map is exactly the reference's closures, `mask * scipy.fftpack.dct(x, norm='ortho')` and
    `scipy.fftpack.idct(mask * w, norm='ortho')`, so `backend="numpy"` and the generic host loop are the reference bit for bit.
    lazy=True: the device context is created when the device loop first asks for it.  An N the device refuses (a prime factor above 5, no
    split within the row cap: `refusal` holds the library's sentence) stays a host map: `fasta()` runs it on the generic host loop, and
    `backend="hip"` raises with that sentence.  tuning (a keyword of this build, as DenseMatrixMap has one): {hip.TUNE_DCT_ROW_CAP: cap} lowers
    the row cap (set before the operator); a cap out of range raises.
    A 2-tuple (H, W) in place of N is the separable transform of an image, A x = mask * (C_H X C_W^T) and A^H w = C_H^T (mask * w) C_W
    (fh_set_dct2, csrc/fh_dct2.h): on host arrays exactly `mask * scipy.fftpack.dctn(x, norm='ortho')` and
    `scipy.fftpack.idctn(mask * w, norm='ortho')`, `mask` of shape (H, W), each axis at most the row cap with prime factors 2, 3 and 5 only
    (an axis of length 1 is the identity).  An int or a 1-tuple is the 1-D operator; any other rank is a ValueError."""

    def __init__(self, N, mask=None, device=0, lazy=False, tuning=None):
        shape = (int(N),) if np.ndim(N) == 0 else tuple(int(k) for k in N)
        if len(shape) not in (1, 2):
            raise ValueError(f"DCTMap takes a length N, a shape (N,) or an image shape (H, W); got {len(shape)} dimensions")
        self.image_shape = shape
        if len(shape) == 2:
            self._init_2d(shape, mask, device, lazy, tuning)
            return
        N = shape[0]
        self.N = N
        self.mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.float64)
        if self.mask is not None and self.mask.shape != (N,):
            raise ValueError(f"mask has shape {self.mask.shape}, a DCT of length {N} takes ({N},)")
        self._tuning = dict(tuning or {})
        cap = self._tuning.get(hip.TUNE_DCT_ROW_CAP, 0)
        self.refusal = hip.dct_refusal(N, cap)           # (a row cap out of range or a library that does not load raises: only a sentence about N is a refusal)
        self.geometry = None if self.refusal is not None else hip.dct_shape(N, cap)
        _DeviceMap.__init__(self, (N,), (N,), device, lazy=lazy or self.refusal is not None)

    def _init_2d(self, shape, mask, device, lazy, tuning):
        H, W = shape
        self.N = H * W
        self.mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.float64)
        if self.mask is not None and self.mask.shape != shape:
            raise ValueError(f"mask has shape {self.mask.shape}, a DCT on an image of shape {shape} takes {shape}")
        self._tuning = dict(tuning or {})
        cap = self._tuning.get(hip.TUNE_DCT_ROW_CAP, 0)
        self.refusal = hip.dct2_refusal(H, W, cap)       # (a row cap out of range or a library that does not load raises: only a sentence about the shape is a refusal)
        self.geometry = None if self.refusal is not None else hip.dct2_shape(H, W, cap)
        _DeviceMap.__init__(self, shape, shape, device, lazy=lazy or self.refusal is not None)

    def _on_context(self, ctx):
        for key, value in self._tuning.items():
            ctx.set_tuning(key, value)
        if len(self.image_shape) == 2:
            ctx.set_dct2(self.image_shape[0], self.image_shape[1], self.mask)
        else:
            ctx.set_dct(self.N, self.mask)

    def _apply_fwd(self, v):
        if len(self.image_shape) == 2:
            from scipy.fftpack import dctn
            y = dctn(v, norm='ortho')
            return y if self.mask is None else self.mask * y
        from scipy.fftpack import dct
        y = dct(v, norm='ortho')
        return y if self.mask is None else self.mask * y

    def _apply_adj(self, w):
        if len(self.image_shape) == 2:
            from scipy.fftpack import idctn
            return idctn(w if self.mask is None else self.mask * w, norm='ortho')
        from scipy.fftpack import idct
        return idct(w if self.mask is None else self.mask * w, norm='ortho')


class ConvMap(_DeviceMap):
    """Periodic convolution of an image (H, W) or a signal (N,) with a small kernel K -- a point-spread function -- and its adjoint, the
    correlation: deblurring, spike deconvolution, inpainting under a blur, compressed sensing by random convolution.
        (A x)[i,j]   = mask[i,j] * sum_{a,b} K[a,b] * x[i-(a-oh), j-(b-ow)]
        (A^H w)[i,j] =             sum_{a,b} K[a,b] * (mask * w)[i+(a-oh), j+(b-ow)]          indices modulo the dimension
    `kernel`: 2-D, or 1-D for a 1-D shape; `origin`: (oh, ow) inside the kernel (an int for a signal), None = (kh // 2, kw // 2);
    `mask`: float64 of the image's shape (a 0/1 mask gives inpainting or subsampled convolution), None = all ones.
    An implicit operator: no matrix is stored, the device convolves directly (fh_set_conv2d, csrc/fh_conv.h: an LDS tile with its halo, a
    sliding register window).  Lazy like the 3-D GradDivMap: the device context is created when the device loop first asks for it, and on
    host arrays the map is exactly `out = zeros; for a: for b: out += K[a,b] * np.roll(x, (a-oh, b-ow), axis=(0,1))` (the adjoint: the
    negated shifts of mask * w) -- the arithmetic the device kernels keep term by term, so `backend="numpy"`, the generic host loop and the
    device agree bit for bit on A x and A^H w.  A kernel the device refuses (more than 16 taps along an axis: `refusal` holds the
    library's sentence) stays a host map: `fasta()` runs it on the generic host loop, and `backend="hip"` raises with that sentence."""

    def __init__(self, shape, kernel, origin=None, mask=None, device=0):
        shape = (int(shape),) if np.ndim(shape) == 0 else tuple(int(k) for k in shape)
        kernel = np.ascontiguousarray(kernel, dtype=np.float64)
        if len(shape) not in (1, 2):
            raise ValueError(f"ConvMap takes an image shape (H, W) or a signal shape (N,); got {len(shape)} dimensions")
        if kernel.ndim != len(shape):
            raise ValueError(f"ConvMap: a {len(shape)}-D shape takes a {len(shape)}-D kernel (got {kernel.ndim} dimensions)")
        if min(shape) < 1 or kernel.size == 0:
            raise ValueError(f"ConvMap takes a non-empty shape and a non-empty kernel (got {shape} and {kernel.shape})")
        self.image_shape = shape
        self.shape2d = shape if len(shape) == 2 else (1, shape[0])
        self.kernel = kernel.reshape((1, -1)) if kernel.ndim == 1 else kernel
        kh, kw = self.kernel.shape
        if origin is None:
            origin = (kh // 2, kw // 2)
        elif len(shape) == 1:
            origin = (0, int(origin if np.ndim(origin) == 0 else origin[0]))
        self.origin = (int(origin[0]), int(origin[1]))
        if not (0 <= self.origin[0] < kh and 0 <= self.origin[1] < kw):
            raise ValueError(f"ConvMap: the origin {self.origin} lies outside the {kh} x {kw} kernel")
        self.mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.float64)
        if self.mask is not None and self.mask.shape != shape:
            raise ValueError(f"mask has shape {self.mask.shape}, a ConvMap on {shape} takes {shape}")
        self.refusal = hip.conv_refusal(self.shape2d[0], self.shape2d[1], kh, kw)      # (a library that does not load raises: only a sentence about the shape is a refusal)
        self.geometry = None if self.refusal is not None else hip.conv_shape(self.shape2d[0], self.shape2d[1], kh, kw)
        _DeviceMap.__init__(self, shape, shape, device, lazy=True)

    def _on_context(self, ctx):
        ctx.set_conv2d(self.shape2d, self.kernel, self.origin, None if self.mask is None else self.mask.reshape(self.shape2d))

    def _rolls(self, v, sign):
        x = np.asarray(v, dtype=np.float64).reshape(self.shape2d)
        out = np.zeros(self.shape2d)
        oh, ow = self.origin
        for a in range(self.kernel.shape[0]):
            for b in range(self.kernel.shape[1]):
                out += self.kernel[a, b] * np.roll(x, (sign * (a - oh), sign * (b - ow)), axis=(0, 1))
        return out

    def _apply_fwd(self, v):
        y = self._rolls(v, 1).reshape(self.image_shape)
        return y if self.mask is None else self.mask * y

    def _apply_adj(self, w):
        w = np.asarray(w, dtype=np.float64).reshape(self.image_shape)
        return self._rolls(w if self.mask is None else self.mask * w, -1).reshape(self.image_shape)
