"""Proximal operators: device-tagged objects + the reference's function names (fasta/proximal.py).

A tagged object bundles `g` and `proxg` of one regulariser and tells `fasta()` which fused device
prox to run (`kind`, `mu`).  Use it for both arguments:

    reg = Shrink(mu);  fasta(A, At, ls.f, ls.gradf, reg.g, reg.prox, x0)

With device-recognised operands `fasta()` never CALLS these objects: it maps the tag to the prox fused
into K-fwd / the one-pass kernel.  Called on a host array -- by a user's closure, by the generic host loop
(generic.py), by the reference itself -- a tag and the module-level functions (`shrink`, `project_Linf_ball`,
`project_L1_ball`, `project_Lnuc_ball`) are ordinary callables with the reference's NumPy semantics
(fasta/proximal.py:12-67), so the reference's `solve()` bodies run unmodified against this module.
`device_prox(tag, x, t)` evaluates the same prox with the DEVICE kernel on a host array, through a scratch
context cached per (device, shape); the -m gpu tests use it to pin the kernels to the reference's known
answers.
"""

import numpy as np

from . import hip

__all__ = ["Shrink", "NonNeg", "LinfProx", "L1Ball", "Box", "TVDualBall", "GroupShrink", "RowBall", "RowSplit", "NuclearShrink", "NuclearBall", "NoProx", "device_prox", "release_scratch",
           "shrink", "project_Linf_ball", "project_L1_ball", "project_Lnuc_ball", "project_nuclear_ball"]


class ProxTag:
    kind = hip.PROX_IDENTITY
    mu = 0.0
    lo = hi = 0.0
    step_scaled = True          # prox parameter is t*mu (True) or mu alone (False, constraint sets)

    def g_from_sums(self, gsum, gmax):
        """g(x) from the device reductions sum|x_i| and max|x_i|."""
        return 0

    # ordinary callables on host arrays (reference semantics); the device loop never calls them ----
    def prox(self, x, t):
        return x

    def __call__(self, x, t):
        return self.prox(x, t)

    def g(self, x):
        return 0

    def prox_on_device(self, x, t, device=0):
        """The fused device prox applied to a host array (scratch context cached per shape)."""
        return device_prox(self, x, t, device)


class NoProx(ProxTag):
    """g = None branch of fasta/__init__.py:88-90 (plain gradient descent)."""


class Shrink(ProxTag):
    """g(x) = mu*||x||_1, proxg(x, t) = shrink(x, t*mu)  (examples/sparse_least_squares.py:43-44)."""
    kind = hip.PROX_SHRINK

    def __init__(self, mu):
        self.mu = float(mu)

    def g_from_sums(self, gsum, gmax):
        return self.mu * gsum

    def prox(self, x, t):
        return shrink(x, t * self.mu)

    def g(self, x):
        return self.mu * np.linalg.norm(np.ravel(x), 1)


class NonNeg(ProxTag):
    """g = 0 on x >= 0, proxg = max(x, 0)  (examples/nn_least_squares.py:41-42)."""
    kind = hip.PROX_NONNEG

    def prox(self, x, t):
        return np.maximum(x, 0)


class LinfProx(ProxTag):
    """g(x) = mu*||x||_inf, proxg(x, t) = project_Linf_ball(x, t*mu)
    (examples/democratic_representation.py:41-42)."""
    kind = hip.PROX_LINF

    def __init__(self, mu):
        self.mu = float(mu)

    def g_from_sums(self, gsum, gmax):
        return self.mu * gmax

    def prox(self, x, t):
        return project_Linf_ball(x, t * self.mu)

    def g(self, x):
        return self.mu * np.linalg.norm(np.ravel(x), np.inf)


class L1Ball(ProxTag):
    """g = 0, proxg(x, t) = project_L1_ball(x, mu) -- radius mu, independent of t (examples/lasso.py:44-45)."""
    kind = hip.PROX_L1BALL
    step_scaled = False

    def __init__(self, mu):
        self.mu = float(mu)

    def prox(self, x, t):
        return project_L1_ball(x, self.mu)


class Box(ProxTag):
    """Clip to [lo, hi] (examples/svm.py:71)."""
    kind = hip.PROX_BOX

    def __init__(self, lo, hi):
        self.lo, self.hi = float(lo), float(hi)

    def prox(self, x, t):
        return np.minimum(np.maximum(x, self.lo), self.hi)


class TVDualBall(ProxTag):
    """Per-pixel projection of 2-vectors onto the unit ball (examples/tv_denoising.py:89-96)."""
    kind = hip.PROX_TVBALL

    def prox(self, Y, t):
        lengths = np.linalg.norm(Y, axis=-1)
        return Y / np.maximum(lengths, 1)[..., None]


class GroupShrink(ProxTag):
    """Row-sparsity regulariser of a matrix unknown X of shape (N, L) (examples/mmv.py:51-59):
    g(X) = mu * (sum over the rows of their Euclidean norms), and proxg(X, t) shrinks every ROW's norm by t*mu -- a row whose norm is
    below t*mu becomes zero, any other row keeps its direction and loses t*mu of its length.  Couples the columns of a row, so the
    device serves it in the multi-column form only (FH_PROX_GROUP, csrc/fh_multi.h)."""
    kind = hip.PROX_GROUP

    def __init__(self, mu):
        self.mu = float(mu)

    def g_from_sums(self, gsum, gmax):
        return self.mu * gsum                   # FH_S_GSUM carries the sum of row norms for this kind

    def prox(self, X, t):
        lengths = np.linalg.norm(X, axis=1)
        # the shrunk length over the old one; an all-zero row is divided by one instead of zero and stays zero
        factor = shrink(lengths, self.mu * t) / (lengths + (lengths == 0))
        return X * factor[:, np.newaxis]

    def g(self, X):
        return self.mu * np.sum(np.sqrt(np.sum(X * X, axis=1)))


class RowBall(ProxTag):
    """Max-norm constraint on a matrix unknown X of shape (N, K) (examples/max_norm.py:51-59): g = 0, and proxg(X, t) brings every ROW whose
    Euclidean norm exceeds mu back to norm mu (rows inside the ball are kept; independent of t).  Couples the columns of a row; the device
    serves it with a quadratic loss only (FH_PROX_ROWBALL, csrc/fh_quad.h)."""
    kind = hip.PROX_ROWBALL
    step_scaled = False

    def __init__(self, mu):
        self.mu = float(mu)

    def prox(self, X, t):
        norms = np.linalg.norm(X, axis=1)
        # Shrink the norms that are too big, and ensure we don't divide by zero
        scale = np.maximum(norms, self.mu) + (norms == 0)
        return self.mu * X / scale[:, np.newaxis]


class RowSplit(ProxTag):
    """Two elementwise terms on one matrix unknown Z = [top; bottom] (examples/nn_factorization.py:59-61): rows [0, split) take the tag `top`
    (NoProx, Shrink, NonNeg or Box), the other rows the tag `bottom` (NoProx, NonNeg or Box: its g must be zero, the l1 term lives on the top
    rows only).  `RowSplit(m, Shrink(mu), Box(0, 1))` is the example's pair.  The device serves it with losses.Factorization only
    (FH_PROX_ROWSPLIT, csrc/fh_bilinear.h)."""
    kind = hip.PROX_ROWSPLIT

    def __init__(self, split, top, bottom):
        if not isinstance(top, ProxTag) or not isinstance(bottom, ProxTag):
            raise ValueError("RowSplit takes two proximal.* tag objects, e.g. RowSplit(m, Shrink(mu), Box(0, 1))")
        if top.kind not in (hip.PROX_IDENTITY, hip.PROX_SHRINK, hip.PROX_NONNEG, hip.PROX_BOX):
            raise ValueError(f"RowSplit: the top rows take NoProx, Shrink, NonNeg or Box (got proximal.{type(top).__name__})")
        if bottom.kind not in (hip.PROX_IDENTITY, hip.PROX_NONNEG, hip.PROX_BOX):
            raise ValueError(f"RowSplit: the bottom rows take NoProx, NonNeg or Box -- a tag whose g is zero (got proximal.{type(bottom).__name__})")
        self.split, self.top, self.bottom = int(split), top, bottom
        self.mu, self.lo, self.hi = top.mu, top.lo, top.hi

    def bind_prox(self, ctx):
        ctx.set_prox_split(self.split, self.top.kind, self.top.mu, self.top.lo, self.top.hi, self.bottom.kind, self.bottom.lo, self.bottom.hi)

    def g_from_sums(self, gsum, gmax):
        return self.top.g_from_sums(gsum, gmax)          # FH_S_GSUM runs over the top rows only for this kind

    def prox(self, Z, t):
        N = self.split
        return np.concatenate((self.top.prox(Z[:N, ...], t), self.bottom.prox(Z[N:, ...], t)))

    def g(self, Z):
        return self.top.g(Z[:self.split, ...])


class NuclearShrink(ProxTag):
    """Low-rank regulariser of a matrix unknown X of shape (M, N) (examples/logistic_matrix_completion.py:44-45): proxg(X, t) soft-thresholds the
    singular values by t*mu, the prox of mu * ||X||_*.  On host arrays `g` and `prox` are the example's closures in the example's own
    arithmetic (a full SVD, the thresholded values on the diagonal of a zero (M, N) matrix, U @ S @ V), so the generic host loop reproduces a
    reference run bit for bit.  NOTE what that arithmetic makes of g: `la.norm(np.diag(s), 1)` is the induced 1-norm of a diagonal MATRIX, its
    largest entry -- the example's objective (and with it the iterate it returns as best) is f + mu * sigma_max(X), not f + mu * ||X||_*.  The
    device reports both norms (FH_S_GSUM: nuclear, FH_S_GMAX: spectral) and `g_from_sums` takes the one the example's `g` evaluates, so that
    device and reference runs agree; `nuclear_norm_from_sums` gives the other.  The device serves it on the identity operator only (FH_PROX_NUCLEAR, csrc/fh_nuclear.h: block
    one-sided Jacobi, no LAPACK), for min(M, N) <= 1024."""
    kind = hip.PROX_NUCLEAR

    def __init__(self, mu):
        self.mu = float(mu)

    def bind_prox(self, ctx, evaluate_objective=True):
        # g is not free at x0 nor at an extrapolated iterate: the values-only decompositions are skipped when nobody reads the objective
        ctx.set_prox_nuclear(self.mu, bool(evaluate_objective))

    def g_from_sums(self, gsum, gmax):
        return self.mu * gmax                   # FH_S_GMAX carries the largest singular value for this kind: what `g` below evaluates

    def nuclear_norm_from_sums(self, gsum, gmax):
        return gsum                             # FH_S_GSUM: the sum of the singular values

    def prox(self, X, t):
        U, s, V = np.linalg.svd(X)
        S = np.zeros(X.shape)
        S[:len(s), :len(s)] = np.diag(shrink(s, t * self.mu))
        return U @ S @ V

    def g(self, X):
        return self.mu * np.linalg.norm(np.diag(np.linalg.svd(X)[1]), 1)


class NuclearBall(ProxTag):
    """Low-rank CONSTRAINT on a matrix unknown X of shape (M, N): g = 0 on { ||X||_* <= radius }, and proxg(X, t) is the Euclidean projection onto that
    ball, independent of t -- the singular values are projected onto the l1 ball of that radius (project_L1_ball), the singular vectors kept.  On host
    arrays `prox` is LAPACK's thin SVD; the device serves it on the identity operator only (FH_PROX_NUCBALL, csrc/fh_nuclear.h: the Jacobi
    decomposition of NuclearShrink and a one-workgroup launch that finds the level), for min(M, N) <= 1024.  (The reference's `project_Lnuc_ball`
    is, despite its name, the soft-threshold: NuclearShrink.)"""
    kind = hip.PROX_NUCBALL
    step_scaled = False

    def __init__(self, radius):
        radius = float(radius)
        if not (radius >= 0 and np.isfinite(radius)):
            raise ValueError(f"NuclearBall needs a finite radius >= 0 (got {radius!r})")
        self.radius = self.mu = radius

    def nuclear_norm_from_sums(self, gsum, gmax):
        return gsum                             # FH_S_GSUM after a forward launch: the sum of the singular values of xprox

    def prox(self, X, t):
        return project_nuclear_ball(X, self.radius)


# ---- the device prox on host arrays -----------------------------------------------------------------
_scratch = {}           # (device, "dense", n) or (device, "tv", H, W) -> operator holding a scratch HipContext


_ELEMENTWISE = (hip.PROX_IDENTITY, hip.PROX_SHRINK, hip.PROX_NONNEG, hip.PROX_BOX)


def _matrix_form(tag, x):
    """Does device_prox take the multi-column kernels for `x`?  GroupShrink always (it couples the columns of a row, and refuses what the
    device cannot hold); an elementwise kind for a 2-D array of at most 16 columns -- same bits as the vector kernels on the flattened
    array.  Everything else (LinfProx / L1Ball on any shape, wider arrays, other ranks) is flattened and takes the vector kernels."""
    if tag.kind == hip.PROX_ROWSPLIT:
        raise ValueError("RowSplit runs on the device with losses.Factorization only: device_prox has no scratch operator for it")
    if tag.kind == hip.PROX_ROWBALL:
        raise ValueError("RowBall runs on the device with a quadratic loss only (losses.Quadratic): device_prox has no scratch operator for it")
    if tag.kind == hip.PROX_GROUP:
        if x.ndim != 2 or x.shape[1] > hip.MAX_RHS:
            raise ValueError(f"GroupShrink needs a 2-D array of at most {hip.MAX_RHS} columns (got shape {x.shape})")
        return True
    return tag.kind in _ELEMENTWISE and x.ndim == 2 and 1 <= x.shape[1] <= hip.MAX_RHS


def _scratch_op(device, x, tv, matrix=False):
    """One scratch operator per (device, shape), kept for the life of the process (`release_scratch()` frees them):
    a prox inside a caller's loop costs two small copies and one launch, not a context create/destroy."""
    from .linalg import DenseMatrixMap, GradDivMap
    rhs = x.shape[1] if matrix else None                         # a matrix unknown: (n, L) on a one-row operator with rhs = L
    key = (device, "tv") + tuple(x.shape[:2]) if tv else ((device, "dense", x.size) if rhs is None else (device, "dense") + tuple(x.shape))
    op = _scratch.get(key)
    if op is None:
        if len(_scratch) >= 8:                                   # bounded: drop the oldest shape
            _scratch.pop(next(iter(_scratch))).close()
        if tv:
            op = GradDivMap(x.shape[:2], device=device)
        elif rhs is None:
            op = DenseMatrixMap(np.zeros((1, x.size)), device=device)
        else:
            op = DenseMatrixMap(np.zeros((1, x.shape[0])), device=device, rhs=rhs)
        if not tv:
            op.ctx.set_loss_lsq(np.zeros(1 if rhs is None else rhs))
            op.ctx.set_vector(hip.VEC_G0, np.zeros(x.size))
        _scratch[key] = op
    return op


def release_scratch():
    """Free the cached scratch contexts of `device_prox`."""
    while _scratch:
        _scratch.popitem()[1].close()


def device_prox(tag, x, t, device=0):
    """prox_{t g}(x) for a host array through the DEVICE kernels: one K-fwd with x0 := x and a zero gradient
    gives xprox = prox(x, t).  GroupShrink takes a 2-D `x` of shape (n, L), L <= 16, and the multi-column kernels; so does an elementwise
    tag on such an array (same bits as on the flattened array).  Every other call is flattened and takes the vector kernels."""
    x = np.asarray(x, dtype=np.float64)
    flat = x.ravel()
    if tag.kind in (hip.PROX_NUCLEAR, hip.PROX_NUCBALL):
        return _device_prox_nuclear(tag, x, t, device)
    tv = tag.kind == hip.PROX_TVBALL
    if tv:
        assert x.ndim == 3 and x.shape[-1] == 2
    ctx = _scratch_op(device, x, tv, matrix=not tv and _matrix_form(tag, x)).ctx
    ctx.set_prox(tag.kind, tag.mu, tag.lo, tag.hi)
    ctx.set_vector(hip.VEC_X0, flat)
    if tv:
        # the stencil path recomputes g0 = grad(A x0 - b); with b := A x it is exactly zero, so xhat = x
        ctx.set_loss_lsq(ctx.apply(flat))
        ctx.init()
    ctx.fwd(float(t))
    return ctx.get_vector(hip.VEC_XPROX, flat.size).reshape(x.shape)


def _device_prox_nuclear(tag, x, t, device):
    """NuclearShrink / NuclearBall through a scratch identity context (csrc/fh_nuclear.h), cached per (device, M, N) like the others."""
    from .linalg import IdentityMap
    if x.ndim != 2:
        raise ValueError(f"{type(tag).__name__} needs a 2-D array (got shape {x.shape})")
    key = (device, "identity") + tuple(x.shape)
    op = _scratch.get(key)
    if op is None:
        if len(_scratch) >= 8:
            _scratch.pop(next(iter(_scratch))).close()
        op = IdentityMap(x.shape, device=device)
        op.ctx.set_loss_lsq(np.zeros(x.size))
        _scratch[key] = op
    ctx = op.ctx
    if tag.kind == hip.PROX_NUCBALL:
        ctx.set_prox(tag.kind, tag.mu)
    else:
        tag.bind_prox(ctx, False)
    ctx.set_vector(hip.VEC_X0, x)
    ctx.set_vector(hip.VEC_G0, np.zeros(x.size))
    ctx.fwd(float(t))
    return ctx.get_vector(hip.VEC_XPROX, x.size).reshape(x.shape)


# ---- the reference's function names (host arrays, NumPy) ------------------------------------------------
def shrink(x, t):
    """Soft-threshold by t (fasta/proximal.py:58-67); small negatives come back as -0.0, as in the reference."""
    return np.sign(x) * np.maximum(np.abs(x) - t, 0)


def project_Linf_ball(x, t):
    """The prox of t*||.||_inf, as the reference implements it (fasta/proximal.py:12-31): clip |x| at the level
    alpha = max_k (sum of the k largest |x_i| - t)/k, or return float64 zeros when that level is not positive.  An image (linalg.ConvMap) is
    projected as the vector of its entries and comes back in its shape."""
    if np.ndim(x) > 1:
        return project_Linf_ball(np.ravel(x), t).reshape(np.shape(x))
    mags = np.abs(x)
    ranked = mags.copy()
    ranked[::-1].sort()                                          # descending, in place through the reversed view
    alpha = np.max((np.cumsum(ranked) - t) / np.arange(1, len(x) + 1))
    if alpha > 0:
        return np.minimum(mags, alpha) * np.sign(x)
    return np.zeros(len(x))


def project_L1_ball(x, t):
    """Euclidean projection onto {||x||_1 <= t} by Moreau's identity (fasta/proximal.py:34-41)."""
    return x - project_Linf_ball(x, t)


def project_Lnuc_ball(X, t):
    """Soft-threshold the singular values of X by t (fasta/proximal.py:44-55), by LAPACK's thin SVD on the host.  The device's form is
    NuclearShrink on the identity operator (FH_PROX_NUCLEAR, csrc/fh_nuclear.h), which the -m gpu tests hold to this function."""
    U, s, Vh = np.linalg.svd(X, full_matrices=False)
    return (U * shrink(s, t)) @ Vh


def project_nuclear_ball(X, radius):
    """Euclidean projection onto {||X||_* <= radius}: LAPACK's thin SVD on the host, the singular values projected onto the l1 ball of that radius.
    The device's form is NuclearBall on the identity operator (FH_PROX_NUCBALL, csrc/fh_nuclear.h), which the -m gpu tests hold to this function."""
    U, s, Vh = np.linalg.svd(X, full_matrices=False)
    s = project_L1_ball(s, radius)
    return (U * s) @ Vh
