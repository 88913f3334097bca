"""Duality-gap certificates for  min_x f(A x) + mu * Omega(x):  the host statement of what `HipContext.dual_gap()` (fh_dual_gap,
csrc/fh_gap.h) evaluates on the device, in plain NumPy, with the same expression per term as the kernel.

With z = A x and g = A^H grad f(z):
    Omega(x) = sum |x_ij|, dual norm Omega°(g) = max |g_ij|                       (proximal.Shrink)
    Omega(x) = sum_j ||x_j,:||_2, dual norm Omega°(g) = max_j ||g_j,:||_2         (proximal.GroupShrink; row norms summed in column order)
    s = 1 if Omega°(g) <= mu else mu / Omega°(g);  u = s * grad f(z) is dual feasible
    P = f(z) + mu * Omega(x),  D = -f*(u),  gap = P - D >= 0  bounds  P - min P.
LeastSquares(b), r = z - b:  D = -.5 s^2 ||r||^2 - s <r, b>,  f(0) = .5 ||b||^2.
LogisticLoss(b), f(z) = sum log(1 + e^z) - y z with y = [b == 1]:  D = -sum h(y_i + s (sigma(z_i) - y_i)),  h(p) = p log p + (1 - p) log(1 - p)
with 0 log 0 = 0, evaluated without cancellation (y = 1: q = s sigma(-z), h = (1 - q) log1p(-q) + q log q; y = 0: the same in p = s sigma(z));
f(0) = m log 2.  At x = 0 the record's dual norm is the critical mu: for every mu at or above it the gap at 0 is exactly 0.

Gap-safe screening (`screen`; on the device fh_screen, csrc/fh_screen.h), least squares only.  With norms2_j = sum_i a_ij^2 (rows in index order):
    gap_safe = gap + kappa * eps * (P + f + 2 sqrt(f f0)),  rho = sqrt(2 gap_safe)
    feature j is zero at every solution when each of its L entries has  (s |g_jl| + rho sqrt(norms2_j)) (1 + 2^-48) < mu
(GroupShrink: s ||g_j,:||_2 in place of s |g_jl|).  The second term of gap_safe bounds what rounding can take from the computed gap:
kappa = `screen_kappa`, the longest addition chain of the certificate's sums.  At x = 0 with s = 1 the gap is zero as an identity (r = -b makes P and
D the same sums) and the radius is 0.  One rounded operation per term, nothing contracted: on exactly representable data the device agrees with ==.
"""

from collections import namedtuple

import numpy as np

from .linalg import is_sparse_matrix
from .losses import LeastSquares, LogisticLoss
from .proximal import GroupShrink, Shrink

__all__ = ["Certificate", "duality_gap", "critical_mu", "certificate_from_parts", "logistic_dual_terms", "logistic_loss_terms", "LN2",
           "Screen", "screen", "screen_from_parts", "screen_kappa", "gap_safe", "column_norms2", "SCREEN_ONE_PLUS"]

LN2 = 0.6931471805599453          # log(2) rounded to nearest (csrc/fh_gap.h: FH_GAP_LN2)


class Certificate(namedtuple("Certificate", "primal dual gap f omega dual_norm scale f0")):
    """primal P, dual D, gap = P - D, f = f(z), omega = Omega(x), dual_norm = Omega°(g), scale = s, f0 = f(0): the order of fh_dual_gap's output."""
    __slots__ = ()

    @property
    def relative(self):
        """gap / f(0): what stopping.DualityGap compares with its tolerance."""
        return self.gap / self.f0


def _tags(loss, prox):
    """(loss tag, prox tag) or TypeError with a sentence; bound methods of a tag (`ls.f`, `reg.prox`) count as the tag."""
    loss = getattr(loss, "__self__", loss)
    prox = getattr(prox, "__self__", prox)
    if type(loss) not in (LeastSquares, LogisticLoss):
        raise TypeError(f"duality_gap: the certificate is stated for losses.LeastSquares and losses.LogisticLoss (got {type(loss).__name__})")
    if type(prox) not in (Shrink, GroupShrink):
        raise TypeError(f"duality_gap: the certificate is stated for proximal.Shrink and proximal.GroupShrink (got {type(prox).__name__})")
    if loss.weights is not None:
        raise TypeError("duality_gap: a loss with observation weights has no certificate here")
    if not prox.mu > 0:
        raise TypeError(f"duality_gap: the certificate needs mu > 0 (got mu = {prox.mu!r})")
    return loss, prox


def _apply(A, x, adjoint=False):
    if isinstance(A, np.ndarray) or is_sparse_matrix(A):
        return (A.T if adjoint else A) @ x
    if adjoint:
        if not hasattr(A, "H"):
            raise TypeError("duality_gap: A must be an ndarray, a scipy.sparse matrix or a map with A(x) and A.H(w)")
        H = A.H
        return H(x) if callable(H) else H @ x
    if not callable(A):
        raise TypeError("duality_gap: A must be an ndarray, a scipy.sparse matrix or a map with A(x) and A.H(w)")
    return A(x)


def _rows(v):
    """An (n, L) view: a vector is one column."""
    v = np.asarray(v, dtype=np.float64)
    return v.reshape(v.shape[0], -1) if v.ndim else v.reshape(1, 1)


def _row_norms(V):
    acc = np.zeros(V.shape[0])
    for l in range(V.shape[1]):                  # column index order, a rounded product and a rounded sum per column: the kernel's order
        acc = acc + V[:, l] * V[:, l]
    return np.sqrt(acc)


def _xlog(a, log_a):
    with np.errstate(invalid="ignore"):
        return np.where(a == 0.0, 0.0, a * log_a)


def logistic_dual_terms(z, b, s):
    """h(y_i + s (sigma(z_i) - y_i)) per row, without cancellation: the smaller of p and 1 - p is formed directly."""
    z, b = np.ravel(np.asarray(z, dtype=np.float64)), np.ravel(np.asarray(b, dtype=np.float64))
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        e = np.exp(np.where(b == 1.0, z, -z))
        q = s * (1.0 / (1.0 + e))
        r = 1.0 - q
        return _xlog(r, np.log1p(-q)) + _xlog(q, np.log(q))


def logistic_loss_terms(z, b):
    """log(1 + e^z) - [b == 1] z per row, the expression of the loss kernels (csrc/fh_device.h: loss_term)."""
    z, b = np.ravel(np.asarray(z, dtype=np.float64)), np.ravel(np.asarray(b, dtype=np.float64))
    with np.errstate(over="ignore"):
        return np.log(1.0 + np.exp(z)) - np.where(b == 1.0, z, 0.0)


def _scale(dual_norm, mu):
    return 1.0 if dual_norm <= mu else mu / dual_norm


def certificate_from_parts(x, g, z, loss, prox):
    """The certificate from x, g = A^H grad f(z) and z = A x as given (vectors read back from a device context, say): no operator is applied."""
    loss, prox = _tags(loss, prox)
    mu = float(prox.mu)
    X, G = _rows(x), _rows(g)
    if X.shape != G.shape:
        raise TypeError(f"duality_gap: x has shape {X.shape}, the gradient {G.shape}")
    z = np.asarray(z, dtype=np.float64)
    if z.shape != loss.b.shape:
        raise TypeError(f"duality_gap: A x has shape {z.shape}, the loss holds b of shape {loss.b.shape}")
    if type(prox) is GroupShrink:
        omega = float(np.sum(_row_norms(X)))
        dual_norm = float(np.max(_row_norms(G), initial=0.0))
    else:
        omega = float(np.sum(np.abs(X)))
        dual_norm = float(np.max(np.abs(G), initial=0.0))
    s = _scale(dual_norm, mu)
    b = loss.b
    if type(loss) is LogisticLoss:
        f = float(np.sum(logistic_loss_terms(z, b)))
        dual = -float(np.sum(logistic_dual_terms(z, b, s)))
        f0 = float(b.size) * LN2
    else:
        r = (z - b).ravel()
        rr, rb, bb = float(r @ r), float(r @ b.ravel()), float(b.ravel() @ b.ravel())
        f = 0.5 * rr
        dual = -((0.5 * (s * s)) * rr) - s * rb
        f0 = 0.5 * bb
    primal = f + mu * omega
    return Certificate(primal, dual, primal - dual, f, omega, dual_norm, s, f0)


def duality_gap(A, loss, prox, x):
    """The certificate of x for min f(A x) + mu * Omega(x) on host arrays.  A: an ndarray, a scipy.sparse matrix or any map with A(x) / A.H(w);
    loss: a tagged LeastSquares or LogisticLoss (no weights); prox: a tagged Shrink or GroupShrink with mu > 0.  Anything else: TypeError."""
    loss, prox = _tags(loss, prox)
    x = np.asarray(x, dtype=np.float64)
    z = np.asarray(_apply(A, x), dtype=np.float64)
    if z.shape != loss.b.shape:
        raise TypeError(f"duality_gap: A x has shape {z.shape}, the loss holds b of shape {loss.b.shape}")
    g = np.asarray(_apply(A, loss.gradf(z), adjoint=True), dtype=np.float64)
    return certificate_from_parts(x, g, z, loss, prox)


def critical_mu(A, loss, prox_class, shape):
    """Omega°(A^H grad f(0)): the smallest mu at which x = 0 solves the problem, for an unknown of the given shape."""
    if prox_class not in (Shrink, GroupShrink):
        raise TypeError(f"critical_mu: the certificate is stated for proximal.Shrink and proximal.GroupShrink (got {getattr(prox_class, '__name__', prox_class)!r})")
    shape = (shape,) if isinstance(shape, (int, np.integer)) else tuple(shape)
    return duality_gap(A, loss, prox_class(1.0), np.zeros(shape)).dual_norm


# ---- gap-safe screening ---------------------------------------------------------------------------------------------------------------------
Screen = namedtuple("Screen", "keep radius certificate norms2")      # keep: n booleans (True = the feature stays); radius = rho
SCREEN_ONE_PLUS = 1.0 + 2.0 ** -48
_EPS = 2.0 ** -52


def _gap_slabs(rows):
    """The slab rule of k_gap_partials (csrc/fasta_hip.hip: gap_slabs): (workgroups, rows per slab) of one side."""
    k = min(max((rows + 255) // 256, 1), 256)
    return k, ((rows + k - 1) // k + 63) // 64 * 64


def screen_kappa(m, n, L=1):
    """The longest addition chain of the certificate's sums for an (m, n) operator and L columns: terms per lane, the depth of block_reduce
    (10), records per lane in add_records, 8 for the closing arithmetic -- the mirror of fh_screen_shape_for's last entry (csrc/fh_screen.h)."""
    (nwg_n, slab_n), (nwg_m, slab_m) = _gap_slabs(int(n)), _gap_slabs(int(m))
    terms = (max(slab_n, slab_m) + 255) // 256 * max(int(L), 1)
    return terms + 10 + (nwg_n + nwg_m + 255) // 256 + 8


def gap_safe(cert, kappa):
    """gap + kappa * eps * (P + f + 2 sqrt(f f0)), never below 0; exactly 0 at x = 0 inside the dual ball.  One rounded operation per line."""
    if cert.omega == 0.0 and cert.scale == 1.0:
        return 0.0
    t1 = cert.f * cert.f0
    t2 = float(np.sqrt(t1))
    t3 = 2.0 * t2
    t4 = cert.primal + cert.f
    t5 = t4 + t3
    ke = float(kappa) * _EPS
    t6 = ke * t5
    t7 = cert.gap + t6
    return max(t7, 0.0)


def _columns_of(A):
    """The stored matrix behind A (an ndarray or a scipy.sparse matrix), or TypeError with a sentence."""
    if isinstance(A, np.ndarray) or is_sparse_matrix(A):
        return A
    M = getattr(A, "matrix", None)
    if M is not None and (isinstance(M, np.ndarray) or is_sparse_matrix(M)):
        return A._host_matrix() if hasattr(A, "_host_matrix") else M
    raise TypeError("screen: A must be an ndarray, a scipy.sparse matrix or a map that holds its matrix (A.matrix): a general map cannot give its columns")


def column_norms2(A):
    """sum_i a_ij^2 per column, rows added in index order (a sparse matrix: its stored entries in row order)."""
    A = _columns_of(A)
    if is_sparse_matrix(A):
        S = A.tocsc()
        S.sort_indices()
        ptr, val = S.indptr, np.asarray(S.data, dtype=np.float64)
        acc = np.zeros(S.shape[1])
        lens = np.diff(ptr)
        for k in range(int(lens.max()) if lens.size else 0):
            sel = np.nonzero(lens > k)[0]
            v = val[ptr[sel] + k]
            acc[sel] = acc[sel] + v * v
        return acc
    A = np.asarray(A, dtype=np.float64)
    acc = np.zeros(A.shape[1])
    for i in range(A.shape[0]):
        acc = acc + A[i] * A[i]
    return acc


def screen_from_parts(cert, g, norms2, prox, kappa):
    """The test from a certificate, g = A^H (A x - b) and norms2 as given: (keep, rho).  One rounded operation per term."""
    prox = getattr(prox, "__self__", prox)
    mu = float(prox.mu)
    G = _rows(g)
    rho = float(np.sqrt(2.0 * gap_safe(cert, kappa)))
    d = rho * np.sqrt(np.asarray(norms2, dtype=np.float64))
    s = cert.scale
    if type(prox) is GroupShrink:
        a = s * _row_norms(G)
        discard = (a + d) * SCREEN_ONE_PLUS < mu
    else:
        a = s * np.abs(G)
        discard = np.all((a + d[:, None]) * SCREEN_ONE_PLUS < mu, axis=1)
    return ~discard, rho


def screen(A, loss, prox, x, norms2=None):
    """The gap-safe test at x for min .5 ||A x - b||^2 + mu * Omega(x): Screen(keep, radius, certificate, norms2).  A feature with keep False is zero
    at every solution.  A: an ndarray, a scipy.sparse matrix or a map that holds its matrix; loss: a tagged LeastSquares (no weights); prox: a tagged
    Shrink or GroupShrink with mu > 0.  norms2: column_norms2(A) if the caller already has it.  Anything else: TypeError."""
    loss, prox = _tags(loss, prox)
    if type(loss) is not LeastSquares:
        raise TypeError("screen: the screening radius is stated for losses.LeastSquares (the constant of the logistic loss differs)")
    M = _columns_of(A)
    x = np.asarray(x, dtype=np.float64)
    z = np.asarray(M @ x, dtype=np.float64)
    if z.shape != loss.b.shape:
        raise TypeError(f"screen: A x has shape {z.shape}, the loss holds b of shape {loss.b.shape}")
    g = np.asarray(M.T @ loss.gradf(z), dtype=np.float64)
    cert = certificate_from_parts(x, g, z, loss, prox)
    if norms2 is None:
        norms2 = column_norms2(M)
    L = x.shape[1] if x.ndim == 2 else 1
    keep, rho = screen_from_parts(cert, g, norms2, prox, screen_kappa(M.shape[0], M.shape[1], L))
    return Screen(keep, rho, cert, norms2)
