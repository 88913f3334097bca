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
"""

from collections import namedtuple

import numpy as np

from .linalg import is_sparse_matrix
from .losses import LeastSquares, LogisticLoss
from .proximal import GroupShrink, Shrink

__all__ = ["Certificate", "duality_gap", "critical_mu", "certificate_from_parts", "logistic_dual_terms", "logistic_loss_terms", "LN2"]

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
