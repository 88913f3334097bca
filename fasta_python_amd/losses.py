"""Smooth terms f(z) recognised by the device loop.

LogisticLoss(b), SoftmaxLoss(y), Quadratic(Q, c), Factorization(S): see the classes.  LeastSquares(b):  f(z) = .5*||z - b||^2,  gradf(z) = z - b   (examples/sparse_least_squares.py:41-42,
same closures in lasso.py:42-43, nn_least_squares.py:39-40, tv_denoising.py:85-86 with b = M/mu).
Pass `ls.f` and `ls.gradf` as the `f` / `gradf` arguments of `fasta()`.
"""

import math

import numpy as np

__all__ = ["LeastSquares", "LogisticLoss", "SoftmaxLoss", "Quadratic", "Factorization"]


def _checked_weights(name, b, weights):
    """The observation weights of an elementwise loss as a float64 array of b's shape (a boolean mask becomes 0.0 / 1.0), or ValueError with a
    sentence that names the first offending entry."""
    W = np.asarray(weights)
    if W.shape != b.shape:
        raise ValueError(f"{name}: weights must have B's shape {b.shape} (got {W.shape})")
    if W.dtype.kind not in "biuf":
        raise ValueError(f"{name}: weights must be real numbers or a boolean mask (got dtype {W.dtype})")
    W = np.ascontiguousarray(W, dtype=np.float64)
    bad = ~(np.isfinite(W) & (W >= 0))
    if bad.any():
        at = tuple(int(k) for k in np.argwhere(bad)[0])
        raise ValueError(f"{name}: weights must be finite and >= 0 (entry {at if len(at) != 1 else at[0]} is {float(W[at])!r})")
    return W


class LeastSquares:
    """f(z) = .5*||z - b||^2; with `weights` W (an array of b's shape, finite and >= 0, or a boolean mask): f(z) = .5 * sum W * (z - b)^2,
    gradf(z) = W * (z - b) -- matrix completion from a subset of the entries.  The device serves weights on the identity operator only
    (fasta(None, None, ls.f, ls.gradf, ...), fh_set_loss_weights)."""

    def __init__(self, b, weights=None):
        self.b = np.ascontiguousarray(b, dtype=np.float64)
        self.weights = None
        if weights is not None:
            self.weights = _checked_weights("LeastSquares", self.b, weights)
            self._sqrtW = np.sqrt(self.weights)
            self.f, self.gradf = self._f_weighted, self._gradf_weighted      # (instance attributes: `ls.f.__self__` is still the tag)

    def bind(self, ctx):
        ctx.set_loss_lsq(self.b)
        if self.weights is not None:
            ctx.set_loss_weights(self.weights)

    @staticmethod
    def f_from_device(s):
        """f1 from the device scalar sum (z-b)^2: .5*la.norm(z-b)**2 (sparse_least_squares.py:41)."""
        return .5 * np.float64(math.sqrt(s)) ** 2          # (math.sqrt: same IEEE result, a fraction of np.sqrt's call cost)

    # The device loop evaluates f inside its kernels and never calls these.  On host arrays they are the reference's
    # closures (sparse_least_squares.py:41-42), bit for bit, so the generic host loop -- or the reference -- can use them.
    def f(self, z):
        return .5 * np.linalg.norm((z - self.b).ravel()) ** 2

    def gradf(self, z):
        return z - self.b

    def _f_weighted(self, z):
        return .5 * np.linalg.norm((self._sqrtW * (z - self.b)).ravel()) ** 2

    def _gradf_weighted(self, z):
        return self.weights * (z - self.b)

    def __call__(self, z):
        return self.f(z)


class LogisticLoss:
    """f(z) = sum log(1+exp(z)) - (b==1)*z, gradf(z) = -b/(1+exp(b*z)) with labels b in {-1,+1}
    (examples/sparse_logistic.py:47-48).  Dense operators only.  With `weights` W (as for LeastSquares): f(z) = sum W * (log(1+exp(z)) - (b==1)*z),
    gradf(z) = W * (-b/(1+exp(b*z))), on the identity operator only."""

    def __init__(self, b, weights=None):
        self.b = np.ascontiguousarray(b, dtype=np.float64)
        self.weights = None
        if weights is not None:
            self.weights = _checked_weights("LogisticLoss", self.b, weights)
            self.f, self.gradf = self._f_weighted, self._gradf_weighted

    def bind(self, ctx):
        ctx.set_loss_logistic(self.b)
        if self.weights is not None:
            ctx.set_loss_weights(self.weights)

    @staticmethod
    def f_from_device(s):
        return np.float64(s)

    def f(self, z):
        return np.sum(np.log(1 + np.exp(z)) - (self.b == 1) * z)

    def gradf(self, z):
        return -self.b / (1 + np.exp(self.b * z))

    # (the select, as in the kernels: log(1 + exp(z)) is inf above z = 709.8 and 0 * inf is NaN -- an unobserved entry contributes exactly 0.0
    # whatever z is; where W != 0 these are W * term and W * grad, bit for bit)
    def _f_weighted(self, z):
        W = self.weights
        with np.errstate(over="ignore", invalid="ignore"):
            return np.sum(np.where(W == 0, 0.0, W * (np.log(1 + np.exp(z)) - (self.b == 1) * z)))

    def _gradf_weighted(self, z):
        W = self.weights
        with np.errstate(over="ignore", invalid="ignore"):
            return np.where(W == 0, 0.0, W * (-self.b / (1 + np.exp(self.b * z))))

    def __call__(self, z):
        return self.f(z)


class SoftmaxLoss:
    """Multinomial logistic loss over a MATRIX unknown: Z = A X is (m, L), one column per class, y integer labels in {0 .. L-1}^m,
    f(Z) = sum_i [logsumexp(Z_i,:) - Z_i,y_i], gradf(Z) = softmax(Z) - Y with Y the one-hot matrix of y.  With proximal.Shrink: sparse
    weights; with proximal.GroupShrink: a feature kept or dropped for all classes at once (the "grouped" multinomial of glmnet).
    On the device a dense or sparse operator in its matrix form serves it (csrc/fh_softmax.h); 2 to 16 classes.

    The arithmetic of a row z is fixed, the same here and in the kernel: mx = max_l z_l, e_l = exp(z_l - mx), s = e_0 + e_1 + ... + e_{L-1}
    with the columns added in index order, term = (mx + log(s)) - z_y, grad_l = e_l / s - Y_l.  The maximum is always subtracted, so
    z = (800, -800) gives (1, 0) and a finite loss.  (The row sums are formed column by column and not by `.sum(axis=1)`, whose
    pairwise blocks add eight or more columns in another order.)"""

    MAX_CLASSES = 16

    def __init__(self, y, classes=None):
        raw = np.asarray(y)
        if raw.ndim != 1 or raw.size == 0:
            raise ValueError(f"SoftmaxLoss needs a non-empty 1-D array of integer class labels (got shape {raw.shape})")
        if raw.dtype.kind not in "iu":
            raise ValueError(f"SoftmaxLoss needs integer class labels (got dtype {raw.dtype})")
        if int(raw.min()) < 0:
            raise ValueError(f"SoftmaxLoss labels must be >= 0 (entry {int(np.argmax(raw < 0))} is {int(raw.min())})")
        top = int(raw.max())
        if classes is None:
            classes = top + 1
        classes = int(classes)
        if not 2 <= classes <= self.MAX_CLASSES:
            raise ValueError(f"SoftmaxLoss serves 2 to {self.MAX_CLASSES} classes (got {classes})")
        if top >= classes:
            raise ValueError(f"SoftmaxLoss labels must be below classes = {classes} (entry {int(np.argmax(raw >= classes))} is {top})")
        self.y = np.ascontiguousarray(raw, dtype=np.int64)
        self.classes = classes
        self._rows = np.arange(self.y.size)
        self.Y = np.zeros((self.y.size, classes))
        self.Y[self._rows, self.y] = 1.0
        self.b = self.Y                         # what the device holds in FH_VEC_B: the shape the solver checks against the operator

    def bind(self, ctx):
        ctx.set_loss_softmax(self.y)

    @staticmethod
    def f_from_device(s):
        return np.float64(s)                    # FH_S_FSQ carries f itself

    def _rows_of(self, Z):
        Z = np.asarray(Z, dtype=np.float64)
        if Z.shape != self.Y.shape:
            raise ValueError(f"SoftmaxLoss: Z has shape {Z.shape}, the labels need {self.Y.shape}")
        mx = Z.max(axis=1)
        E = np.exp(Z - mx[:, np.newaxis])
        s = E[:, 0].copy()
        for l in range(1, self.classes):        # columns in index order
            s += E[:, l]
        return Z, mx, E, s

    def f(self, Z):
        Z, mx, _, s = self._rows_of(Z)
        return np.sum((mx + np.log(s)) - Z[self._rows, self.y])

    def gradf(self, Z):
        _, _, E, s = self._rows_of(Z)
        return E / s[:, np.newaxis] - self.Y

    __call__ = f


class Quadratic:
    """f(x) = .5*<x, Q x> + <c, x>, gradf(x) = Q x + c on a SYMMETRIC float64 matrix Q, which may be indefinite; x is a vector (n,) or a
    matrix (n, L), c has x's shape or is None.  The operator is the identity: `fasta(None, None, q.f, q.gradf, g, prox, x0)`.  Covers
    examples/max_norm.py:49-50 (Q = S + S.T: sum(S * (X @ X.T)) = .5*<X, Q X>) and the dual of examples/svm.py:68-69
    (Q = (l l^T) * (D D^T), c = -1), box-constrained QP and kernel-SVM duals in general.  On the device one product W = Q x gives both the
    value and the gradient (csrc/fh_quad.h); on host arrays `f` / `gradf` are the closures below."""

    def __init__(self, Q, c=None):
        Q = np.asarray(Q)
        if Q.ndim != 2 or Q.shape[0] != Q.shape[1]:
            raise ValueError(f"Quadratic needs a square matrix Q (got shape {Q.shape})")
        if Q.dtype != np.float64:
            raise ValueError(f"Quadratic needs a float64 matrix Q (got {Q.dtype})")
        if not np.array_equal(Q, Q.T):
            i, j = (int(k) for k in np.argwhere(Q != Q.T)[0])
            raise ValueError(f"Quadratic needs an exactly symmetric Q: Q[{i},{j}] = {float(Q[i, j])!r} but Q[{j},{i}] = {float(Q[j, i])!r} "
                             "(pass (Q + Q.T) / 2, or S + S.T as examples/max_norm.py:50 does)")
        self.Q = Q
        self.c = None if c is None else np.ascontiguousarray(c, dtype=np.float64)

    def bind(self, ctx):
        """Nothing to do: Q and c reach the device with the operator (linalg.QuadraticMap: fh_set_quadratic is operator and loss in one call)."""

    @staticmethod
    def f_from_device(s):
        return np.float64(s)                    # FH_S_FSQ carries f itself

    def f(self, x):
        v = .5 * np.sum(x * (self.Q @ x))
        return v if self.c is None else v + np.sum(self.c * x)

    def gradf(self, x):
        w = self.Q @ x
        return w if self.c is None else w + self.c

    __call__ = f


class Factorization:
    """f(Z) = .5*||S - X Y^T||_F^2 with Z = [X; Y]: X = Z[:m] is (m, K), Y = Z[m:] is (n, K), S a 2-D float64 matrix (m, n)
    (examples/nn_factorization.py:48-57).  gradf(Z) = [d Y; d^T X] with d = X Y^T - S.  The smooth term is BILINEAR in (X, Y), so the
    problem is not convex; the operator is the identity: `fasta(None, None, fz.f, fz.gradf, g, prox, Z0)`.  On the device one pass over S
    gives the value and both halves of the gradient (csrc/fh_bilinear.h); on host arrays `f` / `gradf` are the example's closures."""

    def __init__(self, S):
        S = np.asarray(S)
        if S.ndim != 2:
            raise ValueError(f"Factorization needs a 2-D matrix S (got shape {S.shape})")
        if S.dtype != np.float64:
            raise ValueError(f"Factorization needs a float64 matrix S (got {S.dtype})")
        self.S = S
        self.m, self.n = S.shape

    def bind(self, ctx):
        """Nothing to do: S reaches the device with the operator (linalg.BilinearMap: fh_set_factorization is operator and loss in one call)."""

    @staticmethod
    def f_from_device(s):
        return np.float64(s)                    # FH_S_FSQ carries f itself

    def f(self, Z):
        N = self.m
        return .5 * np.linalg.norm((self.S - Z[:N, ...] @ Z[N:, ...].T).ravel())**2

    def gradf(self, Z):
        N = self.m
        X = Z[:N, ...]
        Y = Z[N:, ...]
        d = X @ Y.T - self.S
        return np.concatenate((d @ Y, d.T @ X))

    __call__ = f
