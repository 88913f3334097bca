"""Standardised features and the way back: the host statement of fh_standardize (csrc/fh_standardize.h) and the map from the coefficients of the
standardised problem to the caller's units.

    A_std, st = standardize(A)                       # columns of mean 0 and root-mean-square 1
    x = solve(A_std, b - b.mean())                   # any solver of this package
    beta, beta0 = st.coefficients(x), st.intercept(x, b.mean())      # A @ beta + beta0 = A_std @ x + mean(b)

Per column j of an (m, n) matrix, every line one rounded float64 operation, rows added in index order (as certificates.column_norms2 adds them):
    mean_j  = (sum_i a_ij) / m                              (center; else 0)
    d_ij    = a_ij - mean_j
    scale_j = sqrt((sum_i d_ij^2) / m), 1 where that is 0   (scale; else 1)
    a_ij   <- d_ij / scale_j
The centred squares are summed as such (sum a^2 - m mean^2 cancels).  A sparse matrix is scaled only: centring would fill it."""

import numpy as np

from . import certificates
from .linalg import canonical_csr, is_sparse_matrix

__all__ = ["standardize", "Standardization", "SPARSE_CENTER_REFUSAL"]

SPARSE_CENTER_REFUSAL = "centring would fill the sparse matrix: a sparse matrix is served with scale alone (center=False)"


class Standardization:
    """What standardize() did to the columns: `means` and `scales` (n doubles each) of an m-row matrix."""

    def __init__(self, means, scales, m):
        self.means = np.asarray(means, dtype=np.float64)
        self.scales = np.asarray(scales, dtype=np.float64)
        self.m = int(m)

    def __iter__(self):
        return iter((self.means, self.scales, self.m))

    def __repr__(self):
        return f"Standardization(n={self.means.size}, m={self.m})"

    def coefficients(self, x):
        """The coefficients in the caller's units: x / scales, row-wise for an (n, L) x."""
        x = np.asarray(x, dtype=np.float64)
        return x / (self.scales[:, None] if x.ndim == 2 else self.scales)

    def intercept(self, x, b_mean):
        """b_mean - means @ coefficients(x): a float for a vector x, L floats for an (n, L) x (b_mean: the mean of b, per column of b)."""
        value = np.asarray(b_mean, dtype=np.float64) - self.means @ self.coefficients(x)
        return float(value) if value.ndim == 0 else value


def _scales_from(ss, m, scale):
    if not scale:
        return np.ones(ss.shape)
    s = np.sqrt(ss / float(m))
    s[s == 0.0] = 1.0
    return s


def standardize(A, center=True, scale=True):
    """(A_std, Standardization(means, scales, m)) for an ndarray or a scipy.sparse matrix, as the module text states it.  A is not written.
    A sparse matrix with center=True: TypeError (centring would fill it); center=False and scale=False: ValueError (nothing to do)."""
    if not center and not scale:
        raise ValueError("standardize: neither center nor scale is asked: nothing to do")
    if is_sparse_matrix(A):
        if center:
            raise TypeError("standardize: " + SPARSE_CENTER_REFUSAL)
        from scipy.sparse import csr_matrix
        data, indices, indptr, shape = canonical_csr(A)
        S = csr_matrix((data, indices, indptr), shape=shape)
        scales = _scales_from(certificates.column_norms2(S), shape[0], True)
        return csr_matrix((data / scales[indices], indices, indptr), shape=shape), Standardization(np.zeros(shape[1]), scales, shape[0])
    A = np.asarray(A, dtype=np.float64)
    if A.ndim != 2:
        raise TypeError("standardize: A must be a 2-D ndarray or a scipy.sparse matrix")
    m, n = A.shape
    means = np.zeros(n)
    if center:
        acc = np.zeros(n)
        for i in range(m):
            acc = acc + A[i]
        means = acc / float(m)
    ss = np.zeros(n)
    if scale:
        for i in range(m):
            d = A[i] - means
            ss = ss + d * d
    scales = _scales_from(ss, m, scale)
    return (A - means) / scales, Standardization(means, scales, m)
