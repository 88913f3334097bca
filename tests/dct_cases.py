"""What tests/test_dct_cpu.py and tests/test_gpu_dct.py share about the subsampled DCT operator (csrc/fh_dct.h): the sizes the GPU tier walks,
the fixtures of scripts/make_dct_golden.py, the exact transform, the error bound, and a NumPy MODEL of the device algorithm -- the Makhoul
permutation, the N1 x N2 split with its six-step twiddle and transposes, the Stockham radix passes with the kernel's own index arithmetic,
the post-twiddle and the adjoint chain -- over the radices and the split that the library's rule (fh_dct_shape_for) reports.  The CPU tier
holds the model to scipy.fftpack, which pins that index arithmetic without a device."""
import functools
import glob
import json
import math
import os

import numpy as np
import scipy.fftpack

from fasta_python_amd import hip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dct")
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
FIELDS = ("residuals", "norm_residuals", "stepsizes", "objectives")

# (N, FH_TUNE_DCT_ROW_CAP; 0 = the default 2048)
ONE_ROW = [(N, 0) for N in (1, 2, 3, 4, 5, 6, 8, 9, 15, 16, 25, 30, 45, 64, 96, 125, 1000, 1024, 2048)]
# two levels: at the default cap (6000 = 3 * 2000: a ragged transpose tile and an odd factor), at a cap of 16, and 1000 = 25 x 40 at a cap of 40
# (N1 != N2, every radix).  250 = 2 * 5^3 has NO split with both factors at most 16 (its divisors up to 16 are 1, 2, 5, 10), so at that cap it is
# a refusal (REFUSED_AT_CAP); the same length runs as 10 x 25 at a cap of 25.
TWO_LEVEL = [(4096, 0), (6000, 0), (60, 16), (96, 16), (150, 16), (250, 25), (1000, 40)]
FULL_SIZE = [(1 << 22, 0), (3 << 20, 0)]
SIZES = ONE_ROW + TWO_LEVEL
REFUSED = (7, 1001, 3 ** 15, 0)
REFUSED_AT_CAP = ((250, 16),)


_PI = np.longdouble("3.14159265358979323846264338327950288")


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return json.loads(str(z["meta"])), z, {k[3:]: z[k] for k in z.files if k.startswith("in_")}


def prefix_of(meta, z):
    """Iterations compared: all of them, or -- an adaptive run -- up to where the oracle parts from its twin."""
    return min(int(meta.get("twin_divergence", int(z["iteration_count"]))), int(z["iteration_count"]))


def bound(N, norm2):
    """|dev - exact|_inf <= (8 * ceil(log2 N) + 8) * 2^-53 * |x|_2: at most 8 roundings of relative size 2^-53 per radix pass of a generic
    butterfly over at most ceil(log2 N) passes, and 8 more for the permutation twiddle, the six-step twiddle and the scale."""
    passes = math.ceil(math.log2(N)) if N > 1 else 0
    return (8 * passes + 8) * 2.0 ** -53 * float(norm2)


@functools.lru_cache(maxsize=None)
def _exact_matrix(N):
    """C[k, n] = s_k cos(pi k (2n + 1) / (2N)) in longdouble; the argument is reduced in integers (k (2n + 1) mod 4N) first."""
    k = np.arange(N, dtype=np.int64)[:, None]
    n = np.arange(N, dtype=np.int64)[None, :]
    arg = (k * (2 * n + 1)) % (4 * N)
    M = np.cos(arg.astype(np.longdouble) * (_PI / np.longdouble(2 * N)))
    s = np.full(N, np.sqrt(np.longdouble(2) / np.longdouble(N)))
    s[0] = np.sqrt(np.longdouble(1) / np.longdouble(N))
    return M * s[:, None]


def exact_dct(x, adjoint=False):
    """The orthonormal DCT-II (adjoint: its transpose, the DCT-III) of a vector of at most 2048 entries by the direct O(N^2) sum in longdouble."""
    x = np.asarray(x, dtype=np.longdouble)
    C = _exact_matrix(len(x))
    return (C.T @ x) if adjoint else (C @ x)


# ---- the model of the device algorithm -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def tables(N):
    """tw[j] = e^{-2 pi i j / N} and pw[k] = e^{-i pi k / 2N}, computed in longdouble and rounded once (fasta_hip.hip: dct_alloc_tables)."""
    j = np.arange(N, dtype=np.longdouble)
    a = 2 * _PI * j / np.longdouble(N)
    tw = np.cos(a).astype(np.float64) - 1j * np.sin(a).astype(np.float64)
    a = _PI * j / (2 * np.longdouble(N))
    pw = np.cos(a).astype(np.float64) - 1j * np.sin(a).astype(np.float64)
    return tw, pw


def scales(N):
    return float(np.sqrt(np.longdouble(1) / np.longdouble(N))), float(np.sqrt(np.longdouble(2) / np.longdouble(N)))


def src_index(N):
    """Position j of v holds x[src[j]]: v[j] = x[2j] for j < ceil(N/2), v[N-1-j] = x[2j+1] (csrc/fh_dct.h: dct_src)."""
    j = np.arange(N)
    return np.where(j < (N + 1) // 2, 2 * j, 2 * (N - 1 - j) + 1)


def stockham(rows, radices, tw, N, conj):
    """The row transforms of csrc/fh_dct.h:dct_pass over the rows of a (count, L) complex array: per pass of radix r, current length n and stride s
    (n * s = L), butterfly u = p * s + q reads x[u + j * L / r] and writes y[q + s (r p + k)] = w_n^{p k} sum_j x_j w_r^{j k}."""
    a = np.array(rows, dtype=np.complex128)
    L = a.shape[1]
    n, s = L, 1
    for r in radices:
        per = L // r
        u = np.arange(per)
        p, q = u // s, u % s
        root = np.exp(-2j * np.pi * np.arange(r) / r)
        if conj:
            root = root.conj()
        x = [a[:, u + j * per] for j in range(r)]
        b = np.empty_like(a)
        for k in range(r):
            acc = x[0].copy()
            for j in range(1, r):
                acc = acc + x[j] * root[(j * k) % r]
            w = tw[p * k * (N // n)]
            b[:, q + s * (r * p + k)] = acc * (w.conj() if conj else w)
        a = b
        n //= r
        s *= r
    assert n == 1 and s == L
    return a


def fft_model(v, sh, conj):
    """sum_n v[n] e^{-+2 pi i n k / N} in the device's order: one row (sh.levels == 1) or N2 rows of length N1, the six-step twiddle, a
    transpose, N1 rows of length N2, and the k = b1 + N1 b2 ordering."""
    N = len(v)
    tw, _ = tables(N)
    if sh.levels == 1:
        return stockham(v[None, :], sh.radices1, tw, N, conj)[0]
    N1, N2 = sh.N1, sh.N2
    rows = v.reshape(N1, N2).T                                        # (a2, a1): v[N2 a1 + a2]
    F = stockham(rows, sh.radices1, tw, N, conj)                      # (a2, b1)
    six = tw[np.arange(N2)[:, None] * np.arange(N1)[None, :]]
    F = F * (six.conj() if conj else six)
    G = stockham(F.T, sh.radices2, tw, N, conj)                       # (b1, b2)
    return G.T.reshape(-1)                                            # k = b1 + N1 b2


def model_fwd(x, diag, sh):
    """z = d * C x as the device computes it."""
    x = np.asarray(x, dtype=np.float64)
    N = len(x)
    _, pw = tables(N)
    sc0, sck = scales(N)
    V = fft_model(x[src_index(N)].astype(np.complex128), sh, False)
    s = np.full(N, sck)
    s[0] = sc0
    y = (V * pw).real * s
    return y if diag is None else np.where(diag == 0.0, 0.0, diag * y)


def model_adj(w, diag, sh):
    """x = C^T (d * w) as the device computes it."""
    w = np.asarray(w, dtype=np.float64)
    N = len(w)
    _, pw = tables(N)
    sc0, sck = scales(N)
    s = np.full(N, 0.5 * sck)
    s[0] = sc0
    u = (w if diag is None else w * diag) * s
    um = np.zeros(N)
    um[1:] = u[1:][::-1]                                              # u[N - k], u[N] = 0
    V = pw.conj() * (u - 1j * um)
    v = fft_model(V, sh, True).real
    x = np.empty(N)
    x[src_index(N)] = v
    return x


def operands(N, seed):
    """(x, y, mask): two Gaussian vectors and a 0/1 mask with about half the entries kept."""
    rng = np.random.RandomState(seed)
    x, y = rng.randn(N), rng.randn(N)
    mask = (rng.rand(N) < 0.5).astype(np.float64)
    return x, y, mask


def host_fwd(x, mask=None):
    y = scipy.fftpack.dct(x, norm="ortho")
    return y if mask is None else mask * y


def host_adj(w, mask=None):
    return scipy.fftpack.idct(w if mask is None else mask * w, norm="ortho")
