"""What tests/test_dct2_cpu.py and tests/test_gpu_dct2.py share about the subsampled 2-D DCT operator (csrc/fh_dct2.h): the shapes the GPU tier
walks, the fixtures of scripts/make_dct2_golden.py, the exact separable transform, the error bound, and a NumPy MODEL of the device algorithm --
per axis the Makhoul gather, the Stockham radix passes with the kernel's own index arithmetic (tests/dct_cases.py: stockham, tables, src_index),
the post-twiddle to a real row, the transposes between the axes and the adjoint chain -- over the radices that the library's rule
(fh_dct2_shape_for) reports.  The CPU tier holds the model to the exact transform, which pins that index arithmetic without a device."""
import glob
import json
import os

import numpy as np
import scipy.fftpack

from tests import dct_cases as T1

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dct2")
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
FIELDS = T1.FIELDS

# the smallest shapes at which each part can go wrong: an axis of length 1 (the identity), every radix, a ragged last row group (18 x 40: 40 rows of
# length 18 in groups of 7), ragged 32 x 32 tiles on both sides (36 x 50), the LDS classes 128 -> 512 (96 x 135) and 512 -> 2048 (128 x 540), the
# longest row beside the shortest
SMALL = [(1, 1), (1, 8), (8, 1), (2, 3), (3, 5), (4, 4), (5, 16), (15, 9), (16, 25), (18, 40), (36, 50), (30, 64), (45, 96), (64, 64), (96, 135)]
LARGE = [(128, 540), (2048, 3), (3, 2048)]
SIZES = SMALL + LARGE
FULL_SIZE = (2048, 2048)
REFUSED = (((7, 8), 0, "axis 0 .*prime factor above 5"), ((8, 7), 0, "axis 1 .*prime factor above 5"), ((4096, 4), 0, "axis 0 .*no two-level form per axis"),
           ((4, 4096), 0, "axis 1 .*no two-level form per axis"), ((0, 4), 0, "axis 0 .*is empty"), ((60, 60), 16, "row cap \\(16\\).*no two-level form per axis"))


def ident(shape):
    return f"{shape[0]}x{shape[1]}"


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return json.loads(str(z["meta"])), z, {k[3:]: z[k] for k in z.files if k.startswith("in_")}


prefix_of = T1.prefix_of


def bound(H, W, frob):
    """|dev - exact|_inf <= (beta(H) + beta(W)) * |X|_F, beta(L) = (8 ceil(log2 L) + 8) 2^-53 (tests/dct_cases.py:bound, the 1-D operator's): the
    first pass errs by at most beta |row|_2 per entry; the orthonormal second pass carries a column of those errors at no more than its 2-norm,
    <= beta |X|_F, and adds beta |column|_2 <= beta |X|_F of its own.  The device transforms one real row per complex FFT (no two rows packed into
    one), so there is no factor sqrt(2) on the first term."""
    return (T1.bound(H, 1.0) + T1.bound(W, 1.0)) * float(frob)


def exact_dct2(X, adjoint=False):
    """C_H X C_W^T (adjoint: C_H^T X C_W) in longdouble by the direct sums."""
    X = np.asarray(X, dtype=np.longdouble)
    CH, CW = T1._exact_matrix(X.shape[0]), T1._exact_matrix(X.shape[1])
    return (CH.T @ X @ CW) if adjoint else (CH @ X @ CW.T)


# ---- the model of the device algorithm -------------------------------------------------------------------------------------------------------
def rows_fwd(R, radices):
    """k_dct2_fwd_rows: every row of R through the gather, the row FFT and the post-twiddle to a real row."""
    L = R.shape[1]
    tw, pw = T1.tables(L)
    sc0, sck = T1.scales(L)
    V = T1.stockham(np.asarray(R, dtype=np.float64)[:, T1.src_index(L)].astype(np.complex128), radices, tw, L, False)
    s = np.full(L, sck)
    s[0] = sc0
    return (V * pw).real * s


def rows_adj(R, radices):
    """k_dct2_adj_rows: every real row of R through the pre-twiddle, the inverse row FFT and the scatter."""
    L = R.shape[1]
    tw, pw = T1.tables(L)
    sc0, sck = T1.scales(L)
    s = np.full(L, 0.5 * sck)
    s[0] = sc0
    u = np.asarray(R, dtype=np.float64) * s
    um = np.zeros(u.shape)
    um[:, 1:] = u[:, 1:][:, ::-1]                                     # u[L - k], u[L] = 0
    v = T1.stockham(pw.conj() * (u - 1j * um), radices, tw, L, True).real
    out = np.empty(u.shape)
    out[:, T1.src_index(L)] = v
    return out


def check_geometry(sh):
    """The launches the model stands for exist: every row has one workgroup, whose rows fit its LDS class."""
    for L, rows, lds, rpw, grid in ((sh.H, sh.W, sh.lds_h, sh.rows_h, sh.grid_h), (sh.W, sh.H, sh.lds_w, sh.rows_w, sh.grid_w)):
        assert lds in (128, 512, 2048) and 1 <= rpw and rpw * L <= lds and grid == -(-rows // rpw), sh
    assert sh.tiles == -(-sh.H // 32) * -(-sh.W // 32) and sh.launches == 4


def model_fwd(X, diag, sh):
    """z = d * (C_H X C_W^T) as the device computes it: rows along W, transpose, rows along H, transpose back."""
    check_geometry(sh)
    Y = rows_fwd(rows_fwd(X, sh.radices_w).T.copy(), sh.radices_h).T
    return Y if diag is None else np.where(diag == 0.0, 0.0, diag * Y)


def model_adj(Wm, diag, sh):
    """x = C_H^T (d * w) C_W as the device computes it: transpose, rows along H, transpose, rows along W."""
    check_geometry(sh)
    U = np.asarray(Wm, dtype=np.float64) if diag is None else Wm * diag
    return rows_adj(rows_adj(U.T.copy(), sh.radices_h).T.copy(), sh.radices_w)


def operands(shape, seed):
    """(x, y, mask): two Gaussian images and a 0/1 mask with about half the entries kept."""
    rng = np.random.RandomState(seed)
    x, y = rng.randn(*shape), rng.randn(*shape)
    mask = (rng.rand(*shape) < 0.5).astype(np.float64)
    return x, y, mask


def host_fwd(x, mask=None):
    y = scipy.fftpack.dctn(x, norm="ortho")
    return y if mask is None else mask * y


def host_adj(w, mask=None):
    return scipy.fftpack.idctn(w if mask is None else mask * w, norm="ortho")
