"""What tests/test_standardize_cpu.py and tests/test_gpu_standardize.py share: shapes, data, the path problem and the refusals of
path(standardize=..., intercept=...) (fasta_python_amd/preprocess.py, fasta_python_amd/regpath.py; csrc/fh_standardize.h).

Geometry (hip.screen_shape_for, asserted by the CPU tier).  A lane owns one 16-byte piece (2 float64 or 4 float32 columns) of a tile of 256 pieces
and a slab of rows that is a multiple of 16.  (6, 10): one workgroup.  (33, 530) float64: mp = 48, three slabs of 16 with a ragged last one (one
live row, fifteen padding rows) and two column tiles, n no multiple of 16.  (40, 1030) float32: two tiles of 1024, n no multiple of 32.  (32, 530):
m a power of two, two full slabs.

Exactness (balanced_dyadic).  Column j is (c_j + e_ij) / 8 with small integers c_j and e_ij, where e_.j sums to zero: the entries of the upper half of
the rows are mirrored with the opposite sign, in another order, in the lower half (an odd m leaves one zero).  So the column sum is m c_j / 8, exact in
any order, and the mean is c_j / 8 EXACTLY for every m; d = e / 8 is exact, d^2 is a multiple of 1 / 64 and a column's sum of squares is exact in any
order, with fma or without.  From there on the statement is a chain of single correctly rounded operations (a division by m, a square root, a
division by the scale), spelled alike on both sides: device and host agree with `==`.  Every matrix holds a constant non-zero column (scale 0 -> 1), an
all-zero column and one column 2^20 times larger than the rest (a power of two keeps it exact)."""
import numpy as np

SHAPES = [("f64", 6, 10), ("f64", 33, 530), ("f32", 40, 1030), ("f64", 32, 530), ("f32", 33, 530)]
IDS = ["%s-%dx%d" % s for s in SHAPES]
CONSTANT, ZERO, LARGE = 1, 2, 3                 # the special columns
# storage, m, n -> (slab, nslab, tile_cols, tiles, grid) at 256 compute units
GEOMETRY = {("f64", 6, 10): (16, 1, 512, 1, 1), ("f64", 33, 530): (16, 3, 512, 2, 6), ("f32", 40, 1030): (16, 3, 1024, 2, 6),
            ("f64", 32, 530): (16, 2, 512, 2, 4), ("f32", 33, 530): (16, 3, 1024, 1, 3)}
EPS = 2.0 ** -52


def balanced_dyadic(m, n, seed):
    """(m, n) float64 as the module text states it; exactly representable in float32 too."""
    rng = np.random.RandomState(seed)
    h = m // 2
    E = np.zeros((m, n))
    top = rng.randint(-5, 6, size=(h, n)).astype(np.float64)
    E[:h] = top
    for j in range(n):
        E[m - h:, j] = -top[rng.permutation(h), j]
    c = rng.randint(-3, 4, size=n).astype(np.float64)
    A = (E + c) / 8.0
    A[:, CONSTANT] = 5.0 / 8.0
    A[:, ZERO] = 0.0
    A[:, LARGE] = A[:, LARGE] * 2.0 ** 20
    return A


def two_level(m, n, seed):
    """(m, n) float64, m even: column j is (c_j +- 2^(j mod 3)) / 8 with as many + as - in an order of its own.  The mean is c_j / 8, every
    d is +-2^(j mod 3) / 8, so ss / m = 4^(j mod 3) / 64 and the scale is 2^(j mod 3) / 8, all EXACT: the standardised column holds +-1, and a
    second standardisation finds means of exactly 0 and scales of exactly 1.  The three special columns as in balanced_dyadic."""
    assert m % 2 == 0
    rng = np.random.RandomState(seed)
    sign = np.ones((m, n))
    for j in range(n):
        sign[rng.permutation(m)[:m // 2], j] = -1.0
    A = (rng.randint(-3, 4, size=n) + sign * 2.0 ** (np.arange(n) % 3)) / 8.0
    A[:, CONSTANT] = 5.0 / 8.0
    A[:, ZERO] = 0.0
    A[:, LARGE] = A[:, LARGE] * 2.0 ** 20
    return A


def seeded(m, n, seed):
    """Any data: normal entries about column offsets, the same three special columns (the large one a million times the rest)."""
    rng = np.random.RandomState(seed)
    A = rng.randn(m, n) * np.exp(rng.randn(n)) + 3.0 * rng.randn(n)
    A[:, CONSTANT] = 0.25                       # (a dyadic constant: its sum and its mean are exact, so d = 0 and the scale is 1)
    A[:, ZERO] = 0.0
    A[:, LARGE] = A[:, LARGE] * 1e6
    return A


def stored(A, storage):
    """The values a context of this storage holds for A, as float64."""
    return A.astype(np.float32).astype(np.float64) if storage == "f32" else np.asarray(A, dtype=np.float64)


def long_sparse():
    """tests/sparse_lanes.py: long_matrix(0) (601 x 703, a dense row and a dense column: a long row in both copies) with column 5 emptied but for
    the dense row's entry, which is removed too: an empty column."""
    from tests import sparse_lanes as SL
    S = SL.long_matrix(0).tolil()
    S[:, 5] = 0.0
    S = S.tocsr()
    S.eliminate_zeros()
    S.sort_indices()
    return S


def path_problem(seed=5):
    """(A, b): 64 x 200, column scales spread over six decades, column offsets, five active features and a planted intercept."""
    rng = np.random.RandomState(seed)
    m, n = 64, 200
    scales = 10.0 ** rng.uniform(-3, 3, size=n)
    A = rng.randn(m, n) * scales + rng.randn(n) * scales
    x = np.zeros(n)
    act = rng.permutation(n)[:5]
    x[act] = 2.0 * rng.randn(5) / scales[act]
    return A, A @ x + 7.5 + 0.01 * rng.randn(m)


def sparse_path_problem(seed=6):
    from scipy import sparse as sp
    rng = np.random.RandomState(seed)
    m, n = 48, 90
    S = sp.random(m, n, density=0.2, format="csr", random_state=rng, data_rvs=rng.standard_normal)
    S = sp.csr_matrix(S.multiply(10.0 ** rng.uniform(-3, 3, size=n)))
    scales = np.sqrt(np.asarray(S.multiply(S).sum(axis=0)).ravel() / m)
    x = np.zeros(n)
    act = np.flatnonzero(scales > 0)[:4]
    x[act] = 2.0 / scales[act]
    return S, S @ x + 0.01 * rng.randn(m)


PATH_OPTS = dict(n_mus=5, ratio=1e-2, gap_tolerance=1e-6, max_iters=3000)


def path_refusals(fa):
    """(keywords of path(), the words the TypeError must hold) for every refusal of regpath.py's standardised path; needs no device (maps are lazy)."""
    from scipy import sparse as sp
    rng = np.random.RandomState(0)
    A = rng.randn(8, 12)
    b = rng.randn(8)
    labels = np.where(b > 0, 1.0, -1.0)
    S = sp.csr_matrix(A * (rng.rand(8, 12) < 0.4))
    ls = fa.LeastSquares(b)
    return [
        (dict(A=A, loss=fa.LogisticLoss(labels), intercept=True), ["intercept=True is served for losses.LeastSquares without weights on a dense matrix", "logistic", "no closed form"]),
        (dict(A=A, loss=fa.LogisticLoss(labels), intercept=True, standardize=True), ["intercept=True is served for losses.LeastSquares", "no closed form"]),
        (dict(A=S, loss=ls, intercept=True), ["intercept=True is served for losses.LeastSquares without weights on a dense matrix", "centring would fill the sparse matrix", "standardize=True alone is served"]),
        (dict(A=fa.DenseMatrixMap(A), loss=ls, standardize=True), ["DenseMatrixMap", "the caller's to rewrite", "map.ctx.standardize()", "preprocess.Standardization"]),
        (dict(A=fa.DenseMatrixMap(A), loss=ls, intercept=True), ["DenseMatrixMap", "map.ctx.standardize()", "preprocess.Standardization"]),
        (dict(A=fa.SparseMatrixMap(S), loss=ls, standardize=True), ["SparseMatrixMap", "map.ctx.standardize()", "preprocess.Standardization"]),
        (dict(A=fa.ShardedDenseMatrixMap(A, devices=(0, 0)), loss=ls, standardize=True), ["sharded map", "an ndarray (dense) or a scipy.sparse matrix (scaling only)"]),
    ]
