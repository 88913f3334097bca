"""Shared by tests/test_completion_cpu.py and tests/test_gpu_completion.py: the case tables of the observation weights on the identity operator
(fh_set_loss_weights) and of the nuclear-norm ball (FH_PROX_NUCBALL, csrc/fh_nuclear.h: k_nuc_ball), a NumPy restatement of the device's level
rule -- the ordering with its tie-break, the serial running sums, alpha, phi: a MODEL of the kernel, never the thing under test -- and the exact
inputs.
"""

import collections
import glob
import importlib.util
import json
import os

import numpy as np

from tests import nuclear_cases as NC

EPS = NC.EPS
TOL_FACTOR = NC.TOL_FACTOR          # ||xprox_dev - project_nuclear_ball(xhat, r)||_F <= 32 * p * eps * ||xhat||_F: projection onto a convex set is non-expansive, as thresholding is


# ---- the level rule restated --------------------------------------------------------------------------------------------------------------------
def model_order(sigma):
    """The sigma in the device's order: rank_i = #{j : sigma_j > sigma_i, or sigma_j == sigma_i and j < i}, out[rank_i] = sigma_i."""
    sigma = np.asarray(sigma, dtype=np.float64)
    out = np.zeros(len(sigma))
    for i, si in enumerate(sigma):
        rank = sum(1 for j, sj in enumerate(sigma) if sj > si or (sj == si and j < i))
        out[rank] = si
    return out


def model_level(sigma, radius):
    """(theta, phi, kept) by the device's rule: running sums formed serially in the order above, alpha = max_k (c_k - radius) / k,
    theta = max(alpha, 0), kept_i = max(sigma_i - theta, 0), phi_i = kept_i / (sigma_i + (sigma_i == 0))."""
    sigma = np.asarray(sigma, dtype=np.float64)
    ordered = model_order(sigma)
    c, sums = np.float64(0.0), np.zeros(len(sigma))
    for k, v in enumerate(ordered):                     # serially, in index order: np.cumsum's order
        c = c + v
        sums[k] = c
    alpha = max((sums[k] - radius) / np.float64(k + 1) for k in range(len(sigma)))
    theta = max(alpha, 0.0)
    kept = np.maximum(sigma - theta, 0.0)
    return float(theta), kept / (sigma + (sigma == 0)), kept


# ---- the exact input of the ball: the rows of tests/nuclear_cases.py, sigma = {16, 4, 2, 8, 0} --------------------------------------------------
BALL_RADIUS = 12.0
BALL_THETA = 6.0
BALL_KEPT = (10.0, 0.0, 0.0, 2.0, 0.0)
BALL_FACTORS = (0.625, 0.0, 0.0, 0.25, 0.0)         # kept / sigma
BALL_GSUM, BALL_GMAX, BALL_RANK = 12.0, 10.0, 2


# ... and the same rows scaled {4, 4, 1/2, 2, 0}: sigma = {16, 16, 2, 8, 0}, two EQUAL non-zero values, which only the index orders.  Radius 12:
# ordered 16, 16, 8, 2, 0, running sums 16, 32, 40, 42, 42, (c_k - 12) / k = 4, 10, 9 1/3, 7.5, 6: theta = 10, kept {6, 6, 0, 0, 0}.  (Without the
# tie-break both 16 take rank 0, the second slot of the ordering stays 0 and theta comes out as 4.)
TIE_SCALES = (4.0, 4.0, 0.5, 2.0, 0.0)
TIE_SIGMA = (16.0, 16.0, 2.0, 8.0, 0.0)
TIE_THETA = 10.0
TIE_KEPT = (6.0, 6.0, 0.0, 0.0, 0.0)
TIE_FACTORS = (0.375, 0.375, 0.0, 0.0, 0.0)
TIE_GSUM, TIE_GMAX, TIE_RANK = 12.0, 6.0, 2


def ball_tie_input():
    """(X, its projection onto the nuclear-norm ball of radius 12) with two equal non-zero singular values: all dyadic, no rotation."""
    H = NC.hadamard16()
    X = np.stack([s * H[r] for r, s in zip(NC.EXACT_ROWS, TIE_SCALES)])
    return X, np.stack([f * row for f, row in zip(TIE_FACTORS, X)])


def ball_exact_input():
    """(X, its projection onto the nuclear-norm ball of radius 12): all dyadic, one sweep without a rotation."""
    X, _ = NC.exact_input()
    want = np.stack([f * row for f, row in zip(BALL_FACTORS, X)])
    return X, want


# ---- rotating cases of the ball: the shapes of tests/nuclear_cases.py ----------------------------------------------------------------------------
BallCase = collections.namedtuple("BallCase", "name M N Bk kind")
BALL_CASES = [
    BallCase("three_blocks_bye", 5, 7, 2, "random"),
    BallCase("self_pair", 3, 9, 8, "random"),
    BallCase("one_pair", 16, 40, 8, "random"),
    BallCase("padding_odd_ragged", 33, 130, 4, "random"),
    BallCase("transposed", 40, 16, 8, "random"),
    BallCase("p1_row", 1, 13, 8, "random"),
    BallCase("p1_col", 13, 1, 8, "random"),
    BallCase("several_chunks", 24, 600, 8, "random"),
    BallCase("ties_in_the_ordering", 64, 300, 8, "duplicated"),
    BallCase("radius_above_the_norm", 9, 11, 4, "outside"),
    BallCase("radius_zero", 7, 12, 4, "r0"),
    BallCase("zero_matrix", 6, 10, 2, "zero"),
]
FULL_WIDTH = BallCase("full_ordering_width", 1024, 1024, 0, "rank8")


def ball_input(case):
    """(X, radius) of a rotating case; deterministic."""
    rng = np.random.RandomState(2000 + 7 * case.M + case.N)
    if case.kind == "rank8":
        X = rng.randn(case.M, 8) @ rng.randn(8, case.N) + 1e-3 * rng.randn(case.M, case.N)
        return X, 0.5 * float(np.linalg.svd(X, compute_uv=False).sum())
    X = rng.randn(case.M, case.N)
    if case.kind == "duplicated":
        X[case.M // 2:] = X[:case.M - case.M // 2]
    if case.kind == "zero":
        return np.zeros((case.M, case.N)), 3.0
    total = float(np.linalg.svd(X, compute_uv=False).sum())
    if case.kind == "outside":
        return X, 1.25 * total
    if case.kind == "r0":
        return X, 0.0
    return X, 0.4 * total


def tolerance(X, factor=TOL_FACTOR):
    return NC.tolerance(X, factor)


# ---- the weighted step: shapes, losses, prox kinds -------------------------------------------------------------------------------------------------
STEP_SHAPES = [(1, 1), (3, 5), (33, 130)]              # one entry; one ragged workgroup; several workgroups, ragged
SECOND_TRIP = (725, 725)                               # 525 625 entries: just past the 2048 x 256 grid cap, the grid-stride loop makes a second trip
STEP_KINDS = ["identity", "shrink", "nonneg", "box", "nuclear", "nucball"]


def step_problem(M, N, seed=5):
    """Dyadic data of one step: X0, B in eighths, weights in {0, 1/4, 1/2, 1, 2} -- every elementwise expression of a least-squares step with
    tau and coef powers of two is exact in float64."""
    rng = np.random.RandomState(seed + 31 * M + N)
    X0 = rng.randint(-8, 9, (M, N)) / 4.0
    B = rng.randint(-8, 9, (M, N)) / 8.0
    W = rng.choice([0.0, 0.25, 0.5, 1.0, 2.0], size=(M, N))
    return X0, B, W


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------------------
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "completion")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
EXPECTED = ["wlog_ball_12x20_adaptive", "wlog_nuc_12x20_adaptive", "wlsq_ball_12x20_accelerated", "wlsq_ball_12x20_adaptive",
            "wlsq_nuc_12x20_accelerated", "wlsq_nuc_12x20_adaptive", "wlsq_nuc_12x20_backtracks", "wlsq_nuc_12x20_plain", "wlsq_nuc_20x12_adaptive",
            "wlsq_shrink_9x7_adaptive"]
HISTORIES = NC.HISTORIES
MIN_PREFIX = NC.MIN_PREFIX


def capture_script():
    """scripts/make_completion_golden.py as a module: the ONE place that states how the fixtures were captured."""
    path = os.path.join(HERE, os.pardir, "scripts", "make_completion_golden.py")
    spec = importlib.util.spec_from_file_location("make_completion_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    return meta, z, {k[3:]: z[k] for k in z.files if k.startswith("in_")}


def compared_prefix(meta, z):
    """(iterations compared, whole run?)"""
    total = int(z["iteration_count"])
    k = min(int(meta["twin_divergence"]), total)
    return k, k == total
