"""Shared by tests/test_nuclear_cpu.py and tests/test_gpu_nuclear.py: the case table of the singular-value thresholding
(csrc/fh_nuclear.h), a NumPy restatement of its block one-sided Jacobi rule -- a MODEL of the device algorithm, used to hold the rule
itself to the tolerance without a GPU, never the thing under test -- and the exact inputs.
"""

import collections
import glob
import importlib.util
import json
import os

import numpy as np

EPS = float(np.finfo(np.float64).eps)
MAX_SWEEPS = 30                     # csrc/fh_nuclear.h: NUC_MAX_SWEEPS (outer sweeps and inner sweeps of a step alike)
TOL_FACTOR = 32.0                   # ||xprox_dev - project_Lnuc_ball(xhat, t)||_F <= 32 * p * eps * ||xhat||_F
MODEL_FACTOR = 8.0                  # ... and a quarter of it for the restatement
AUTO_BLOCK_ROWS = 1                 # csrc/fh_nuclear.h: NUC_AUTO_BLOCK_ROWS (FH_TUNE_NUC_BLOCK_ROWS = 0)
COLUMN_CHUNK = 256                  # columns a workgroup stages per trip of the Gram pass


def shape_of(M, N, block_rows=0):
    """What fh_nuclear_shape_for must report for an (M, N) unknown: the geometry rule restated."""
    Bk = block_rows or AUTO_BLOCK_ROWS
    transposed = M > N
    p, q = min(M, N), max(M, N)
    P = -(-p // Bk) * Bk
    nb = P // Bk
    nbe = nb + (nb & 1)
    qpad, Ppad = q + (q & 1), P + (P & 1)
    ld = qpad + Ppad
    return dict(transposed=int(transposed), p=p, q=q, Bk=Bk, P=P, nb=nb,
                steps_per_sweep=1 if nb == 1 else nbe - 1, wgs_per_step=1 if nb == 1 else nbe // 2,
                column_chunk=COLUMN_CHUNK, chunks_per_row=-(-qpad // COLUMN_CHUNK), ld=ld, bytes=P * ld * 8,
                lds_bytes=(2 * Bk * (COLUMN_CHUNK + 2) + 2 * (2 * Bk) * (2 * Bk) + 256) * 8)


def step_pairs(nb, r):
    """Block pairs of step r of a sweep: the round-robin tournament over nb blocks (circle method, the last of an even count stays put);
    an odd nb gives one block a bye, nb = 1 a single self-pair (b = -1)."""
    if nb == 1:
        return [(0, -1)]
    nbe = nb + (nb & 1)
    out = []
    for k in range(nbe // 2):
        a, b = (nbe - 1, r) if k == 0 else ((r + k) % (nbe - 1), (r + nbe - 1 - k) % (nbe - 1))
        if max(a, b) >= nb:
            continue                                    # the bye
        out.append((min(a, b), max(a, b)))
    return out


def _diagonalise(G, dead_thr, tol):
    """Cyclic Jacobi on the symmetric G with the device's rules; returns (V, rotations)."""
    R = G.shape[0]
    G = G.copy()
    V = np.eye(R)
    for k in range(R):
        if not G[k, k] > dead_thr:
            G[k, :] = 0.0
            G[:, k] = 0.0
    total = 0
    for _ in range(MAX_SWEEPS):
        rot = 0
        for i in range(R - 1):
            for j in range(i + 1, R):
                gij = G[i, j]
                if not abs(gij) > tol * np.sqrt(G[i, i] * G[j, j]):
                    continue
                zeta = (G[j, j] - G[i, i]) / (2.0 * gij)
                t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = c * t
                for A in (G, V):
                    ci, cj = A[:, i].copy(), A[:, j].copy()
                    A[:, i], A[:, j] = c * ci - s * cj, s * ci + c * cj
                ri, rj = G[i, :].copy(), G[j, :].copy()
                G[i, :], G[j, :] = c * ri - s * rj, s * ri + c * rj
                G[i, j] = G[j, i] = 0.0
                rot += 1
        total += rot
        if rot == 0:
            break
    return V, total


Info = collections.namedtuple("Info", "sweeps steps rotations rank gsum converged")


def model_svt(X, thr, block_rows=0):
    """prox of thr * ||.||_* at X by the device's rule: (xprox, Info)."""
    X = np.asarray(X, dtype=np.float64)
    M, N = X.shape
    sh = shape_of(M, N, block_rows)
    Bk, p, q, P, nb = sh["Bk"], sh["p"], sh["q"], sh["P"], sh["nb"]
    W = np.zeros((P, q))
    W[:p] = X.T if sh["transposed"] else X
    Jt = np.eye(P)
    fro2 = float(np.sum(X * X))
    dead_thr = (EPS * np.sqrt(fro2)) ** 2
    tol = EPS * np.sqrt(q)
    sweeps = steps = rotations = 0
    converged = False
    while sweeps < MAX_SWEEPS:
        sweeps += 1
        rot_sweep = 0
        for r in range(sh["steps_per_sweep"]):
            steps += 1
            for a, b in step_pairs(nb, r):
                rows = list(range(a * Bk, (a + 1) * Bk)) + ([] if b < 0 else list(range(b * Bk, (b + 1) * Bk)))
                Wr = W[rows]
                V, rot = _diagonalise(Wr @ Wr.T, dead_thr, tol)
                if rot:
                    W[rows] = V.T @ Wr
                    Jt[rows] = V.T @ Jt[rows]
                    rot_sweep += rot
        rotations += rot_sweep
        if rot_sweep == 0:
            converged = True
            break
    sigma = np.sqrt(np.sum(W * W, axis=1))
    kept = np.maximum(sigma - thr, 0.0)
    phi = kept / (sigma + (sigma == 0))
    out = (Jt.T[:p] * phi) @ W
    info = Info(sweeps, steps, rotations, int(np.sum(sigma[:p] > thr)), float(np.sum(kept[:p])), converged)
    return (out.T if sh["transposed"] else out), info


# ---- the exact input ----------------------------------------------------------------------------------------------------------------------
def hadamard16():
    H = np.array([[1.0]])
    for _ in range(4):
        H = np.block([[H, H], [H, -H]])
    return H


EXACT_ROWS = (1, 3, 6, 10, 15)
EXACT_SCALES = (4.0, 1.0, 0.5, 2.0, 0.0)
EXACT_SIGMA = (16.0, 4.0, 2.0, 8.0, 0.0)
EXACT_THR = 4.0
EXACT_FACTORS = (0.75, 0.0, 0.0, 0.5, 0.0)
EXACT_GSUM, EXACT_RANK = 16.0, 2


def exact_input():
    """(X, expected prox at threshold 4): mutually orthogonal rows of the 16 x 16 Sylvester-Hadamard matrix, every product a power of two."""
    H = hadamard16()
    X = np.stack([s * H[r] for r, s in zip(EXACT_ROWS, EXACT_SCALES)])
    want = np.stack([f * row for f, row in zip(EXACT_FACTORS, X)])
    return X, want


# ---- rotating cases ------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name M N Bk kind")
CASES = [
    Case("three_blocks_bye", 5, 7, 2, "random"),
    Case("self_pair", 3, 9, 8, "random"),
    Case("one_pair", 16, 40, 8, "random"),
    Case("padding_odd_ragged", 33, 130, 4, "random"),
    Case("transposed", 40, 16, 8, "random"),
    Case("p1_row", 1, 13, 8, "random"),
    Case("p1_col", 13, 1, 8, "random"),
    Case("several_chunks", 24, 600, 8, "random"),
    Case("rank_deficient", 64, 300, 8, "duplicated"),
    Case("zero", 6, 10, 2, "zero"),
    Case("all_below", 7, 12, 4, "below"),
    Case("mu_zero", 9, 11, 4, "mu0"),
]


def case_input(case):
    """(X, threshold tau * mu) of a rotating case; deterministic."""
    rng = np.random.RandomState(1000 + 7 * case.M + case.N)
    X = rng.randn(case.M, case.N)
    if case.kind == "duplicated":
        X[case.M // 2:] = X[:case.M - case.M // 2]
    if case.kind == "zero":
        return np.zeros((case.M, case.N)), 0.5
    smax = float(np.linalg.svd(X, compute_uv=False)[0])
    if case.kind == "below":
        return X, 1.5 * smax
    if case.kind == "mu0":
        return X, 0.0
    return X, 0.35 * smax


def tolerance(X, factor=TOL_FACTOR):
    return factor * min(X.shape) * EPS * float(np.linalg.norm(X))


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------------
HERE = os.path.dirname(os.path.abspath(__file__))
NUCLEAR = os.path.join(HERE, "golden", "nuclear")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(NUCLEAR, "*.npz")))
EXPECTED = ["lmc_12x20_accelerated", "lmc_12x20_adaptive", "lmc_12x20_backtracks", "lmc_12x20_plain", "lmc_20x12_adaptive", "lsq_10x14_plain",
            "shrink_9x7_adaptive"]
HISTORIES = ("residuals", "norm_residuals", "stepsizes", "objectives")
MIN_PREFIX = 30                                # a fixture may be compared on a prefix only if the prefix has at least this many iterations


def capture_script():
    """scripts/make_nuclear_golden.py as a module: the ONE place that states how the fixtures were captured."""
    path = os.path.join(HERE, os.pardir, "scripts", "make_nuclear_golden.py")
    spec = importlib.util.spec_from_file_location("make_nuclear_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load(name):
    z = np.load(os.path.join(NUCLEAR, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    return meta, z, {k[3:]: z[k] for k in z.files if k.startswith("in_")}


def compared_prefix(meta, z):
    """(iterations compared, whole run?)"""
    total = int(z["iteration_count"])
    k = min(int(meta["twin_divergence"]), total)
    return k, k == total
