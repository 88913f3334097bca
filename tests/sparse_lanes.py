"""Inputs and exact models for the tests of the sparse gather kernels (csrc/fh_sparse.h, csrc/fh_spmulti.h): matrices that land on a chosen
kernel instantiation, operands on which float64 arithmetic is EXACT, and a NumPy model of one step.  A plain helper module: the CPU tier
(tests/test_sparse_lanes_cpu.py) checks every condition claimed here, the GPU tier (tests/test_gpu_sparse_lanes.py) runs the kernels.

The instantiation is chosen by the host (csrc/fasta_hip.hip: sp_upload_side) from the mean row length of each copy of the operator and the
column count of the unknown; lanes_of restates that rule once.  exact_matrix(G, LB, seed) is a matrix whose both copies resolve to G.

Exactness: every matrix holds small integers, every operand multiples of 1/2, tau = 1/2 and the FISTA coefficient 1/4, so every product,
sum, quotient by tau and extrapolation of a step is a multiple of 1/16 (its squares of 1/256) far below 2^53 of them: float64 represents
every intermediate of every summation order, and a kernel's result must EQUAL the model's, whatever its lanes, trees and partial sums."""
import collections

import numpy as np
from scipy import sparse as sp

from fasta_python_amd import hip, proximal

FH_WG = 256                                   # csrc/fh_device.h
SP_LONG_FACTOR, SP_LONG_MEANS = 64, 16        # csrc/fh_sparse.h
ALL_LB = (2, 4, 8, 16)
PAIRS = [(G, LB) for LB in ALL_LB for G in (4, 8, 16, 32, 64) if G >= max(4, LB // 2)]          # SPMC_FOR_EACH of csrc/fh_spmulti.h
VECTOR_G = [4, 8, 16, 32, 64]                                                                 # SP_FOR_EACH of csrc/fh_sparse.h
TAU, COEF = 0.5, 0.25

Lanes = collections.namedtuple("Lanes", "G E longer long_rows")


def column_lanes(LB):
    """C: lanes per gathered row of the operand -- 1 for a vector unknown (LB = 0), LB / 2 for a matrix unknown."""
    return max(1, LB // 2)


def lb_of(L):
    """Device columns per row of an (n, L) unknown; 0 for the vector form (L None or 0)."""
    return 0 if not L else next(lb for lb in ALL_LB if lb >= L)


def lanes_of(M, C):
    """The host's rule for one copy `M` (CSR: A, or A^T by rows) at C column lanes, restated once: a group of G lanes works on E = G / C
    entries per trip; G is the smallest of max(4, C) .. 64 with 2 E >= the mean row length; a row is long (a workgroup of its own) beyond
    max(64 E, 16 mean rows) entries."""
    M = M.tocsr()
    lens = np.diff(M.indptr)
    mean = M.nnz / M.shape[0] if M.shape[0] else 0.0
    G = max(4, C)
    while G < 64 and 2.0 * (G // C) < mean:
        G *= 2
    E = G // C
    longer = max(SP_LONG_FACTOR * E, int(SP_LONG_MEANS * mean))
    return Lanes(G, E, longer, np.flatnonzero(lens > longer))


def both_lanes(S, LB):
    """(lanes of A by rows, lanes of A^T by rows) at LB device columns."""
    return lanes_of(S.tocsr(), column_lanes(LB)), lanes_of(S.T.tocsr(), column_lanes(LB))


def row_ranges(M, C, ncu=256):
    """part[0 .. nwg] of sp_upload_side: contiguous row ranges balanced by the trips a group spends on a row, ceil(len / E) + 2 (a long row
    costs 1), for at most 8 workgroups per compute unit."""
    M = M.tocsr()
    la = lanes_of(M, C)
    rows = M.shape[0]
    lens = np.diff(M.indptr)
    cost = np.where(lens > la.longer, 1, (lens + la.E - 1) // la.E + 2)
    groups = FH_WG // la.G
    nwg = max(1, min((rows + groups - 1) // groups, max(1, ncu) * 8))
    total = int(cost.sum())
    part = [0]
    run, r = 0, 0
    for w in range(1, nwg):
        goal = (total * w + nwg - 1) // nwg
        while r < rows and run < goal:
            run += int(cost[r])
            r += 1
        part.append(r)
    part.append(rows)
    return np.array(part)


# ---- matrices ------------------------------------------------------------------------------------------------------------------------------
def _int_values(rng, k):
    return (rng.randint(1, 4, size=k) * rng.choice([-1, 1], size=k)).astype(np.float64)          # non-zero integers in [-3, 3]


def _csr(m, n, rows, cols, vals):
    S = sp.csr_matrix((vals, (rows, cols)), shape=(m, n))
    S.sort_indices()
    return S


def exact_matrix(G, LB, seed=0):
    """230 x 251, both copies on exactly G lanes per row at LB columns (LB = 0: the vector form).  Every row holds 2 E - 1 entries (2 when
    E = 1) at random distinct columns -- the last lane of a group walks one entry fewer than the others -- except every 37th row from row 5,
    which is empty; the last three columns are empty."""
    m, n = 230, 251
    E = G // column_lanes(LB)
    per = 2 if E == 1 else 2 * E - 1
    rng = np.random.RandomState(1000 * LB + G + 7919 * seed)
    rows, cols = [], []
    for r in range(m):
        if r % 37 == 5:
            continue
        rows.append(np.full(per, r))
        cols.append(rng.choice(n - 3, size=per, replace=False))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return _csr(m, n, rows, cols, _int_values(rng, rows.size))


def long_matrix(LB, seed=0):
    """601 x 703 with 3 entries per row, one dense row (311) and one dense column (407): both copies hand exactly one row to a whole
    workgroup at every LB in {0, 2, 4, 8, 16}."""
    m, n = 601, 703
    rng = np.random.RandomState(5000 + LB + 7919 * seed)
    D = np.zeros((m, n))
    for r in range(m):
        D[r, rng.choice(n, size=3, replace=False)] = _int_values(rng, 3)
    D[311, :] = _int_values(rng, n)
    D[:, 407] = _int_values(rng, m)
    S = sp.csr_matrix(D)
    S.sort_indices()
    return S


def staircase(seed=0):
    """400 x 400, row r holds r % 97 entries: rows of 0 .. 96 entries next to each other, so the trip-balanced row ranges are uneven -- some
    workgroups own more rows than they have groups (two trips of the row loop), some fewer (idle groups in the only trip)."""
    m = n = 400
    rng = np.random.RandomState(9000 + 7919 * seed)
    rows, cols = [], []
    for r in range(m):
        k = r % 97
        rows.append(np.full(k, r))
        cols.append(rng.choice(n, size=k, replace=False))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return _csr(m, n, rows, cols, _int_values(rng, rows.size))


# ---- operands ------------------------------------------------------------------------------------------------------------------------------
def _shape(k, L):
    return (k,) if not L else (k, L)


def apply_operands(S, L, seed=0):
    """(V, W): integer operands in [-4, 4] for A V and A^T W."""
    m, n = S.shape
    rng = np.random.RandomState(77 + 7919 * seed + (L or 0))
    return rng.randint(-4, 5, size=_shape(n, L)).astype(np.float64), rng.randint(-4, 5, size=_shape(m, L)).astype(np.float64)


def step_operands(S, L, seed=0):
    """(X0, B) for one exact step: X0 holds multiples of 1/2 in [-2, 2], and B = A X0 + N with N multiples of 1/2 in [-1, 1], two thirds of
    them zero -- the first residual is N, so the gradients stay small enough for every later sum to be exact (the CPU tier checks it)."""
    m, n = S.shape
    rng = np.random.RandomState(99 + 7919 * seed + (L or 0))
    X0 = rng.randint(-4, 5, size=_shape(n, L)) * 0.5
    N = rng.randint(-2, 3, size=_shape(m, L)) * 0.5 * (rng.randint(0, 3, size=_shape(m, L)) == 0)
    return X0, S @ X0 + N


def group_problem(S, L, seed=0):
    """(A, X0, B, tau, mu) for a GroupShrink step, which is not exact (a square root and a division per row) and is held to the mixed
    relative / absolute tolerances of tests/test_gpu_sparse_mmv.py.  Those were set for unit-scale data, so A = S / 8 (a power of two: the
    same pattern, the same lanes; the longest rows, 127 entries, then have the squared norm of that test's rows), X0 and the noise of B are
    of its sizes, and the threshold tau * mu sits at 0.8 of the median row norm of xhat: some rows vanish, the others shrink."""
    A = (S * 0.125).tocsr() if sp.issparse(S) else np.asarray(S) * 0.125
    m, n = A.shape
    rng = np.random.RandomState(123 + 7919 * seed + L)
    X0 = rng.randn(n, L) * 0.1
    B = A @ X0 + rng.randn(m, L) * 0.5
    tau = 0.25
    norms = np.linalg.norm(X0 - tau * (A.T @ (A @ X0 - B)), axis=1)
    return A, X0, B, tau, float(np.round(0.8 * np.median(norms) / tau, 3))


PROX_KINDS = ("shrink", "box", "nonneg", "none")


def prox_tag(kind):
    return {"shrink": lambda: proximal.Shrink(1.0), "box": lambda: proximal.Box(-1.5, 2.0), "nonneg": proximal.NonNeg, "none": proximal.NoProx}[kind]()


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
def dense_of(S):
    """The operator as a dense ndarray: a scipy matrix is expanded, a dense array (tests/mc_paths.py) is taken as it is."""
    return np.asarray(S.todense()) if sp.issparse(S) else np.asarray(S)


def _prox(tag, X, tau):
    dt = X.dtype.type
    if tag.kind == hip.PROX_SHRINK:
        return np.sign(X) * np.maximum(np.abs(X) - dt(tau) * dt(tag.mu), dt(0))
    if tag.kind == hip.PROX_NONNEG:
        return np.maximum(X, dt(0))
    if tag.kind == hip.PROX_BOX:
        return np.minimum(np.maximum(X, dt(tag.lo)), dt(tag.hi))
    if tag.kind == hip.PROX_GROUP:
        nu = np.sqrt(np.sum(X * X, axis=1))
        scale = np.maximum(nu - dt(tau) * dt(tag.mu), dt(0)) / (nu + (nu == 0))
        return X * scale[:, None]
    assert tag.kind == hip.PROX_IDENTITY, tag.kind
    return X.copy()


def _gsum(tag, X):
    if tag.kind == hip.PROX_GROUP:
        return np.sum(np.sqrt(np.sum(X * X, axis=1)))
    return np.sum(np.abs(X))


def row_norm_sum(X):
    """Sum of the Euclidean row norms of X in extended precision."""
    X = np.asarray(X, dtype=np.longdouble)
    return np.sum(np.sqrt(np.sum(X * X, axis=1)))


def exact_step(S, X0, B, tag, tau=TAU, coef=COEF, dtype=np.float64):
    """NumPy model of fh_init -> fh_fwd -> fh_adj (plain) -> fh_adj (accelerated) in `dtype`, least squares; S a scipy matrix or a dense
    array.  Returns a dict: the matrices
    G0, XHAT, XPROX, Z, G1 (plain adjoint), G1A and X1 (accelerated adjoint), and the scalar blocks `init`, `fwd`, `adj`, `adja`, each a
    dict from FH_S_* slot to value -- the slots tests/test_gpu_sparse*.py:test_single_step_scalars_match_numpy check."""
    A = dense_of(S).astype(dtype)
    t = np.dtype(dtype).type
    X0, B = np.asarray(X0).astype(dtype), np.asarray(B).astype(dtype)
    tau, coef = t(tau), t(coef)
    sq = lambda V: np.sum(V * V)
    Z0 = A @ X0
    G0 = A.T @ (Z0 - B)
    out = {"G0": G0, "init": {hip.S_FSQ: sq(Z0 - B), hip.S_GSUM: _gsum(tag, X0)}}
    Xh = X0 - tau * G0
    Xp = _prox(tag, Xh, tau)
    dX, Z = Xp - X0, A @ Xp
    out.update(XHAT=Xh, XPROX=Xp, Z=Z)
    out["fwd"] = {hip.S_FSQ: sq(Z - B), hip.S_DXG0: np.sum(dX * G0), hip.S_DX2: sq(dX), hip.S_XH2: sq(Xp - Xh), hip.S_G02: sq(G0),
                  hip.S_GSUM: _gsum(tag, Xp), hip.S_GMAX: np.max(np.abs(Xp)), hip.S_RDOT: np.sum((X0 - Xp) * (Xp - X0))}

    def adjoint(X1, Z1):
        G1 = A.T @ (Z1 - B)
        dG = G1 + (Xh - X0) / tau
        return G1, {hip.S_DXDG: np.sum(dX * dG), hip.S_DG2: sq(dG), hip.S_FSQ_ADJ: sq(Z1 - B), hip.S_XH2_ADJ: sq(X1 - Xh),
                    hip.S_GSUM_ADJ: _gsum(tag, X1), hip.S_GMAX_ADJ: np.max(np.abs(X1))}

    out["G1"], out["adj"] = adjoint(Xp, Z)
    X1, Z1 = Xp + coef * (Xp - X0), Z + coef * (Z - Z0)
    out["X1"] = X1
    out["G1A"], out["adja"] = adjoint(X1, Z1)
    return out


MATRICES = ("G0", "XHAT", "XPROX", "Z", "G1", "G1A", "X1")
BLOCKS = ("init", "fwd", "adj", "adja")

# (rtol, atol) a step that is NOT exact (GroupShrink) is held to: those of tests/test_gpu_sparse_mmv.py:test_single_step_scalars_match_numpy
GROUP_TOL = {"G0": (1e-12, 1e-13), "XHAT": (1e-12, 1e-14), "XPROX": (1e-12, 1e-14), "Z": (1e-12, 1e-13), "G1": (1e-11, 1e-13),
             "G1A": (1e-11, 1e-13), "X1": (1e-12, 1e-14)}


def scalar_tol(block, slot):
    if block == "init":
        return (1e-12, 0.0)
    if slot in (hip.S_DXDG, hip.S_DG2):
        return (1e-10, 1e-13)
    if slot in (hip.S_FSQ_ADJ, hip.S_GSUM_ADJ):
        return (1e-11, 0.0)
    if slot == hip.S_GMAX_ADJ:
        return (1e-12, 0.0)
    return (1e-11, 1e-13)


# ---- the cases, shared by the CPU tier (conditions on the inputs) and the GPU tier (the kernels) --------------------------------------------
def step_cases():
    """(G, LB, L, prox kind) of the exact one-step tests: every matrix pair and every vector G (LB = 0, L = None); the prox kind rotates so
    that each kind meets every LB, the column count alternates between LB (no padding column) and LB - 1 (LB = 2: 2 and 1)."""
    out = []
    for LB in (0,) + ALL_LB:
        Gs = VECTOR_G if LB == 0 else [G for G, lb in PAIRS if lb == LB]
        for i, G in enumerate(Gs):
            L = None if LB == 0 else (LB if i % 2 == 0 else LB - 1)
            out.append((G, LB, L, PROX_KINDS[(i + LB // 2) % 4]))
    return out


def apply_cases():
    """(G, LB, L) of the exact apply tests: every pair with and without a padding column, and every vector G."""
    out = [(G, 0, None) for G in VECTOR_G]
    for G, LB in PAIRS:
        out += [(G, LB, LB), (G, LB, LB - 1)]
    return out


def group_cases():
    """(G, LB, L) of the GroupShrink step tests: every pair, the column count alternating the other way round."""
    return [(G, LB, LB - 1 if i % 2 == 0 else LB) for i, (G, LB) in enumerate(PAIRS)]
