"""Inputs, geometry and models for the tests of the quadratic smooth term (fh_set_quadratic, csrc/fh_quad.h: k_qd_prologue / k_qd_fwd /
k_qd_grad).  A plain helper module, the sibling of tests/mc_paths.py: the CPU tier (tests/test_quad_cpu.py) checks every condition claimed
here, the GPU tier (tests/test_gpu_quad.py) runs the kernels.

Shapes (csrc/fh_quad.h walks a row of Q as k_mc_fwd walks a row of A, so the reasoning is that of tests/mc_paths.py):
  n = 1030  ld2 = 520 pieces: 3 trips of 256 lanes (5 of 128 at LB = 16), 8 live lanes in the last; FH_TUNE_FWD_GRID_CAP = 3, 4 or 5 does not
            divide the row groups, so the workgroups of k_qd_fwd make unequal numbers of passes; 5 workgroups of the elementwise launches
  n = 24    ld2 = 16: one trip, nearly every lane clamped; two row groups at R = 16
  n = 200   untuned: the control
  n = 1, 17 one entry; one row more than a padded block of 16

Exactness: Q holds -1, 0, 1, symmetric, three quarters of the entries zero; c and x0 are multiples of 1/2, tau = 1/2, coef = 1/4: every
product, sum and extrapolation of init -> fwd -> adj -> fwd_adj -> adj(accel) is a multiple of 2^-9 far below 2^53 of them whatever the order of
summation, so a kernel's result must EQUAL the model's."""
import collections
import functools
import glob
import importlib.util
import json
import os

import numpy as np

from fasta_python_amd import hip, proximal

FH_WG = 256
MC_FOR_EACH = {2: (2, 16), 4: (4, 16), 8: (8, 8), 16: (8, 8)}          # csrc/fh_multi.h: LB -> (CH, R); csrc/fh_quad.h takes the same shapes
ALL_LB = (2, 4, 8, 16)
TAU, COEF = 0.5, 0.25
N_WIDE, N_NARROW, N_CONTROL = 1030, 24, 200
PROX_KINDS = ("shrink", "box", "nonneg", "none")

HERE = os.path.dirname(os.path.abspath(__file__))
QUAD = os.path.join(HERE, "golden", "quad")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(QUAD, "*.npz")))
EXPECTED = ["gnone_50_plain", "group_64x6_adaptive", "maxnorm_130x10_adaptive", "maxnorm_60x5_accelerated", "maxnorm_60x5_adaptive",
            "maxnorm_60x5_plain", "maxnorm_75x3_plain", "maxnorm_97x16_accelerated", "nonneg_70x2_accelerated", "shrink_90_adaptive",
            "svm_rbf_80_accelerated", "svm_rbf_80_adaptive", "svm_rbf_80_backtracks", "svm_rbf_80_c10_adaptive", "svm_rbf_80_plain"]
HISTORIES = ("residuals", "norm_residuals", "stepsizes", "objectives")
MIN_PREFIX = 30                                # a fixture may be compared on a prefix only if the prefix has at least this many iterations

Case = collections.namedtuple("Case", "n LB L cap nt kind")


def round_up(v, k):
    return (v + k - 1) // k * k


def lb_of(L):
    return 2 if L <= 2 else 4 if L <= 4 else 8 if L <= 8 else 16


def uneven_cap(nrg):
    cap = 3
    while nrg % cap == 0:
        cap += 1
    return cap


def columns_of(LB):
    """L = LB, LB - 1 and the fewest columns this LB serves (LB = 2: 2 and 1, the vector unknown)."""
    out = [LB, LB - 1]
    fewest = LB // 2 + 1
    return out + [fewest] * (fewest not in out)


@functools.lru_cache(maxsize=None)
def cases():
    """Every (n, L, grid cap, load policy); the four exact prox kinds rotate so that each kind meets each LB."""
    out, seen = [], collections.Counter()

    def add(n, L, cap, nt):
        LB = lb_of(L)
        out.append(Case(n, LB, L, cap, nt, PROX_KINDS[(seen[LB] + LB // 2) % 4]))
        seen[LB] += 1

    for LB in ALL_LB:
        R = MC_FOR_EACH[LB][1]
        for L in columns_of(LB):
            for nt in (0, 1):
                add(N_WIDE, L, uneven_cap(round_up(N_WIDE, 16) // R), nt)
        for L in (LB, LB - 1):
            for nt in (0, 1):
                add(N_NARROW, L, 0, nt)
        for i, L in enumerate((LB, LB - 1)):
            add(N_CONTROL, L, 0, -1 if i == 0 else i % 2)
    for n in (1, 17):
        for L in (1, 3, 16):
            add(n, L, 0, -1)
    return tuple(out)


def case_id(c):
    return f"n{c.n}-LB{c.LB}-L{c.L}-cap{c.cap}-nt{c.nt}-{c.kind}"


def tuning_of(case):
    t = {}
    if case.nt >= 0:
        t[hip.TUNE_NT_LOADS] = case.nt
    if case.cap:
        t[hip.TUNE_FWD_GRID_CAP] = case.cap
    return t


def expected_shape(case):
    """The hip.QuadShape a case must be launched with, from the case's own numbers and the rules restated here once."""
    CH, R = MC_FOR_EACH[case.LB]
    ld = round_up(case.n, 16)
    ld2, nrg = ld // 2, ld // R
    lanes = FH_WG * CH // case.LB
    grid = min(nrg, case.cap or 512)
    ntrip = -(-ld2 // lanes)
    nt = case.nt if case.nt >= 0 else int(ld * ld * 8 > 256 << 20)
    return hip.QuadShape(LB=case.LB, CH=CH, R=R, NT=nt, fwd_grid=grid, nrg=nrg, ntrip=ntrip, last_live=ld2 - (ntrip - 1) * lanes,
                         pass_max=-(-nrg // grid), pass_min=nrg // grid, npro=-(-ld // FH_WG), ngrad=-(-ld // FH_WG))


def claimed_path(case):
    """What the case's n claims of its launch: (trips at LB < 16, trips at LB = 16, live lanes of the last trip, uneven passes)."""
    return {N_WIDE: (3, 5, 8, True), N_NARROW: (1, 1, 16, False), N_CONTROL: (1, 1, 104, False), 1: (1, 1, 8, False), 17: (1, 1, 16, False)}[case.n]


# ---- exact inputs ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_matrix(n):
    """(n, n) of -1, 0, 1, symmetric, three quarters of the entries zero."""
    rng = np.random.RandomState(5000 + n)
    U = np.triu(rng.choice([-1, 1], size=(n, n)) * (rng.randint(0, 4, size=(n, n)) == 0))
    Q = (U + np.triu(U, 1).T).astype(np.float64)
    Q.setflags(write=False)
    return Q


def _shape(n, L):
    return (n, L)


@functools.lru_cache(maxsize=None)
def exact_inputs(n, L):
    """(Q, c, X0): c multiples of 1/2 in [-1, 1], two thirds zero; X0 multiples of 1/2 in [-2, 2]."""
    Q = exact_matrix(n)
    rng = np.random.RandomState(77 + 31 * n + L)
    X0 = rng.randint(-4, 5, size=_shape(n, L)) * 0.5
    c = rng.randint(-2, 3, size=_shape(n, L)) * 0.5 * (rng.randint(0, 3, size=_shape(n, L)) == 0)
    for V in (X0, c):
        V.setflags(write=False)
    return Q, c, X0


def prox_tag(kind):
    return {"shrink": lambda: proximal.Shrink(1.0), "box": lambda: proximal.Box(-1.5, 2.0), "nonneg": proximal.NonNeg, "none": proximal.NoProx,
            "group": lambda: proximal.GroupShrink(1.0), "rowball": lambda: proximal.RowBall(1.0)}[kind]()


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
    if tag.kind == hip.PROX_ROWBALL:
        nu = np.sqrt(np.sum(X * X, axis=1))
        return dt(tag.mu) * X / (np.maximum(nu, dt(tag.mu)) + (nu == 0))[:, None]
    assert tag.kind == hip.PROX_IDENTITY, tag.kind
    return X.copy()


def _gsum(tag, X):
    if tag.kind == hip.PROX_GROUP:
        return np.sum(np.sqrt(np.sum(X * X, axis=1)))
    return np.sum(np.abs(X))


MATRICES = ("G0", "XHAT", "XPROX", "W", "G1", "G1A", "X1")
BLOCKS = ("init", "fwd", "adj", "adja")


def model_step(Q, c, X0, tag, tau=TAU, coef=COEF, dtype=np.float64, terms=None):
    """NumPy model of fh_init -> fh_fwd -> fh_adj (plain) -> fh_adj (accelerated) in `dtype` for f(X) = .5 <X, Q X> + <c, X>.  Returns the
    matrices MATRICES and the scalar blocks BLOCKS (dicts from FH_S_* slot to value).  `terms`: a dict that receives, per (block, slot), the
    array whose sum the slot is -- what the CPU tier sums once more in integers."""
    t = np.dtype(dtype).type
    Q, c, X0 = (np.asarray(V).astype(dtype) for V in (Q, c, X0))
    tau, coef, half = t(tau), t(coef), t(0.5)
    out = {}

    def block(name, **slots):
        out[name] = {}
        for key, arr in slots.items():
            slot = getattr(hip, "S_" + key)
            out[name][slot] = np.max(arr) if key.startswith("GMAX") else np.sum(arr)
            if terms is not None:
                terms[(name, slot)] = arr

    def gterm(X):
        return np.sqrt(np.sum(X * X, axis=1)) if tag.kind == hip.PROX_GROUP else np.abs(X)

    W0 = Q @ X0
    G0 = W0 + c
    block("init", FSQ=X0 * (half * W0 + c), GSUM=gterm(X0), GMAX=np.abs(X0))
    Xh = X0 - tau * G0
    Xp = _prox(tag, Xh, tau)
    dX, W = Xp - X0, Q @ Xp
    block("fwd", FSQ=Xp * (half * W + c), DXG0=dX * G0, DX2=dX * dX, XH2=(Xp - Xh) * (Xp - Xh), G02=G0 * G0, GSUM=gterm(Xp), GMAX=np.abs(Xp),
          RDOT=(X0 - Xp) * (Xp - X0))

    def adjoint(name, X1, W1):
        G1 = W1 + c
        dG = G1 + (Xh - X0) / tau
        block(name, DXDG=dX * dG, DG2=dG * dG, FSQ_ADJ=X1 * (half * W1 + c), XH2_ADJ=(X1 - Xh) * (X1 - Xh), GSUM_ADJ=gterm(X1), GMAX_ADJ=np.abs(X1))
        return G1

    G1 = adjoint("adj", Xp, W)
    X1, W1 = Xp + coef * (Xp - X0), W + coef * (W - W0)
    G1A = adjoint("adja", X1, W1)
    out.update(G0=G0, XHAT=Xh, XPROX=Xp, W=W, G1=G1, G1A=G1A, X1=X1)
    return out


@functools.lru_cache(maxsize=None)
def exact_model(n, L, kind):
    Q, c, X0 = exact_inputs(n, L)
    want = model_step(Q, c, X0, prox_tag(kind))
    for name in MATRICES:
        want[name].setflags(write=False)
    return want


# ---- a step that is not exact: GROUP / ROWBALL ---------------------------------------------------------------------------------------------------
def rownorm_problem(n, L, kind):
    """(Q, c, X0, tau, tag) for a GroupShrink / RowBall step on unit-scale data (Q = exact_matrix / 8, a power of two: the same pattern): the
    threshold sits at 0.8 of the median row norm of xhat, so some rows vanish / lie inside the ball and the others shrink / are projected."""
    Q = exact_matrix(n) * 0.125
    rng = np.random.RandomState(321 + 31 * n + L)
    X0 = rng.randn(n, L) * 0.1
    c = rng.randn(n, L) * 0.5
    tau = 0.25
    norms = np.linalg.norm(X0 - tau * (Q @ X0 + c), axis=1)
    med = float(np.round(0.8 * np.median(norms), 3))
    tag = proximal.GroupShrink(med / tau) if kind == "group" else proximal.RowBall(med)
    return Q, c, X0, tau, tag


# (rtol, atol) of a step that is not exact: those of tests/sparse_lanes.py, W in Z's place
ROWNORM_TOL = {"G0": (1e-12, 1e-13), "XHAT": (1e-12, 1e-14), "XPROX": (1e-12, 1e-14), "W": (1e-12, 1e-13), "G1": (1e-11, 1e-13),
               "G1A": (1e-11, 1e-13), "X1": (1e-12, 1e-14)}


def scalar_tol(block, slot):
    if block == "init":
        return (1e-12, 1e-13)
    if slot in (hip.S_DXDG, hip.S_DG2):
        return (1e-10, 1e-13)
    if slot in (hip.S_GSUM_ADJ, hip.S_GMAX_ADJ):
        return (1e-11, 0.0)
    return (1e-11, 1e-13)           # (f itself included: unlike a sum of squares it cancels, so it gets the absolute term too)


def rownorm_cases():
    """(n, L, kind, nt): every LB with and without a padding column, both kinds, the load policy alternating."""
    out = []
    for i, LB in enumerate(ALL_LB):
        for j, kind in enumerate(("group", "rowball")):
            out.append((N_WIDE, LB - 1 if (i + j) % 2 == 0 else LB, kind, (i + j) % 2))
            out.append((N_NARROW, LB if (i + j) % 2 == 0 else LB - 1, kind, (i + j + 1) % 2))
    out.append((17, 3, "rowball", 0))
    return [r for r in out if r[1] >= 2]                # (the two kinds couple the columns of a row: a matrix unknown)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------------
def capture_script():
    """scripts/make_quad_golden.py as a module: the ONE place that states how the fixtures were captured."""
    path = os.path.join(HERE, os.pardir, "scripts", "make_quad_golden.py")
    spec = importlib.util.spec_from_file_location("make_quad_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load(name):
    z = np.load(os.path.join(QUAD, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    return meta, z, {k[3:]: z[k] for k in z.files if k.startswith("in_")}


def compared_prefix(meta, z):
    """(iterations compared, whole run?)"""
    total = int(z["iteration_count"])
    k = min(int(meta["twin_divergence"]), total)
    return k, k == total
