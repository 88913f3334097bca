"""Inputs, geometry and models for the tests of the bilinear smooth term f(Z) = .5 ||S - X Y^T||^2, Z = [X; Y] (fh_set_factorization,
csrc/fh_bilinear.h: k_bl_prologue / k_bl_pass / k_bl_extrap / k_bl_grad).  A plain helper module, the sibling of tests/quad_cases.py: the CPU
tier (tests/test_factor_cpu.py) checks every condition claimed here, the GPU tier (tests/test_gpu_factor.py) runs the kernels.

Shapes (m, n) of S.  A work item of the pass is a row panel of PR rows x a column tile of 512 columns (one 16-byte piece per lane); a lane walks
down the panel RB = 32 / LB rows per trip (one row at LB = 16):
  1031 x 517  65 panels of 16 rows, the last one of 7 rows (so the last trip is ragged wherever a trip has several rows: 7 = 4 + 3 = 7 of 8 = 7 of 16);
              2 column tiles, the last one with 5 columns = 3 live lanes of 256 (nearly every lane idle); 130 tiles, which
              FH_TUNE_FWD_GRID_CAP = 7 does not divide: workgroups take 19 or 18 tiles; 7 workgroups of the elementwise launches
  24 x 9      2 panels (16 + 8 rows), one tile with 5 live lanes
  1 x 40, 40 x 1   a single row / a single column of S (m = 1, n = 1); K = 1 among their column counts
  200 x 300   untuned: the control
Per LB the column counts LB, LB - 1 and the fewest; both load policies.

Exactness: S holds -1, 0, 1, three quarters of the entries zero; X0, Y0 and the g0 the step starts from are multiples of 1/2, sparse and small;
tau = 1/2, coef = 1/4; the top prox kinds rotate, BOX(0, 1) on the bottom.  Every product, sum and extrapolation of init -> fwd -> adj ->
fwd_adj -> adj(accel) is then a multiple of a power of two (2^-24 at the finest: the squared gradient difference at the extrapolated point)
far below 2^53 of them whatever the order of summation and whether or not a multiply-add is fused, so a kernel's result must EQUAL the model's."""
import collections
import functools
import glob
import importlib.util
import json
import os

import numpy as np

from fasta_python_amd import hip, proximal

FH_WG = 256
BL_TC, BL_N = 512, 32                       # csrc/fh_bilinear.h
ALL_LB = (2, 4, 8, 16)
TAU, COEF = 0.5, 0.25
WIDE, NARROW, CONTROL = (1031, 517), (24, 9), (200, 300)
ROW, COLUMN = (1, 40), (40, 1)
TOP_KINDS = ("shrink", "box", "nonneg", "none")

HERE = os.path.dirname(os.path.abspath(__file__))
FACTOR = os.path.join(HERE, "golden", "factor")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(FACTOR, "*.npz")))
EXPECTED = ["gnone_40x30x2_plain", "nnf_30x30x1_adaptive", "nnf_50x70x3_adaptive", "nnf_60x40x5_accelerated", "nnf_60x40x5_adaptive",
            "nnf_60x40x5_backtracks", "nnf_60x40x5_plain", "nnf_97x33x16_accelerated", "nonneg_45x35x6_adaptive"]
HISTORIES = ("residuals", "norm_residuals", "stepsizes", "objectives")
MIN_PREFIX, MIN_BACKTRACKS = 30, 5

Case = collections.namedtuple("Case", "m n LB K cap nt kind")


def round_up(v, k):
    return (v + k - 1) // k * k


def lb_of(K):
    return 2 if K <= 2 else 4 if K <= 4 else 8 if K <= 8 else 16


def ns_of(LB):
    """GX sums of a trip that go through the reduce-scatter (csrc/fh_bilinear.h: bl_ns)."""
    return 16 if LB == 16 else BL_N


def columns_of(LB):
    """K = LB, LB - 1 and the fewest columns this LB serves (LB = 2: 2 and 1)."""
    out = [LB, LB - 1]
    fewest = LB // 2 + 1
    return out + [fewest] * (fewest not in out)


@functools.lru_cache(maxsize=None)
def cases():
    """Every (shape, K, grid cap, load policy); the four top prox kinds rotate so that each kind meets each LB."""
    out, seen = [], collections.Counter()

    def add(shape, K, cap, nt):
        LB = lb_of(K)
        out.append(Case(shape[0], shape[1], LB, K, cap, nt, TOP_KINDS[(seen[LB] + LB // 2) % 4]))
        seen[LB] += 1

    for LB in ALL_LB:
        for K in columns_of(LB):
            for nt in (0, 1):
                add(WIDE, K, 7, nt)
        for i, K in enumerate((LB, LB - 1)):
            add(NARROW, K, 0, i)
        add(CONTROL, LB, 0, -1)
    for shape in (ROW, COLUMN):
        for K in (1, 3, 16):
            add(shape, K, 0, -1)
    return tuple(out)


def case_id(c):
    return f"{c.m}x{c.n}-LB{c.LB}-K{c.K}-cap{c.cap}-nt{c.nt}-{c.kind}"


def tuning_of(case):
    t = {}
    if case.nt >= 0:
        t[hip.TUNE_NT_LOADS] = case.nt
    if case.cap:
        t[hip.TUNE_FWD_GRID_CAP] = case.cap
    return t


def expected_shape(case):
    """The hip.BilinearShape a case must be launched with, from the case's own numbers and the rule restated here once."""
    m, n, LB = case.m, case.n, case.LB
    rb = ns_of(LB) // LB
    nct = -(-n // BL_TC)
    panels = max(1, -(-512 // nct))
    pr = min(1024, max(16, round_up(-(-m // panels), 16)))
    nrp = -(-m // pr)
    last = m - (nrp - 1) * pr
    items = nrp * nct
    grid = min(items, case.cap or 512)
    nt = case.nt if case.nt >= 0 else int(round_up(m, 16) * round_up(n, 16) * 8 > 256 << 20)
    return hip.BilinearShape(LB=LB, NT=nt, tile_rows=pr, tile_cols=BL_TC, row_panels=nrp, col_tiles=nct, RB=rb, trips=pr // rb, last_rows=last,
                             last_live_rows=last - (last - 1) // rb * rb, last_live_lanes=-(-n // 2) - (nct - 1) * (BL_TC // 2), grid=grid,
                             tiles_max=-(-items // grid), tiles_min=items // grid, nelem=-(-round_up(m + n, 16) // FH_WG),
                             gx_bytes=nct * m * LB * 8, gy_bytes=nrp * n * LB * 8)


def claimed_path(case):
    """What a case's shape claims of its launch: (row panels, rows of the last panel, column tiles, live lanes of the last tile, uneven loads)."""
    return {WIDE: (65, 7, 2, 3, True), NARROW: (2, 8, 1, 5, False), CONTROL: (13, 8, 1, 150, False), ROW: (1, 1, 1, 20, False),
            COLUMN: (3, 8, 1, 1, False)}[(case.m, case.n)]


# ---- exact inputs ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_matrix(m, n):
    """(m, n) of -1, 0, 1, three quarters of the entries zero."""
    rng = np.random.RandomState(7000 + 13 * m + n)
    S = (rng.choice([-1, 1], size=(m, n)) * (rng.randint(0, 4, size=(m, n)) == 0)).astype(np.float64)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def exact_inputs(m, n, K):
    """(S, Z0, G0): Z0 = [X0; Y0] multiples of 1/2 -- X0 in [-1, 1], Y0 in [-1, 2] so that BOX(0, 1) clips both ways, each three quarters
    zero -- and the g0 the step starts from, multiples of 1/2 in [-1, 1], half of them zero."""
    S = exact_matrix(m, n)
    rng = np.random.RandomState(99 + 31 * m + 7 * n + K)
    X0 = rng.randint(-2, 3, size=(m, K)) * 0.5 * (rng.randint(0, 4, size=(m, K)) == 0)
    Y0 = rng.randint(-2, 5, size=(n, K)) * 0.5 * (rng.randint(0, 4, size=(n, K)) == 0)
    G0 = rng.randint(-2, 3, size=(m + n, K)) * 0.5 * (rng.randint(0, 2, size=(m + n, K)) == 0)
    Z0 = np.concatenate((X0, Y0))
    for V in (Z0, G0):
        V.setflags(write=False)
    return S, Z0, G0


def top_tag(kind):
    return {"shrink": lambda: proximal.Shrink(1.0), "box": lambda: proximal.Box(-0.75, 1.0), "nonneg": proximal.NonNeg, "none": proximal.NoProx}[kind]()


BOTTOM = proximal.Box(0.0, 1.0)


def _prox(tag, X, tau):
    dt = X.dtype.type
    if tag.kind == hip.PROX_SHRINK:
        return np.sign(X) * np.maximum(np.abs(X) - dt(tau) * dt(tag.mu), dt(0))
    if tag.kind == hip.PROX_NONNEG:
        return np.maximum(X, dt(0))
    if tag.kind == hip.PROX_BOX:
        return np.minimum(np.maximum(X, dt(tag.lo)), dt(tag.hi))
    assert tag.kind == hip.PROX_IDENTITY, tag.kind
    return X.copy()


MATRICES = ("GINIT", "XHAT", "XPROX", "G1", "G1A", "X1")
BLOCKS = ("init", "fwd", "adj", "adja")


def model_step(S, Z0, G0, m, top, bottom, tau=TAU, coef=COEF, dtype=np.float64, terms=None, split_gsum=True):
    """NumPy model of fh_init -> (G0 set) -> fh_fwd -> fh_adj (plain) -> fh_adj (accelerated) in `dtype`.  top / bottom: the prox tags of rows
    [0, m) and [m, m + n); bottom = None: `top` on all rows (then FH_S_GSUM runs over all rows).  Returns the matrices MATRICES and the scalar
    blocks BLOCKS (dicts from FH_S_* slot to value).  `terms`: a dict that receives, per (block, slot), the array whose sum the slot is."""
    t = np.dtype(dtype).type
    S, Z0, G0 = (np.asarray(V).astype(dtype) for V in (S, Z0, G0))
    tau, coef, half = t(tau), t(coef), t(0.5)
    out = {}

    def block(name, **slots):
        out[name] = {}
        for key, arr in slots.items():
            slot = getattr(hip, "S_" + key)
            out[name][slot] = np.max(arr) if key.startswith("GMAX") else (half * np.sum(arr) if key.startswith("FSQ") else np.sum(arr))
            if terms is not None:
                terms[(name, slot)] = arr

    def smooth(Z):
        X, Y = Z[:m], Z[m:]
        d = X @ Y.T - S
        return d, np.concatenate((d @ Y, d.T @ X))

    def gterm(Z):
        return np.abs(Z[:m]) if (bottom is not None and split_gsum) else np.abs(Z)

    d0, GI = smooth(Z0)
    block("init", FSQ=d0 * d0, GSUM=gterm(Z0), GMAX=gterm(Z0))          # (fh_init takes both g terms over the rows of the l1 term)
    Zh = Z0 - tau * G0
    Zp = _prox(top, Zh, tau) if bottom is None else np.concatenate((_prox(top, Zh[:m], tau), _prox(bottom, Zh[m:], tau)))
    dZ = Zp - Z0
    d1, G1 = smooth(Zp)
    block("fwd", FSQ=d1 * d1, DXG0=dZ * G0, DX2=dZ * dZ, XH2=(Zp - Zh) * (Zp - Zh), G02=G0 * G0, GSUM=gterm(Zp), GMAX=np.abs(Zp),
          RDOT=(Z0 - Zp) * (Zp - Z0))

    def adjoint(name, Z1, dd, Gg):
        dG = Gg + (Zh - Z0) / tau
        block(name, DXDG=dZ * dG, DG2=dG * dG, FSQ_ADJ=dd * dd, XH2_ADJ=(Z1 - Zh) * (Z1 - Zh), GSUM_ADJ=gterm(Z1), GMAX_ADJ=np.abs(Z1))

    adjoint("adj", Zp, d1, G1)
    Z1 = Zp + coef * (Zp - Z0)
    d2, G1A = smooth(Z1)
    adjoint("adja", Z1, d2, G1A)
    out.update(GINIT=GI, XHAT=Zh, XPROX=Zp, G1=G1, G1A=G1A, X1=Z1, D=(d0, d1, d2))
    return out


@functools.lru_cache(maxsize=None)
def exact_model(m, n, K, kind):
    S, Z0, G0 = exact_inputs(m, n, K)
    want = model_step(S, Z0, G0, m, top_tag(kind), BOTTOM)
    for name in MATRICES:
        want[name].setflags(write=False)
    return want


# ---- unit-scale data -----------------------------------------------------------------------------------------------------------------------------
def unit_problem(m, n, K):
    """(S, Z0, G0, tau) at unit scale: factors of the example's kind, S their noisy product, g0 a random direction."""
    rng = np.random.RandomState(555 + 31 * m + 7 * n + K)
    X, Y = rng.rand(m, K) * (rng.rand(m, K) > 0.5), rng.rand(n, K)
    S = X @ Y.T / K + 0.1 * rng.randn(m, n)
    Z0 = np.concatenate((rng.randn(m, K) * 0.5, rng.rand(n, K) * 1.5 - 0.25))
    G0 = rng.randn(m + n, K)
    return S, Z0, G0, 0.25


# (rtol, atol) of a step that is not exact: those of tests/quad_cases.py (DESIGN.md sections 11 and 13), the gradient in W's place
UNIT_TOL = {"GINIT": (1e-12, 1e-13), "XHAT": (1e-12, 1e-14), "XPROX": (1e-12, 1e-14), "G1": (1e-11, 1e-13), "G1A": (1e-11, 1e-13), "X1": (1e-12, 1e-14)}


def scalar_tol(block, slot):
    if block == "init":
        return (1e-12, 1e-13)
    if slot in (hip.S_DXDG, hip.S_DG2):
        return (1e-10, 1e-13)
    if slot in (hip.S_GSUM_ADJ, hip.S_GMAX_ADJ):
        return (1e-11, 0.0)
    return (1e-11, 1e-13)


def unit_cases():
    """(m, n, K, cap, nt): every LB with and without a padding column at the wide shape, the load policy alternating; the small shapes once."""
    out = []
    for i, LB in enumerate(ALL_LB):
        out.append(WIDE + (LB - 1 if i % 2 == 0 else LB, 7, i % 2))
    out += [NARROW + (5, 0, 0), ROW + (1, 0, -1), COLUMN + (16, 0, -1), CONTROL + (10, 0, -1)]
    return out


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------------
def capture_script():
    """scripts/make_factor_golden.py as a module: the ONE place that states how the fixtures were captured."""
    path = os.path.join(HERE, os.pardir, "scripts", "make_factor_golden.py")
    spec = importlib.util.spec_from_file_location("make_factor_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load(name):
    z = np.load(os.path.join(FACTOR, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    return meta, z, {k[3:]: z[k] for k in z.files if k.startswith("in_")}


def compared_prefix(meta, z):
    """(iterations compared, whole run?)"""
    total = int(z["iteration_count"])
    k = min(int(meta["twin_divergence"]), total)
    return k, k == total
