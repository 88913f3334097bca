"""The stations of tests/test_gpu_carry.py: one operator form each, with one short program, built from the case modules the form's own suite
uses (the "home" modules) -- never from new models -- so that ONE context can be carried through every form and every number it returns compared.

What a change of operator keeps: the arrival counters, the scalar block with the clipping level that warm-starts the
next level search, every FH_TUNE_* value and -- through the dense setters -- the solver flags.  A station therefore states its tuning IN FULL
(TUNING_AUTO first, then its own keys), sets its operator before its loss and prox, runs its program and reads back every scalar block and
every vector a launch wrote.  The numbers are held two ways:

  * against the home module's model, by the home suite's own comparison (imported: `==` where the home suite is exact, the home tolerance
    where it is not);
  * against the SAME program on a fresh context (`fresh`), bit for bit -- all stations but the level-search ones, whose clipping level the
    home suites hold to a tolerance and which start their search from whatever level the context last held.

tests/test_carry_cpu.py checks, without a device, that the list is complete; tests/test_gpu_carry.py runs the transitions."""
import collections
import json

import numpy as np

import fasta_python_amd as fa
from fasta_python_amd import certificates as ce
from fasta_python_amd import hip
from oracle import fasta_np as fo
from tests import completion_cases as CC
from tests import conv_cases as CV
from tests import dct2_cases as D2
from tests import dct_cases as D1
from tests import factor_cases as FC
from tests import fused_paths as FP
from tests import gap_cases as GC
from tests import mc_paths as MC
from tests import nuclear_cases as NC
from tests import quad_cases as QC
from tests import refusal_cases as RC
from tests import run_paths as RP
from tests import softmax_cases as SM
from tests import sparse_lanes as SL
from tests import tv3d_cases as T3
from tests import tv_paths as TV

HOME_MODULES = (FP, RP, MC, SL, TV, T3, QC, FC, D1, D2, CV, NC, CC, SM, GC)

# ---- tuning ------------------------------------------------------------------------------------------------------------------------------------
# Every FH_TUNE_* key hip.py mirrors (but TEST_HOOKS, which no station sets) at its automatic value.  Two keys have no way back to "automatic"
# once written (csrc/fasta_hip.hip:set_tuning_one): NT_LOADS (the context starts at -1; a write leaves 0 or 1) and FUSED_VARIANT (a write clears
# fused_variant_auto).  They stand here at what the automatic rule resolves to on every station's shape -- plain loads below 256 MiB of matrix,
# the scheduling word 2 | 32 with the floor of 16 rows per team -- and a fresh context writes them too, so both sides of a comparison hold the same.
TUNING_AUTO = {getattr(hip, k): 0 for k in vars(hip) if k.startswith("TUNE_") and k != "TUNE_TEST_HOOKS"}
TUNING_AUTO[hip.TUNE_SEQ_POLL] = 1
TUNING_AUTO[hip.TUNE_FUSED_VARIANT] = (16 << 16) | 34
# keys the shipped library refuses to write on a carried context: the experimental sweep forms (FH_E_ARG in the shipped library) and LD_PAD
# ("must be set before the matrix": FH_E_STATE once any operator is held).  No station changes them, so they stay at the value fh_create gave.
NEVER_WRITTEN = frozenset(hip.EXPERIMENTAL_KEYS) | {hip.TUNE_LD_PAD}


def write_tuning(c, own):
    """TUNING_AUTO, then the station's own keys: the station behaves the same whatever ran before it."""
    assert hip.TUNE_TEST_HOOKS not in own and not set(own) & NEVER_WRITTEN
    for key, value in {**TUNING_AUTO, **own}.items():
        if key not in NEVER_WRITTEN:
            c.set_tuning(key, value)


# ---- traces ------------------------------------------------------------------------------------------------------------------------------------
VEC = {"X0": hip.VEC_X0, "G0": hip.VEC_G0, "XHAT": hip.VEC_XHAT, "XPROX": hip.VEC_XPROX, "X1": hip.VEC_X1, "G1": hip.VEC_G1, "BEST": hip.VEC_BEST,
       "Z": hip.VEC_Z}
N_SIDE = ("X0", "G0", "XHAT", "XPROX", "X1", "G1", "BEST")
NO_GRADIENT = ("X0", "XPROX", "X1", "BEST", "Z")          # the 2-D stencil never materialises g0, g1 or xhat (csrc/fh_host_ctx.h:vec_ptr)


class Trace(collections.OrderedDict):
    """name -> array of everything a program read back, in order"""

    def put(self, name, value):
        assert name not in self, name
        self[name] = np.array(value, dtype=np.float64, copy=True)

    def read(self, c, tag, names):
        (m, n), L = c.shape(), c.rhs or 1
        for v in names:
            self.put(f"{tag}.{v}", c.get_vector(VEC[v], (m if v == "Z" else n) * L))

    def padding(self, c, tag, names):
        """the padding behind the n-side vectors is zero (the idiom of tests/test_gpu_run_paths.py:padding_is_zero, for any column count)"""
        from tests.test_gpu_run_paths import padding_is_zero
        n, L = c.shape()[1], c.rhs or 1
        self.put(f"{tag}.padding", [padding_is_zero(c, VEC[v], n * L) for v in names])
        assert self[f"{tag}.padding"].all(), (tag, names, self[f"{tag}.padding"])

    def home(self, tag, got):
        """what a home suite's run_step returned (a dict, a tuple of dicts or a list of arrays), flattened"""
        if isinstance(got, dict):
            for k, v in got.items():
                self.home(f"{tag}.{k}", v)
        elif isinstance(got, (list, tuple)) and not np.isscalar(got) and any(isinstance(v, (dict, np.ndarray, list, tuple)) for v in got):
            for i, v in enumerate(got):
                self.home(f"{tag}.{i}", v)
        else:
            self.put(tag, got)


def first_difference(a, b):
    """None if two traces hold the same names and the same bits (NaN == NaN: the nuclear ball reports g as NaN where it is not free)"""
    if list(a) != list(b):
        return f"names differ: {[k for k in a if k not in b]} / {[k for k in b if k not in a]}"
    for k in a:
        if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k], equal_nan=True):
            bad = np.flatnonzero(~((a[k] == b[k]) | (np.isnan(a[k]) & np.isnan(b[k]))).ravel()) if a[k].shape == b[k].shape else []
            where = f", first at {bad[0]}: {a[k].ravel()[bad[0]]!r} != {b[k].ravel()[bad[0]]!r}" if len(bad) else ""
            return f"{k}: {len(bad)} entries differ{where}"
    return None


def tail(c, t, tau, coef, names=N_SIDE + ("Z",), accel=True):
    """What follows the home suite's step on the same context: commit, the pair under one synchronisation, an accelerated attempt, commit --
    the launches that start from a committed state and the pointer rotation of fh_commit.  No home model covers them: held against `fresh`."""
    c.commit()
    t.read(c, "commit1", [v for v in names if v in ("X0", "G0")])
    t.put("tail.pair", c.fwd_adj(tau))
    t.read(c, "tail.pair", [v for v in names if v in ("XHAT", "XPROX", "Z", "G1")])
    if accel:
        t.put("tail.fwd", c.fwd(tau))
        t.put("tail.adja", c.adj(tau, True, coef))
        t.read(c, "tail.adja", [v for v in names if v in ("G1", "X1")])
    c.commit(True)
    t.read(c, "commit2", [v for v in names if v in ("X0", "G0", "BEST")])


def assert_blocks(got, want, matrices, blocks):
    """the comparison of the exact home suites (tests/test_gpu_mc_paths.py:assert_exact_step and its siblings): `==` on every keyed matrix and scalar"""
    for name in matrices:
        assert got[name].shape == np.shape(want[name]) and np.array_equal(got[name], want[name]), name
    for block in blocks:
        for slot, v in want[block].items():
            assert got[block][slot] == v, f"{block} scalar {slot}: {got[block][slot]!r} != {v!r}"


def assert_close_blocks(got, want, matrices, blocks, mat_tol, scalar_tol):
    """... and of the home suites that hold a square root and a division per row to a tolerance (GroupShrink, RowBall): the home module's numbers"""
    for name in matrices:
        rtol, atol = mat_tol[name]
        np.testing.assert_allclose(got[name], np.asarray(want[name], dtype=np.float64), rtol=rtol, atol=atol, err_msg=name)
    for block in blocks:
        for slot, v in want[block].items():
            rtol, atol = scalar_tol(block, slot)
            assert abs(got[block][slot] - float(v)) <= rtol * abs(float(v)) + atol, (block, slot, got[block][slot], float(v))


# ---- the station -------------------------------------------------------------------------------------------------------------------------------
class Station:
    """name; setter: the entry of refusal_cases.SETTERS whose calls put the operator in; op: its OP_* form; home: the case module its operands
    and model come from; tuning: its own keys; run(c, t): setter, loss, prox, operands, the shape assertion, the program, the home comparison
    -- everything read goes into the Trace t; bitwise: held against `fresh` bit for bit; storage: of the context it needs;
    tau: a step size at which fh_fwd / fh_adj may be called again once the program has ended (the leaving states of the GPU tier)."""

    def __init__(self, name, setter, home, run, tuning=None, bitwise=True, storage="f64", tau=0.5, exact=True, leaves_lazy=False, dense=False):
        self.name, self.setter, self.home, self._run, self.tuning = name, setter, home, run, dict(tuning or {})
        self.bitwise, self.storage, self.tau, self.exact, self.leaves_lazy, self.dense = bitwise, storage, tau, exact, leaves_lazy, dense
        self.op = RC.OP_OF.get(setter, "OP_DENSE")

    def __repr__(self):
        return self.name

    def run(self, c):
        t = Trace()
        write_tuning(c, self.tuning)
        self._run(c, t)
        t.put("timeout word", [c.recovered_count(k) for k in (hip.RECOVERED_LEVEL_FALLBACK, hip.RECOVERED_LEVEL_FAILED, hip.RECOVERED_RUN_TIMEOUT)])
        return t


_FRESH, _MEMO = {}, {}


def once(key, thunk):
    """operands and host models are computed once per process and shared (never modified: a station only reads them)"""
    if key not in _MEMO:
        _MEMO[key] = thunk()
    return _MEMO[key]


def fresh(station):
    """The station's trace on a context of its own: computed once per process, shared by every test, never modified."""
    if station.name not in _FRESH:
        with hip.HipContext(0, storage=station.storage) as c:
            t = station.run(c)
        for v in t.values():
            v.setflags(write=False)
        _FRESH[station.name] = t
    return _FRESH[station.name]


def assert_as_fresh(station, t, where):
    """a carried context's trace against the fresh one's: the same bits, or (level search) the same names -- run() already held it to its model"""
    ref = fresh(station)
    if station.bitwise:
        msg = first_difference(t, ref)
        assert msg is None, f"{station.name} {where}: {msg}"
    else:
        assert list(t) == list(ref), f"{station.name} {where}"
        for k in t:
            if k.endswith(".exact"):
                assert np.array_equal(t[k], ref[k]), f"{station.name} {where}: {k}"


def set_columns(c, L):
    """fh_set_rhs on the dense operator the context holds.  A dense setter keeps the prox kind it finds (tests/golden/refusals: survive/...), and
    fh_set_rhs refuses a kind the multi-column form does not serve (LINF, L1BALL, TVBALL left by a station before): the station's own prox follows."""
    c.set_prox(hip.PROX_IDENTITY)
    c.set_rhs(L)


# ---- dense: the one-pass kernel, the device loop, the one-read set-up --------------------------------------------------------------------------
def _prox_of(c, kind):
    k, mu, lo, hi = RP.PROX[kind]
    c.set_prox(k, mu, lo, hi)


def _smallest(cases, key=lambda k: k.m * k.n):
    cases = list(cases)
    assert cases
    return min(cases, key=key)


def _several_teams(k):
    sh = FP.expected_shape(k)
    return (sh.TEAM >= 2 and sh.nteams >= 2 and len([r for r in FP.r_ends(sh, FP.round_up(k.m, 16)) if r]) >= 2
            and not FP.paths_of(sh, k.m, k.n)["idle members"])


ONEPASS = _smallest(k for k in FP.exact_step_cases() if k.storage == "f64" and 0 < k.cus <= 64 and k.mode == "accel" and _several_teams(k))
ONEPASS_F32 = _smallest(k for k in FP.exact_step_cases() if k.storage == "f32" and 0 < k.cus <= 64 and k.mode == "accel" and _several_teams(k))
SETUP = _smallest(k for k in FP.setup_cases() if k.storage == "f64" and FP.expected_shape(k).TEAM >= 2 and FP.expected_shape(k).nteams >= 2)
RUN = _smallest(k for k in RP.cases() if RP.expected_shape(k).G - RP.expected_shape(k).empty_wgs >= 2 and RP.launches_of(k) >= 2 and not k.ctl)


def _onepass(case, host_f32=False):
    def run(c, t):
        from tests import test_gpu_fused_paths as G
        st = FP.operands(case)
        c.set_matrix(st.A.astype(np.float32) if host_f32 else st.A)                # (-1, 0, 1: exact in float32; fh_set_matrix_f32 in float32 storage)
        c.set_loss_lsq(st.b)
        _prox_of(c, case.kind)
        G.check_geometry(c, case)
        G.enter(c, case, st)
        for k in range(2):                                                         # the other slot parity, the counters the first launch re-armed
            got = G.launch(c, case)
            G.assert_equals_model(got, case)
            t.home(f"launch{k}", {**got, "padding": [len(got["padding"])]})
        c.commit()
        t.read(c, "commit", ("X0", "G0"))
        t.put("plain", c.step(FP.TAU))                                            # (no model: the state after the commit; held against `fresh`)
        t.read(c, "plain", ("XHAT", "XPROX", "X1", "G1", "Z"))
        c.commit()
    return run


def _pinned_tuning(case):
    return FP.tuning_of(case)


def _run_loop(c, t):
    from tests import test_gpu_run_paths as G
    case = RUN
    A, x0, b, _ = RP.operands(case)
    c.set_matrix(A)
    c.set_loss_lsq(b)
    _prox_of(c, case.kind)
    c.set_vector(hip.VEC_X0, x0)
    assert c.run_shape() == RP.expected_shape(case) and c.run_supported() and c.cu_count()[0] >= 64
    o, st = RP.run_opts(case), G.start(c, case)
    h = c.run(RP.launches_of(case), o, st)
    assert st.stopped in (0, 1)
    out = G.collect(c, case, st, [list(r) for r in h])
    out["padding"] = all(G.padding_is_zero(c, RP.VECTORS[name], case.n) for name in ("X0", "G0", "XHAT", "G1", "BEST"))
    G.assert_equals_model(out, case)
    t.home("run", {k: v for k, v in out.items() if v is not None})


def _setup(c, t):
    from tests.test_gpu_run_paths import padding_is_zero
    case = SETUP
    o, mdl = FP.setup_operands(case), FP.setup_model(case)
    c.set_matrix(o.A)
    c.set_loss_lsq(o.b)
    _prox_of(c, case.kind)
    device_cus, used = c.cu_count()
    assert used == case.cus and c.setup_shape() == FP.expected_shape(case, device_cus)
    for rep in range(2):                                                           # (the body of test_the_one_read_set_up_is_exact_on_every_path)
        for which, v in ((hip.VEC_T0, o.t0), (hip.VEC_T1, o.t1), (hip.VEC_X0, o.x0), (hip.VEC_T2, np.ones(case.n)), (hip.VEC_G0, np.ones(case.n))):
            c.set_vector(which, v)
        s = c.setup()
        assert s[15] == 0.0
        for name, slot in (("FSQ", hip.S_FSQ), ("DX2", hip.S_DX2), ("DG2", hip.S_DG2), ("GSUM", hip.S_GSUM)):
            assert s[slot] == mdl[name], (rep, name, s[slot], mdl[name])
        g0, t2 = c.get_vector(hip.VEC_G0, case.n), c.get_vector(hip.VEC_T2, case.n)
        assert np.array_equal(g0, mdl["g0"]) and np.array_equal(t2, mdl["t2"])
        assert padding_is_zero(c, hip.VEC_G0, case.n, scratch=hip.VEC_T0) and padding_is_zero(c, hip.VEC_T2, case.n, scratch=hip.VEC_T0)
        t.home(f"setup{rep}", {"scalars": s, "g0": g0, "t2": t2})
    c.commit()
    z = c.get_vector(hip.VEC_Z, case.m)
    assert np.array_equal(z, mdl["z"])
    t.put("z", z)


# ---- dense and sparse: the K-fwd / K-adj pair in the vector and the multi-column form ----------------------------------------------------------
PAIR_TUNING, PAIR_KIND = next((tu, kind) for tu, kind in MC.vector_cases() if tu.get(hip.TUNE_ADJ_CPT) == 1 and kind == "shrink")
RHS4, RHS4_NT = next((k, nt) for k, nt in MC.group_cases() if k.L == 4 and k.name == "staged")
CSR_G, CSR_KIND = 16, "nonneg"
CSR_RHS = next(k for k in SL.step_cases() if k[1] == 4 and k[2] == 3)              # (G, LB, L, kind): three columns in rows of four doubles


def _sl_step(c, t, S, L, X0, B, tag, tau, coef, want, tol=None):
    """tests/test_gpu_sparse_lanes.py:run_step (init -> fwd -> adj -> fwd_adj -> adj(accel)) and its comparison, then the tail"""
    from tests.test_gpu_sparse_lanes import run_step
    got = run_step(c, S, L, X0, B, tag, tau, coef)
    if tol is None:
        assert_blocks(got, want, SL.MATRICES, SL.BLOCKS)
        assert np.array_equal(got["G1_pair"], want["G1"]) and np.array_equal(got["Z_pair"], want["Z"])
    else:
        assert_close_blocks(got, want, SL.MATRICES, SL.BLOCKS, SL.GROUP_TOL, SL.scalar_tol)
    assert np.array_equal(got["pair"][:hip.S_ALPHA], np.concatenate([got["fwd"][:hip.S_DXDG], got["adj"][hip.S_DXDG:hip.S_ALPHA]]))
    t.home("step", got)
    tail(c, t, tau, coef)
    if L or not hasattr(S, "indptr"):                                              # (the sparse vector form's padding is never written: csrc/fh_sparse.h)
        t.padding(c, "end", ("G0", "XHAT", "XPROX", "X1", "G1"))


def _dense_pair(c, t):
    m, n = MC.VECTOR_M, MC.VECTOR_N
    A, X0, B = MC.step_inputs(m, n, None)
    c.set_matrix(A)
    slab, cpt = PAIR_TUNING[hip.TUNE_ADJ_SLAB_ROWS], PAIR_TUNING[hip.TUNE_ADJ_CPT]
    assert -(-m // slab) >= 2 and m % slab and n > 2 * FP.FH_WG * cpt and c.rhs == 0     # two slabs, the last ragged; two column chunks of 256 lanes x cpt pairs
    _sl_step(c, t, A, None, X0, B, SL.prox_tag(PAIR_KIND), MC.TAU, MC.COEF, once("pair model", lambda: MC.step_model(m, n, None, PAIR_KIND)))


def _dense_rhs4(c, t):
    case = RHS4
    A, X0, B, tau, mu = once("rhs4 operands", lambda: SL.group_problem(MC.matrix(case.m, case.n), case.L))
    c.set_matrix(A)
    set_columns(c, case.L)
    sh = c.multi_shape()
    assert sh == MC.expected_shape(case, RHS4_NT) and sh.nslab >= 2 and sh.fwd_grid >= 2 and sh.ncc >= 2 and sh.stages >= 2
    tag = fa.GroupShrink(mu)
    want = once("rhs4 model", lambda: SL.exact_step(A, X0, B, tag, tau=tau, coef=0.37, dtype=np.longdouble))
    _sl_step(c, t, A, case.L, X0, B, tag, tau, 0.37, want, tol=True)


def _csr(G, LB, L, kind):
    def run(c, t):
        from tests.test_gpu_sparse_lanes import assert_lanes
        S = SL.exact_matrix(G, LB)
        if L:
            c.set_matrix_csr_rhs(S.indptr, S.indices, S.data, S.shape, L)
        else:
            c.set_matrix_csr(S.indptr, S.indices, S.data, S.shape)
        assert_lanes(c, S, SL.lb_of(L), G)
        assert min(c.sparse_lanes(0)[1], c.sparse_lanes(1)[1]) >= 2
        tag = SL.prox_tag(kind)
        X0, B = SL.step_operands(S, L)
        _sl_step(c, t, S, L, X0, B, tag, SL.TAU, SL.COEF, once(("csr model", G, LB, L, kind), lambda: SL.exact_step(S, X0, B, tag)))
    return run


SOFTMAX_L = 4


def _dense_softmax(c, t):
    """the step of tests/test_gpu_softmax.py:test_single_step_scalars_match_numpy, its operands by the same recipe (the softmax suite has no case
    module of step operands: its shapes put one workgroup on a launch) at the multi-column geometry of RHS4 (several slabs and chunks): the loss
    and the gradient against the host twin at the home test's tolerances (STEP_TOL, imported), everything against `fresh`"""
    case, L, tau = RHS4, SOFTMAX_L, 0.3
    rng = np.random.RandomState(13 + L)
    A = np.random.RandomState(14).randn(case.m, case.n) * 0.03
    X0, y = rng.randn(case.n, L) * 0.5, rng.randint(0, L, case.m)
    c.set_matrix(A)
    set_columns(c, L)
    sh = c.multi_shape()
    assert sh.nslab >= 2 and sh.fwd_grid >= 2 and sh.ncc >= 2
    sm = fa.SoftmaxLoss(y, classes=L)
    sm.bind(c)
    tag = fa.GroupShrink(0.05)
    c.set_prox(tag.kind, tag.mu, tag.lo, tag.hi)
    c.set_vector(hip.VEC_X0, X0)
    t.put("init", c.init())
    t.read(c, "init", ("G0",))
    Z0 = A @ X0
    from tests.test_gpu_softmax import STEP_TOL
    np.testing.assert_allclose(t["init.G0"].reshape(case.n, L), A.T @ sm.gradf(Z0), **STEP_TOL["G0"])
    np.testing.assert_allclose(t["init"][hip.S_FSQ], sm.f(Z0), **STEP_TOL["F0"])
    t.put("fwd", c.fwd(tau))
    t.read(c, "fwd", ("XHAT", "XPROX", "Z"))
    np.testing.assert_allclose(t["fwd.Z"].reshape(case.m, L), A @ t["fwd.XPROX"].reshape(case.n, L), **STEP_TOL["Z"])
    np.testing.assert_allclose(t["fwd"][hip.S_FSQ], sm.f(t["fwd.Z"].reshape(case.m, L)), **STEP_TOL["fwd scalars"])
    t.put("adj", c.adj(tau))
    t.read(c, "adj", ("G1",))
    np.testing.assert_allclose(t["adj.G1"].reshape(case.n, L), A.T @ sm.gradf(t["fwd.Z"].reshape(case.m, L)), **STEP_TOL["G1"])
    tail(c, t, tau, 0.37)
    t.padding(c, "end", ("G0", "XHAT", "XPROX", "X1", "G1"))


def _dense_generated(c, t):
    """fh_generate_matrix (no home case module holds a generated matrix: a ragged shape of several K-fwd workgroups and two column chunks, dyadic
    x0 and b): the matrix is read back, xhat is the exact elementwise expression of the device's g0, everything else is held against `fresh` alone"""
    m, n, tau = 203, 1030, 0.25
    c.generate_matrix(m, n, 0, 7, 0.5)
    A = c.get_matrix_rows(0, m)
    rng = np.random.RandomState(3)
    x0, b = rng.randint(-4, 5, n) * 0.5, rng.randint(-4, 5, m) * 0.5
    c.set_loss_lsq(b)
    c.set_prox(hip.PROX_SHRINK, 0.5)
    c.set_vector(hip.VEC_X0, x0)
    t.put("A", A)
    t.put("init", c.init())
    t.read(c, "init", ("G0",))
    t.put("fwd", c.fwd(tau))
    t.read(c, "fwd", ("XHAT", "XPROX", "Z"))
    assert np.array_equal(t["fwd.XHAT"], x0 - tau * t["init.G0"])
    t.put("adj", c.adj(tau))
    t.read(c, "adj", ("G1",))
    tail(c, t, tau, 0.5)


# ---- the stencils ------------------------------------------------------------------------------------------------------------------------------
def _stencil_plain(c, t):
    """tests/test_gpu_tv_paths.py: the plain pair and two one-pass launches back to back on 300 workgroups, no prox (exact)"""
    from tests import test_gpu_tv_paths as G
    g, prox = TV.GEOMETRY[TV.BACK_TO_BACK], TV.IDENTITY
    c.set_stencil(g.H, g.W)
    assert c.fused_supported() == 2 and TV.sweep_shape(g.H, g.W, g.rows)[0] * TV.sweep_shape(g.H, g.W, g.rows)[1] >= 2
    one, two = once("stencil plain model", lambda: TV.plain_twice(TV.reference_number(prox), g.H, g.W, prox))
    t.put("init", G.start(c, g.H, g.W, prox))
    t.put("fwd", c.fwd(0.125))
    t.put("adj", c.adj(0.125))
    m1 = dict(one, **{name: TV.as_image(one[name]) for name in ("xprox", "z", "x1")})
    G.assert_vector(c, hip.VEC_XPROX, m1["xprox"], "pair xprox")
    G.assert_vector(c, hip.VEC_Z, m1["z"], "pair z")
    G.assert_scalars(t["fwd"], m1, prox, ("S_FSQ", "S_DXG0", "S_DX2", "S_XH2", "S_G02", "S_RDOT"), "pair fwd")      # (as the home suite's two-launch test)
    G.assert_scalars(t["adj"], m1, prox, TV.ADJ_SCALARS, "pair adj")
    t.read(c, "pair", ("XPROX", "Z"))
    for k, m in enumerate((one, two)):
        scal = c.step(0.125)
        t.put(f"step{k}", scal)
        t.read(c, f"step{k}", ("XPROX", "Z"))
        G.assert_launch(c, scal, dict(m, **{name: TV.as_image(m[name]) for name in ("xprox", "z", "x1")}), prox, TV.STATE["plain"], f"step {k}")
        t.read(c, f"commit{k}", ("X0", "BEST"))


LAZY_STATE = "keeps"


def _stencil_lazy(c, t):
    """the accelerated one-pass sweep with the TV-ball prox from a lagged state (step_accel, commit, step_accel, commit): the context is LEFT with its
    iterate kept lazily and commits > 0.  The model's scalars at the home suite's summation bound; the bits against `fresh`."""
    from tests import test_gpu_tv_paths as G
    g, prox, state = TV.GEOMETRY[TV.BITS_GEOMETRY], TV.TVBALL, TV.STATE[LAZY_STATE]
    c.set_stencil(g.H, g.W)
    sh = TV.sweep_shape(g.H, g.W, g.rows)
    assert state.accel and state.lagged and sh[0] * sh[1] >= 2
    scal = G.one_pass(c, g.H, g.W, prox, state, "lazy")
    t.put("accel", scal)
    t.read(c, "accel", ("XPROX", "Z", "X1"))
    G.assert_launch(c, scal, once("stencil lazy model", lambda: TV.model(g.H, g.W, prox, state.name)), prox, state, "lazy")
    t.read(c, "commit", ("X0", "BEST", "XPROX"))


TV3D_INDEX = len(T3.ALL_SHAPES) - 1
assert T3.ALL_SHAPES[TV3D_INDEX] == T3.RAGGED


def _tv3d(c, t):
    from tests.test_gpu_tv3d import run_step
    shape, kind = T3.RAGGED, T3.PROX_KINDS[TV3D_INDEX % len(T3.PROX_KINDS)]
    c.set_stencil3d(*shape)
    sh = c.tv3d_shape()
    assert sh[:7] == hip.tv3d_shape(*shape, planes=T3.PLANES, ncu=c.cu_count()[0])[:7] and sh.chunks >= 2 and sh.tiles_h >= 2 and sh.tiles_w >= 2
    x0, b = T3.exact_operands(shape, 100 + TV3D_INDEX)
    ops = T3.FloatOps(np.float64)
    want_blocks, want_vec = once("tv3d model", lambda: T3.exact_step(x0, b, kind, ops))
    blocks, vec = run_step(c, shape, x0, b, T3.prox_args(kind), T3.TAU, T3.COEF)
    for name, v in want_vec.items():
        assert np.array_equal(vec[name], v), (name, kind)
    for call, block in want_blocks.items():
        want = T3.block_as_float(block, ops)
        assert np.array_equal(blocks[call][:15], want[:15]) and blocks[call][15] == 0.0, call
    t.home("step", {"blocks": blocks, "vec": vec})
    tail(c, t, T3.TAU, T3.COEF)


# ---- the operators that bring their own smooth term ------------------------------------------------------------------------------------------------
QUAD1 = next(k for k in QC.cases() if k.n == QC.N_WIDE and k.L == 1 and k.kind == "shrink")
QUAD2 = next((n, L, kind, nt) for n, L, kind, nt in QC.rownorm_cases() if n == QC.N_WIDE and L == 2 and kind == "rowball")
QUAD2_CASE = QC.Case(QUAD2[0], QC.lb_of(QUAD2[1]), QUAD2[1], QC.uneven_cap(QC.round_up(QUAD2[0], 16) // QC.MC_FOR_EACH[QC.lb_of(QUAD2[1])][1]), QUAD2[3], QUAD2[2])
FACTOR = next(k for k in FC.cases() if k.K == 2 and k.nt == 0 and k.kind == "box")


def _quad_tail(c, t, n, L, tau, coef):
    tail(c, t, tau, coef, names=N_SIDE)
    t.padding(c, "end", ("G0", "XHAT", "XPROX", "X1", "G1"))


def _quad1(c, t):
    from tests import test_gpu_quad as G
    case = QUAD1
    Q, cvec, X0 = QC.exact_inputs(case.n, case.L)
    c.set_quadratic(Q, cvec, case.L)
    sh = G.assert_shape(c, case)
    assert sh.ntrip >= 2 or sh.pass_max >= 2
    got = G.run_step(c, case.n, case.L, X0, QC.prox_tag(case.kind), QC.TAU, QC.COEF)
    assert_blocks(got, once("quad1 model", lambda: QC.exact_model(case.n, case.L, case.kind)), QC.MATRICES, QC.BLOCKS)
    t.home("step", got)
    _quad_tail(c, t, case.n, case.L, QC.TAU, QC.COEF)


def _quad2(c, t):
    from tests import test_gpu_quad as G
    n, L, kind, nt = QUAD2
    Q, cvec, X0, tau, tag = once("quad2 operands", lambda: QC.rownorm_problem(n, L, kind))
    case = QUAD2_CASE                                                              # (as tests/test_gpu_quad.py builds the wide row-norm cases)
    c.set_quadratic(Q, cvec, L)
    assert c.quad_shape() == QC.expected_shape(case) and c.rhs == L
    def model():
        terms = {}
        return QC.model_step(Q, cvec, X0, tag, tau=tau, coef=QC.COEF, dtype=np.longdouble, terms=terms), terms
    want, terms = once("quad2 model", model)
    got = G.run_step(c, n, L, X0, tag, tau, QC.COEF)
    G.assert_rownorm_step(got, want, terms, n, L, kind, tag)                       # (the home suite's own comparison)
    t.home("step", got)
    _quad_tail(c, t, n, L, tau, QC.COEF)


def _factor(c, t):
    from tests import test_gpu_factor as G
    case = FACTOR
    m, n, K = case.m, case.n, case.K
    S, Z0, G0 = FC.exact_inputs(m, n, K)
    c.set_factorization(S, K)
    sh = G.assert_shape(c, case)
    assert sh.row_panels >= 2 and c.shape() == (m + n, m + n) and c.rhs == K
    got = G.run_step(c, m, n, K, Z0, G0, FC.top_tag(case.kind), FC.BOTTOM, FC.TAU, FC.COEF)          # (the split prox: fh_set_prox_split)
    assert_blocks(got, once("factor model", lambda: FC.exact_model(m, n, K, case.kind)), FC.MATRICES, FC.BLOCKS)
    t.home("step", got)
    _quad_tail(c, t, m + n, K, FC.TAU, FC.COEF)


# ---- the transforms and the convolution -------------------------------------------------------------------------------------------------------------
DCT_N, DCT_CAP = next((N, cap) for N, cap in D1.SIZES if cap and N == 1000)      # two levels under the row cap: five launches per transform
DCT2_SHAPE = (45, 96)
assert DCT2_SHAPE in D2.SIZES
CONV = max(CV.SHAPES, key=lambda k: int(np.prod(k[0])))


def _transform_step(c, t, n, x0, b, tau, check_z):
    """init -> fwd -> adj -> tail with the shrink prox; xhat and xprox are elementwise (exact given g0), z by the home suite's bound"""
    c.set_loss_lsq(b)
    tag = fa.Shrink(0.3)
    c.set_prox(tag.kind, tag.mu, tag.lo, tag.hi)
    c.set_vector(hip.VEC_X0, x0)
    t.put("init", c.init())
    t.read(c, "init", ("G0",))
    t.put("fwd", c.fwd(tau))
    t.read(c, "fwd", ("XHAT", "XPROX", "Z"))
    xh = x0 - tau * t["init.G0"]
    assert np.array_equal(t["fwd.XHAT"], xh) and np.array_equal(t["fwd.XPROX"], np.asarray(tag.prox(xh, tau)))
    check_z(t["fwd.Z"], t["fwd.XPROX"])
    assert t["fwd"][hip.S_GMAX] == np.abs(t["fwd.XPROX"]).max() and t["fwd"][15] == 0.0
    t.put("adj", c.adj(tau))
    t.read(c, "adj", ("G1",))
    tail(c, t, tau, 0.5)


def _dct(c, t):
    from tests.test_gpu_dct import assert_transform
    N = DCT_N
    c.set_tuning(hip.TUNE_DCT_ROW_CAP, DCT_CAP)
    x, y, mask = D1.operands(N, N)
    c.set_dct(N, mask)
    sh = c.dct_shape()
    assert sh == hip.dct_shape(N, DCT_CAP, ncu=c.cu_count()[0]) and sh.levels == 2 and sh.launches == 5 and sh.N1 * sh.N2 == N
    _transform_step(c, t, N, x * 1.5, mask * y, 0.9, lambda z, xp: assert_transform(z, xp, mask, False, "z"))


def _dct2(c, t):
    from tests.test_gpu_dct2 import assert_transform
    shape = DCT2_SHAPE
    x, y, mask = D2.operands(shape, 7)
    c.set_dct2(*shape, mask)
    assert c.dct2_shape() == hip.dct2_shape(*shape, ncu=c.cu_count()[0])
    n = shape[0] * shape[1]
    _transform_step(c, t, n, x.ravel() * 1.5, (mask * y).ravel(), 0.9,
                    lambda z, xp: assert_transform(z.reshape(shape), xp.reshape(shape), mask, False, "z"))


def _conv(c, t):
    """the body of tests/test_gpu_conv.py:test_one_exact_step_every_vector_and_every_scalar on the largest of its shapes"""
    case = CONV
    shape, kshape, origin, masked = case
    i = CV.SHAPES.index(case)
    n, kind = int(np.prod(shape)), CV.PROX_KINDS[i % len(CV.PROX_KINDS)]
    x0, b, K, o2, mask = once("conv operands", lambda: CV.exact_operands(case, 500 + i))
    ops = CV.IntOps()
    blocks, vec = once("conv model", lambda: CV.exact_step(x0, b, K, o2, mask, kind, ops))
    H, W = CV.shape2d(shape)
    c.set_conv2d((H, W), np.reshape(K, CV.shape2d(kshape)), origin=o2, diag=None if mask is None else np.reshape(mask, (H, W)))
    sh = c.conv_shape()
    assert sh == hip.conv_shape(H, W, *CV.shape2d(kshape), ncu=c.cu_count()[0]) and sh.grid >= 2
    c.set_loss_lsq(b.ravel())
    c.set_prox(*CV.prox_args(kind))
    c.set_vector(hip.VEC_X0, x0.ravel())
    got = {"init": c.init()}
    dev = {"g0": c.get_vector(hip.VEC_G0, n)}
    got["fwd"] = c.fwd(CV.TAU)
    dev.update(xhat=c.get_vector(hip.VEC_XHAT, n), xprox=c.get_vector(hip.VEC_XPROX, n), z=c.get_vector(hip.VEC_Z, n))
    got["adj"] = c.adj(CV.TAU)
    dev["g1"] = c.get_vector(hip.VEC_G1, n)
    got["fwd_adj"] = c.fwd_adj(CV.TAU)
    got["adj_accel"] = c.adj(CV.TAU, accel=True, coef=CV.COEF)
    dev.update(x1=c.get_vector(hip.VEC_X1, n), g1_accel=c.get_vector(hip.VEC_G1, n))
    for name, v in vec.items():
        assert np.array_equal(dev[name], v.ravel() / ops.unit), name
    for call in ("init", "fwd", "adj", "fwd_adj", "adj_accel"):
        want = CV.block_as_float(blocks[call], ops)
        assert np.array_equal(got[call][:15], want[:15]) and got[call][15] == 0.0, call
    t.home("step", {"blocks": got, "vec": dev})
    tail(c, t, CV.TAU, CV.COEF)


# ---- the identity operator: the nuclear prox, weights and the nuclear ball ------------------------------------------------------------------------------
ID_SHAPE = CC.STEP_SHAPES[-1]                                                      # 33 x 130: several column chunks, a ragged last one


def _identity(kind, loss, weighted):
    def run(c, t):
        from tests import test_gpu_completion as G
        X0, B, W = CC.step_problem(*ID_SHAPE)
        if loss == "logistic":
            B = G.labels_of(B)
        if not weighted:
            W = None
        c.set_identity(*ID_SHAPE)
        (c.set_loss_lsq if loss == "lsq" else c.set_loss_logistic)(B)
        if weighted:
            c.set_loss_weights(W)
        G.bind(c, G.TAGS[kind])
        sh = c.nuclear_shape()
        assert sh._asdict() == NC.shape_of(*ID_SHAPE) and sh.wgs_per_step >= 2
        t.home("step", G.one_step(c, ID_SHAPE, loss, B, W, X0, G.TAGS[kind]))          # (checks every vector and scalar against NumPy / LAPACK itself)
        t.put("info", list(c.nuclear_info()))
        if weighted:
            c.set_loss_weights(None)                                                   # every other setter refuses a context that holds weights
            t.put("unweighted", c.init())
            t.read(c, "unweighted", ("G0",))
    return run


# ---- the level search: the l1 ball ----------------------------------------------------------------------------------------------------------------
L1_DENSE_N = 20001
assert 16384 < L1_DENSE_N <= 262144


def _l1ball(c, t, n, x0, g0, tau, several, check_z=None):
    """One forward launch as the home suites hold the level search (tests/test_gpu_dct.py:test_one_forward_launch_per_prox_kind): xhat bit for bit,
    xprox against the sort-based projection at the home tolerance.  The search starts from the level the context last held."""
    from tests.test_gpu_dct import LEVEL_RTOL, level_atol
    xh = x0 - tau * g0
    tag = fa.L1Ball(0.3 * float(np.abs(xh).sum()))
    c.set_prox(tag.kind, tag.mu, tag.lo, tag.hi)
    c.set_vector(hip.VEC_X0, x0)
    t.put("init.exact", c.init()[:hip.S_GSUM])                                     # (x0 and b are the same on both sides: the same sums, the same order)
    c.set_vector(hip.VEC_G0, g0)
    before = [c.recovered_count(k) for k in (hip.RECOVERED_LEVEL_FALLBACK, hip.RECOVERED_LEVEL_FAILED)]
    s = c.fwd(tau)
    got_h, got_p = c.get_vector(hip.VEC_XHAT, n), c.get_vector(hip.VEC_XPROX, n)
    assert np.array_equal(got_h, xh)
    np.testing.assert_allclose(got_p, fo.project_l1(xh, tag.mu), rtol=LEVEL_RTOL, atol=level_atol(n, xh))
    assert s[hip.S_GMAX] == np.abs(got_p).max() and s[15] == 0.0 and several
    assert before == [c.recovered_count(k) for k in (hip.RECOVERED_LEVEL_FALLBACK, hip.RECOVERED_LEVEL_FAILED)]
    t.put("xhat.exact", got_h)
    t.put("g02.exact", [s[hip.S_G02]])                                             # (the one forward sum that does not pass through the level)
    t.put("fwd", s)
    t.put("xprox", got_p)
    t.read(c, "fwd", ("Z",))
    if check_z is not None:
        check_z(t["fwd.Z"], got_p)
    t.put("adj", c.adj(tau))
    t.read(c, "adj", ("G1", "X1"))
    assert np.array_equal(t["adj.X1"], got_p) and np.array_equal(t["adj"][:hip.S_DXDG], s[:hip.S_DXDG])
    t.padding(c, "end", ("XHAT", "XPROX", "X1", "G1"))
    c.commit()
    t.read(c, "commit", ("X0",))
    assert np.array_equal(t["commit.X0"], got_p)


def _l1_dense(c, t):
    n, m = L1_DENSE_N, 8
    A = FP.matrix(m, n, 4)
    rng = np.random.RandomState(300 + n)
    c.set_matrix(A)
    c.set_loss_lsq(np.zeros(m))
    _l1ball(c, t, n, rng.randn(n) * 1.5, rng.randn(n), 0.9, several=n > 16384)


def _l1_dct(c, t):
    N = 4096
    assert (N, 0) in D1.SIZES
    rng = np.random.RandomState(300 + N)
    from tests.test_gpu_dct import assert_transform
    mask = D1.operands(N, N)[2]
    c.set_dct(N, mask)
    c.set_loss_lsq(np.zeros(N))
    _l1ball(c, t, N, rng.randn(N) * 1.5, rng.randn(N), 0.9, several=c.dct_shape().launches >= 1,
            check_z=lambda z, xp: assert_transform(z, xp, mask, False, "z"))


def _l1_conv(c, t):
    shape, kshape, origin, masked = CONV
    H, W = CV.shape2d(shape)
    n = H * W
    rng = np.random.RandomState(300 + CV.SHAPES.index(CONV))
    Kt, o2 = rng.randn(*CV.shape2d(kshape)), CV.origin2d(kshape, origin)
    c.set_conv2d((H, W), Kt, origin=o2)
    c.set_loss_lsq(np.zeros(n))
    _l1ball(c, t, n, rng.randn(n) * 1.5, rng.randn(n), 0.9, several=c.conv_shape().grid >= 2,
            check_z=lambda z, xp: np.testing.assert_array_equal(z, CV.conv(xp.reshape(H, W), Kt, o2, None).ravel()))      # (as tests/test_gpu_conv.py: bit for bit)


# ---- the duality gap ----------------------------------------------------------------------------------------------------------------------------------
GAP_SHAPE = (1000, 1000, 1)
assert GAP_SHAPE in GC.SHAPES


def _gap(c, t):
    """tests/test_gpu_gap.py:test_least_squares_on_dyadic_data_gives_the_host_record_bit_for_bit on one dense shape of two slabs a side"""
    m, n, L = GAP_SHAPE
    A, b, x = once("gap operands", lambda: GC.dyadic_problem(m, n, L, seed=m + 3 * n + L))
    assert -(-n // FP.FH_WG) >= 2 and -(-m // FP.FH_WG) >= 2                      # csrc/fasta_hip.hip:gap_slabs: a slab of partials per 256 rows
    c.set_matrix(A)
    loss = fa.LeastSquares(b)
    loss.bind(c)
    for k, mu in enumerate((1.0, 0.25)):
        reg = fa.Shrink(mu)
        c.set_prox(reg.kind, reg.mu, 0.0, 0.0)
        c.set_vector(hip.VEC_X0, x)
        t.put(f"init{k}", c.init())
        got = c.dual_gap()
        assert tuple(got) == tuple(ce.duality_gap(A, loss, reg, x)) and got == c.dual_gap()
        t.put(f"gap{k}", tuple(got))
    t.put("fwd", c.fwd(0.25))
    t.put("adj", c.adj(0.25))
    c.commit()
    t.put("gap after a plain step", tuple(c.dual_gap()))
    t.read(c, "end", ("X0", "G0"))


# ---- the list -----------------------------------------------------------------------------------------------------------------------------------------
STATIONS = (
    Station("dense one-pass", "dense", FP, _onepass(ONEPASS), _pinned_tuning(ONEPASS), tau=FP.TAU, dense=True),
    Station("dense pair", "dense", MC, _dense_pair, PAIR_TUNING, tau=MC.TAU, dense=True),
    Station("dense rhs4 group", "dense_rhs2", MC, _dense_rhs4, MC.tuning_of(RHS4, RHS4_NT), exact=False, tau=0.25),
    Station("dense softmax", "dense_rhs2", SM, _dense_softmax, MC.tuning_of(RHS4, RHS4_NT), exact=False, tau=0.3),
    Station("dense generated", "dense_generated", MC, _dense_generated, exact=False, tau=0.25, dense=True),
    Station("dense fh_run", "dense", RP, _run_loop, RP.tuning_of(RUN), dense=True),
    Station("dense fh_setup", "dense", FP, _setup, _pinned_tuning(SETUP), dense=True),
    Station("csr", "csr", SL, _csr(CSR_G, 0, None, CSR_KIND), tau=SL.TAU),
    Station("csr rhs", "csr_rhs2", SL, _csr(*CSR_RHS), tau=SL.TAU),
    Station("stencil plain", "stencil", TV, _stencil_plain, {hip.TUNE_TV_ROWS: TV.GEOMETRY[TV.BACK_TO_BACK].rows, hip.TUNE_TV_U: 2, hip.TUNE_TV_PIPE: 1}, tau=0.125),
    Station("stencil lazy", "stencil", TV, _stencil_lazy, {hip.TUNE_TV_ROWS: TV.GEOMETRY[TV.BITS_GEOMETRY].rows, hip.TUNE_TV_U: 2, hip.TUNE_TV_PIPE: 1},
            exact=False, leaves_lazy=True, tau=0.0625),
    Station("stencil 3-D", "stencil3d", T3, _tv3d, {hip.TUNE_TV3_PLANES: T3.PLANES}, tau=T3.TAU),
    Station("quadratic L1", "quad1", QC, _quad1, QC.tuning_of(QUAD1), tau=QC.TAU),
    Station("quadratic L2 rowball", "quad2", QC, _quad2, QC.tuning_of(QUAD2_CASE), exact=False, tau=0.25),
    Station("factorisation split", "factor", FC, _factor, FC.tuning_of(FACTOR), tau=FC.TAU),
    Station("dct two-level", "dct", D1, _dct, {hip.TUNE_DCT_ROW_CAP: DCT_CAP}, exact=False, tau=0.9),
    Station("dct 2-D", "dct2", D2, _dct2, exact=False, tau=0.9),
    Station("convolution", "conv", CV, _conv, tau=CV.TAU),
    Station("identity nuclear", "identity", NC, _identity("nuclear", "lsq", False), exact=False, tau=0.25),
    Station("identity weights nucball", "identity", CC, _identity("nucball", "logistic", True), exact=False, tau=0.25),
    Station("l1 ball dense", "dense", D1, _l1_dense, bitwise=False, exact=False, tau=0.9, dense=True),
    Station("l1 ball dct", "dct", D1, _l1_dct, bitwise=False, exact=False, tau=0.9),
    Station("l1 ball conv", "conv", CV, _l1_conv, bitwise=False, exact=False, tau=0.9),
    Station("duality gap", "dense", GC, _gap, tau=0.25, dense=True),
)
# float32 storage: the setters tests/golden/refusals/c_abi.json records as accepted in state "f32" (read, not listed: F32_SETTERS)
F32_STATIONS = (
    Station("f32 dense one-pass", "dense", FP, _onepass(ONEPASS_F32), _pinned_tuning(ONEPASS_F32), storage="f32", tau=FP.TAU, dense=True),
    Station("f32 dense from float32", "dense_f32_host", FP, _onepass(ONEPASS_F32, host_f32=True), _pinned_tuning(ONEPASS_F32), storage="f32", tau=FP.TAU, dense=True),
    Station("f32 dense generated", "dense_generated", MC, _dense_generated, exact=False, storage="f32", tau=0.25, dense=True),
    Station("f32 stencil plain", "stencil", TV, _stencil_plain, {hip.TUNE_TV_ROWS: TV.GEOMETRY[TV.BACK_TO_BACK].rows, hip.TUNE_TV_U: 2, hip.TUNE_TV_PIPE: 1},
            storage="f32", tau=0.125),
    Station("f32 stencil 3-D", "stencil3d", T3, _tv3d, {hip.TUNE_TV3_PLANES: T3.PLANES}, storage="f32", tau=T3.TAU),
)
BY_NAME = {s.name: s for s in STATIONS + F32_STATIONS}
assert len(BY_NAME) == len(STATIONS) + len(F32_STATIONS)


def f32_setters():
    """the entries of refusal_cases.SETTERS every call of which the fixture records as accepted on a float32-storage context"""
    with open(RC.GOLDEN) as f:
        cases = json.load(f)["cases"]
    return sorted(name for name in RC.SETTERS if all(status == 0 for status, _ in cases[f"state/f32/{name}"]["got"]))


# ---- the transition plan --------------------------------------------------------------------------------------------------------------------------------
def plan(stations, predecessor):
    """The programs one test runs on one context: P, s1, P, s2, ... through every other station -- every ordered pair (P, s) and (s, P)."""
    out = []
    for s in stations:
        if s is not predecessor:
            out += [predecessor, s]
    return out + [predecessor]


def pairs_of(stations):
    """every ordered pair of distinct stations the plans of all predecessors run back to back"""
    seen = set()
    for p in stations:
        seq = plan(stations, p)
        seen |= {(a.name, b.name) for a, b in zip(seq, seq[1:])}
    return seen


def long_chain(stations, seed=20, factor=3):
    """a fixed-seed order of `factor` times the number of stations: `factor` shuffles of the list, no station twice in a row"""
    rng, out = np.random.RandomState(seed), []
    for _ in range(factor):
        order = [stations[k] for k in rng.permutation(len(stations))]
        if out and order[0] is out[-1]:
            order.append(order.pop(0))
        out += order
    return out


# ---- how a predecessor is left ---------------------------------------------------------------------------------------------------------------------------
def leave_committed(c, p):
    pass                                                                           # every program ends with fh_commit (the lazy station: lazy, commits > 0)


def leave_mid_attempt(c, p):
    if p.leaves_lazy:
        return                                                                     # (lazy: fh_fwd is refused until the next fh_init; it IS a leaving state)
    c.fwd(p.tau)                                                                   # fwd done, adj not


def leave_accelerated(c, p):
    if p.setter == "stencil" or p.leaves_lazy:
        return                                                                     # (its accelerated attempt is the lazy station's program)
    c.fwd(p.tau)
    c.adj(p.tau, True, 0.5)                                                        # last_accel set, not committed


LEAVINGS = {"after commit": leave_committed, "mid-attempt": leave_mid_attempt, "after an accelerated attempt": leave_accelerated}
# the successors the leaving states are run into at least: a dense, a stencil and an identity station
LEAVING_SUCCESSORS = ("dense pair", "dense one-pass", "stencil plain", "identity nuclear", "duality gap")
# fh_run ends its program inside the device loop's own state and the level-search / gap stations hold no step size worth a further attempt
LEAVING_PREDECESSORS = tuple(s.name for s in STATIONS if s.name not in ("dense fh_run", "dense fh_setup", "duality gap") and s.bitwise)

# setters the library refuses, with arguments from the home modules' REFUSED lists (every argument refusal stands before set_begin: the context
# keeps the operator it held)
REFUSED_SETTERS = {
    "a DCT length with a prime factor above 5": lambda c: c.set_dct(D1.REFUSED[0]),
    "a 2-D DCT axis with a prime factor above 5": lambda c: c.set_dct2(*D2.REFUSED[0][0]),
    "a convolution origin outside its kernel": lambda c: c.set_conv2d((8, 8), np.ones((2, 2)), origin=(2, 0)),
}


# ---- the prox kind a setter finds ------------------------------------------------------------------------------------------------------------------------
# P leaves the context on a kind the next form does not serve; the next operator is set and run WITHOUT any fh_set_prox: set_begin's
# reset_unserved must have brought the kind back to IDENTITY, which is what a fresh context holds.
UNSERVED_LEAVERS = ("dense rhs4 group", "stencil lazy", "quadratic L2 rowball", "factorisation split", "identity nuclear", "identity weights nucball")
BARE_DCT_N = 96
BARE_TV3D = (3, 4, 5)
BARE_CONV = next(k for k in CV.SHAPES if k[0] == (7, 9) and not k[3])
assert (BARE_DCT_N, 0) in D1.SIZES and BARE_TV3D in T3.SHAPES


def _bare_dct(c):
    x, y, mask = D1.operands(BARE_DCT_N, 5)
    c.set_dct(BARE_DCT_N, mask)
    return x, mask * y


def _bare_conv(c):
    x0, b, K, o2, mask = CV.exact_operands(BARE_CONV, 1)
    c.set_conv2d(CV.shape2d(BARE_CONV[0]), np.reshape(K, CV.shape2d(BARE_CONV[1])), origin=o2)
    return x0.ravel(), b.ravel()


def _bare_tv3d(c):
    x0, b = T3.exact_operands(BARE_TV3D, 3)
    c.set_stencil3d(*BARE_TV3D)
    return x0, b


def _bare_csr(c):
    S = SL.exact_matrix(4, 0)
    c.set_matrix_csr(S.indptr, S.indices, S.data, S.shape)
    return SL.step_operands(S, None)


BARE = {"dct": _bare_dct, "convolution": _bare_conv, "stencil 3-D": _bare_tv3d, "csr": _bare_csr}


# ... but a kind the next form DOES serve is kept, as every setter keeps it (tests/golden/refusals: survive/...): the TV ball on the 3-D stencil
KEPT_KINDS = {("stencil lazy", "stencil 3-D"): hip.PROX_TVBALL}


def bare_program(c, which, tau=0.5, identity=True):
    """the operator, the loss, x0 -- and no prox call: init, fwd, adj, commit, everything read"""
    t = Trace()
    write_tuning(c, {})
    x0, b = BARE[which](c)
    c.set_loss_lsq(b)
    c.set_vector(hip.VEC_X0, x0)
    t.put("init", c.init())
    t.read(c, "init", ("G0",))
    t.put("fwd", c.fwd(tau))
    t.read(c, "fwd", ("XHAT", "XPROX", "Z"))
    assert np.array_equal(t["fwd.XPROX"], t["fwd.XHAT"]) == identity               # no prox: the identity
    t.put("adj", c.adj(tau))
    t.read(c, "adj", ("G1", "X1"))
    c.commit()
    t.read(c, "commit", ("X0", "G0"))
    return t
