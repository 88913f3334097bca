"""GPU tests of ONE context carried through every operator form (the stations of tests/carry_cases.py), bit for bit.

The other GPU suites test each kernel family on fresh contexts, one form per context.  A context is long-lived in real use -- every *Map keeps
one across fasta() calls, regpath.path warm-starts a grid on one, proximal.device_prox switches prox kinds on cached scratch contexts -- and an
operator setter does not reset what the forms share: the arrival counters, the scalar block with the warm-start level of the level search,
every FH_TUNE_* value and, through the dense setters, the solver flags.  Here every ordered pair of stations runs back
to back on one context, a predecessor is left in each state a solve can be abandoned in, a refused setter stands between two stations, one
form changes its geometry, and one long chain runs them all; every program's scalars, vectors and padding are compared with the home suite's
model by the home suite's comparison and with the same program on a fresh context, `==`."""
import numpy as np
import pytest

from fasta_python_amd import hip
from tests import carry_cases as K
from tests import fused_paths as FP
from tests import mc_paths as MC

pytestmark = pytest.mark.gpu
IDS = lambda v: v.name.replace(" ", "_") if isinstance(v, K.Station) else str(v).replace(" ", "_")


def carry(c, stations, what):
    for k, s in enumerate(stations):
        K.assert_as_fresh(s, s.run(c), f"({what}, program {k} of {[x.name for x in stations]})")


# ---- every ordered pair ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", K.STATIONS, ids=IDS)
def test_every_station_after_and_before_this_one(p):
    """P, s1, P, s2, ..., P on one context: every pair (P, s) and (s, P); the second and later runs of P are compared as the first."""
    with hip.HipContext(0) as c:
        carry(c, K.plan(K.STATIONS, p), f"predecessor {p.name}")


@pytest.mark.parametrize("p", K.F32_STATIONS, ids=IDS)
def test_every_float32_storage_station_after_and_before_this_one(p):
    """the same plan over the setters the refusal fixture records as accepted on a float32-storage context"""
    assert sorted({s.setter for s in K.F32_STATIONS}) == K.f32_setters()
    with hip.HipContext(0, storage="f32") as c:
        carry(c, K.plan(K.F32_STATIONS, p), f"float32 storage, predecessor {p.name}")


def test_one_long_chain():
    """a fixed-seed order of three times the number of stations on one context: accumulation that pairs cannot show"""
    with hip.HipContext(0) as c:
        carry(c, K.long_chain(K.STATIONS), "long chain")


# ---- how the predecessor was left, and what a dense setter keeps of it -------------------------------------------------------------------------------
COLD_M, COLD_N = 40, 600


def cold_probe(c):
    """A dense operator set on whatever the context was, then every call a caller may make BEFORE fh_set_vector(X0) / fh_init: the answers --
    values, or the status and text of the refusal -- in order.  What the dense setters keep (lazy, last_accel, commits, at_state, loss_kind)
    must not show in any of them."""
    A, X0, B = MC.step_inputs(COLD_M, COLD_N, None)
    out = []

    def ask(name, fn):
        try:
            v = fn()
            out.append((name, np.array(v, dtype=np.float64) if not isinstance(v, tuple) else np.array(tuple(v))))
        except hip.HipError as exc:
            out.append((name, str(exc)))

    K.write_tuning(c, {})
    c.set_matrix(A)
    for v in ("X0", "XPROX", "X1", "BEST", "G0", "Z"):                              # (lazy kept: the c->lazy branches of fh_get_vector)
        ask(f"get {v} before the loss", lambda: c.get_vector(K.VEC[v], COLD_M if v == "Z" else COLD_N))
    ask("gap before the loss", c.dual_gap)                                          # (at_state kept; loss_kind kept with has_b false)
    ask("init before the loss", c.init)
    ask("fwd before the loss", lambda: c.fwd(0.5))
    c.set_loss_lsq(B)
    c.set_prox(hip.PROX_SHRINK, 1.0)
    ask("gap before init", c.dual_gap)
    ask("fwd before init", lambda: c.fwd(0.5))                                      # x0 = g0 = 0 on a fresh context: a launch, not a refusal
    ask("commit after fwd alone", lambda: (c.commit(), c.get_vector(hip.VEC_X0, COLD_N))[1])      # (last_accel kept: fh_commit branches on it)
    ask("X1 after that commit", lambda: c.get_vector(hip.VEC_X1, COLD_N))
    ask("fwd after that commit", lambda: c.fwd(0.5))
    ask("adj before init", lambda: c.adj(0.5))
    ask("step before init", lambda: c.step(0.5))
    for v in ("X0", "XPROX", "X1", "Z"):
        ask(f"get {v} before init", lambda: c.get_vector(K.VEC[v], COLD_M if v == "Z" else COLD_N))
    c.set_vector(hip.VEC_X0, X0)
    ask("init", c.init)
    ask("gap", c.dual_gap)
    ask("fwd", lambda: c.fwd(0.5))
    return out


_COLD = []


def assert_cold_probe_as_fresh(c, where):
    if not _COLD:
        with hip.HipContext(0) as f:
            _COLD.append(cold_probe(f))
    got, want = cold_probe(c), _COLD[0]
    assert [n for n, _ in got] == [n for n, _ in want]
    for (name, g), (_, w) in zip(got, want):
        same = (isinstance(g, str) and isinstance(w, str) and g == w) if isinstance(g, str) or isinstance(w, str) else np.array_equal(g, w, equal_nan=True)
        assert same, f"{where}: '{name}' answers {g!r} on the carried context, {w!r} on a fresh one"


def successors():
    return [K.BY_NAME[n] for n in K.LEAVING_SUCCESSORS]


@pytest.mark.parametrize("leaving", list(K.LEAVINGS), ids=IDS)
@pytest.mark.parametrize("p", [K.BY_NAME[n] for n in K.LEAVING_PREDECESSORS], ids=IDS)
def test_a_predecessor_left_in_every_state(p, leaving):
    """P is run and left -- after its commit, mid-attempt (fwd done, adj not), after an accelerated attempt that is not committed -- then a dense
    operator is set and asked everything before its first fh_init (the three leads: lazy, at_state, loss_kind), then a dense, a stencil and an
    identity station run; all answers are a fresh context's."""
    with hip.HipContext(0) as c:
        for s in [None] + successors():
            if s is p:
                continue
            K.assert_as_fresh(p, p.run(c), f"before '{leaving}'")
            K.LEAVINGS[leaving](c, p)
            if s is None:
                assert_cold_probe_as_fresh(c, f"{p.name} left {leaving}")
            else:
                K.assert_as_fresh(s, s.run(c), f"after {p.name} left {leaving}")


def test_observation_weights_removed_again():
    """weights set, a step, weights removed: the next dense, stencil and identity stations (and the cold dense probe) answer as on a fresh context"""
    p = K.BY_NAME["identity weights nucball"]
    with hip.HipContext(0) as c:
        for s in [None] + successors():
            K.assert_as_fresh(p, p.run(c), "weights")
            if s is None:
                assert_cold_probe_as_fresh(c, "weights removed")
            else:
                K.assert_as_fresh(s, s.run(c), "after the weights were removed")


def test_the_lazy_stencil_iterate_does_not_outlive_its_operator():
    """The narrowest form of what the chains above found: after an accelerated one-pass stencil solve the iterate is kept lazily; a dense setter
    kept the flag, and fh_fwd / fh_step on the NEW operator before its first fh_init were refused in the stencil's words, where a fresh context
    launches on x0 = 0."""
    p = K.BY_NAME["stencil lazy"]
    A, X0, B = MC.step_inputs(COLD_M, COLD_N, None)
    with hip.HipContext(0) as c, hip.HipContext(0) as f:
        p.run(c)
        for ctx in (c, f):
            K.write_tuning(ctx, {})
            ctx.set_matrix(A)
            ctx.set_loss_lsq(B)
            ctx.set_prox(hip.PROX_SHRINK, 1.0)
        assert np.array_equal(c.get_vector(hip.VEC_X0, COLD_N), f.get_vector(hip.VEC_X0, COLD_N))
        assert np.array_equal(c.fwd(0.5), f.fwd(0.5)) and np.array_equal(c.adj(0.5), f.adj(0.5))
        assert np.array_equal(c.get_vector(hip.VEC_G1, COLD_N), f.get_vector(hip.VEC_G1, COLD_N))


_BARE = {}


@pytest.mark.parametrize("name", K.UNSERVED_LEAVERS, ids=IDS)
def test_a_prox_kind_the_next_form_does_not_serve_is_dropped_by_its_setter(name):
    """P ends on GROUP, TVBALL, ROWBALL, ROWSPLIT, NUCLEAR or NUCBALL; a DCT, a convolution, a 3-D stencil and a CSR operator are then set and run
    with NO prox call: every scalar and vector is what a fresh context (IDENTITY) gives -- not a launch refused for a kind the form does not serve."""
    p = K.BY_NAME[name]
    with hip.HipContext(0) as c:
        for which in K.BARE:
            kept = K.KEPT_KINDS.get((name, which))
            if (which, kept) not in _BARE:
                with hip.HipContext(0) as f:
                    if kept is not None:
                        f.set_prox(kept)                                            # (an empty context may hold it for the operator to come)
                    _BARE[(which, kept)] = K.bare_program(f, which, identity=kept is None)
            K.assert_as_fresh(p, p.run(c), f"before a bare {which}")
            msg = K.first_difference(K.bare_program(c, which, identity=kept is None), _BARE[(which, kept)])
            assert msg is None, f"a bare {which} after {name}: {msg}"


# ---- a refused setter in between ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refused", list(K.REFUSED_SETTERS), ids=IDS)
def test_a_refused_setter_in_between_changes_nothing(refused):
    """P, a setter the library refuses, then s -- for every P.  Every argument refusal of a setter stands before its set_begin
    (csrc/fasta_hip.hip), so the refused call gives nothing back: the context still answers for P's operator, and s equals its model."""
    succ = successors()
    with hip.HipContext(0) as c:
        for k, p in enumerate(K.STATIONS):
            s = succ[k % len(succ)]
            K.assert_as_fresh(p, p.run(c), "before the refused setter")
            shape, L = c.shape(), c.rhs
            with pytest.raises(hip.HipError, match=rf"^\[{hip.E_ARG}\]"):
                K.REFUSED_SETTERS[refused](c)
            assert (c.shape(), c.rhs) == (shape, L)
            K.assert_as_fresh(s, s.run(c), f"after {p.name} and {refused}")


# ---- the same form, another geometry --------------------------------------------------------------------------------------------------------------------
def exact_dense_step(c, m, n, L, kind, t=None):
    """the exact step of tests/test_gpu_mc_paths.py on a dense (m, n) matrix with L columns (None: a vector), on whatever the context was"""
    from tests.test_gpu_mc_paths import assert_exact_step, assert_zero_padding
    A, X0, B = MC.step_inputs(m, n, L)
    K.write_tuning(c, {})
    c.set_matrix(A)
    if L:
        K.set_columns(c, L)
    assert c.rhs == (L or 0)
    assert_exact_step(c, A, L, X0, B, kind, MC.step_model(m, n, L, kind))
    if L:
        assert_zero_padding(c, m, n, L)


@pytest.mark.parametrize("name", ["dense pair", "dense one-pass", "dense fh_run", "dense fh_setup", "dense rhs4 group"], ids=IDS)
def test_a_dense_matrix_of_another_shape_before_and_after(name):
    s = K.BY_NAME[name]
    with hip.HipContext(0) as c:
        exact_dense_step(c, COLD_M, COLD_N, None, "shrink")
        K.assert_as_fresh(s, s.run(c), "after 40 x 600")
        exact_dense_step(c, COLD_M, COLD_N, None, "box")
        K.assert_as_fresh(s, s.run(c), "after 40 x 600, again")


def test_the_column_count_goes_1_4_16_1_on_one_matrix():
    """fh_set_rhs re-lays the vectors and the workspace out on the matrix the context holds: every launch equals its model"""
    m, n = 200, 1000                                                                # the "default" geometry of tests/mc_paths.py
    A = MC.matrix(m, n)
    from tests.test_gpu_mc_paths import assert_exact_step, assert_zero_padding
    with hip.HipContext(0) as c:
        K.write_tuning(c, {})
        c.set_matrix(A)
        for L, kind in ((1, "shrink"), (4, "box"), (16, "nonneg"), (1, "box"), (0, "shrink"), (16, "shrink")):
            K.set_columns(c, L)
            assert c.rhs == L
            _, X0, B = MC.step_inputs(m, n, L or None)
            assert_exact_step(c, A, L or None, X0, B, kind, MC.step_model(m, n, L or None, kind))
            if L:
                assert_zero_padding(c, m, n, L)


def test_the_pinned_cus_go_to_the_whole_device_and_back_with_another_operator_in_between():
    """FH_TUNE_FUSED_CUS pinned -> whole device -> pinned: other teams, other slots, a refill of the hand-off slots, the co-residency verdict taken
    again -- with a stencil and a sparse station in between.  Exact sums do not depend on the geometry: every launch equals the model."""
    from tests import test_gpu_fused_paths as G
    case, s = K.ONEPASS, K.BY_NAME["dense one-pass"]
    st = FP.operands(case)
    with hip.HipContext(0) as c:
        K.assert_as_fresh(s, s.run(c), "pinned")
        for between in ("stencil plain", "csr"):
            K.assert_as_fresh(K.BY_NAME[between], K.BY_NAME[between].run(c), "in between")
            K.write_tuning(c, {**s.tuning, hip.TUNE_FUSED_CUS: 0})
            c.set_matrix(st.A)
            c.set_loss_lsq(st.b)
            K._prox_of(c, case.kind)
            assert c.fused_launch_shape().grid != FP.expected_shape(case).grid
            G.enter(c, case, st)
            G.assert_equals_model(G.launch(c, case), case)
            c.set_tuning(hip.TUNE_FUSED_CUS, case.cus)                                  # ... and back on the operator the context holds
            G.check_geometry(c, case)
            G.assert_equals_model(G.launch(c, case), case)
            K.assert_as_fresh(s, s.run(c), "pinned again")
