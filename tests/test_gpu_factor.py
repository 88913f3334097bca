"""GPU tests of the bilinear smooth term f(Z) = .5 ||S - X Y^T||^2, Z = [X; Y] (fh_set_factorization; csrc/fh_bilinear.h: k_bl_prologue /
k_bl_pass / k_bl_extrap / k_bl_grad), every one through the C ABI.

Shapes, column counts and tuning are those of tests/factor_cases.py (several row panels and column tiles with a ragged last one each, a grid
cap that does not divide the tile count, a tile with nearly every lane idle, m = 1, n = 1, K = 1, every LB with and without padding columns,
both load policies); every test first asks the library what it is about to launch (fh_bilinear_shape) and compares that with what the case
claims.  The exact step runs on operands for which every product and every sum is exactly representable whatever the order of summation and
whether or not a multiply-add is fused (tests/test_factor_cpu.py proves it without a device): np.array_equal / ==, no tolerance.  Unit-scale
data is compared against an np.longdouble model at the tolerances of DESIGN.md section 13; the signed sums get 64 * 2^-52 of the sum of their
terms' magnitudes added."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import fasta_python_amd as fa
from fasta_python_amd import hip, proximal
from fasta_python_amd import stopping as fstop
from tests import factor_cases as FC
from tests import gpu_util as G

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float64).eps)


def first_bad(name, got, want):
    bad = np.argwhere(got != want)
    if bad.size:
        i = tuple(bad[0])
        return f"{name}: {len(bad)} wrong entries, first at {bad[0]}: {got[i]!r} != {want[i]!r}"
    return None


def padding_is_zero(c, which, rows, K, scratch=hip.VEC_T0):
    """fh_diff_norm adds up the WHOLE device buffers -- padding columns and rows -- so against a buffer that holds the same logical entries and
    untouched (zero) padding the norm is exactly zero only if the padding of `which` is."""
    c.set_vector(scratch, c.get_vector(which, rows * K))
    return c.diff_norm(which, scratch) == 0.0


def context(S, K, tuning):
    c = hip.HipContext(0)
    for key, value in tuning.items():
        c.set_tuning(key, value)
    c.set_factorization(S, K)
    return c


def set_prox(c, m, top, bottom):
    if bottom is None:
        c.set_prox(top.kind, top.mu, top.lo, top.hi)
    else:
        c.set_prox_split(m, top.kind, top.mu, top.lo, top.hi, bottom.kind, bottom.lo, bottom.hi)


def run_step(c, m, n, K, Z0, G0, top, bottom, tau, coef):
    """init -> (g0 set) -> fwd -> adj -> fwd_adj -> adj(accel): what the device returned, keyed as tests/factor_cases.py:model_step keys its model."""
    rows = m + n
    mat = lambda which: c.get_vector(which, rows * K).reshape(rows, K)
    got = {}
    set_prox(c, m, top, bottom)
    c.set_vector(hip.VEC_X0, Z0)
    got["init"] = c.init()
    got["GINIT"] = mat(hip.VEC_G0)
    c.set_vector(hip.VEC_G0, G0)
    got["fwd"] = c.fwd(tau)
    got["XHAT"], got["XPROX"] = mat(hip.VEC_XHAT), mat(hip.VEC_XPROX)
    got["adj"] = c.adj(tau)
    got["G1"] = mat(hip.VEC_G1)
    got["pair"] = c.fwd_adj(tau)
    got["G1_pair"] = mat(hip.VEC_G1)
    got["adja"] = c.adj(tau, accel=True, coef=coef)
    got["G1A"], got["X1"] = mat(hip.VEC_G1), mat(hip.VEC_X1)
    # the latest adjoint launch was accelerated: this forward launch takes the value-only pass
    got["fwd_value_only"] = c.fwd(tau)
    return got


def assert_shape(c, case):
    sh = c.bilinear_shape()
    print(f"\n{FC.case_id(case)}: {sh}", end="")
    assert sh == FC.expected_shape(case) == hip.bilinear_shape(case.m, case.n, case.K, grid_cap=case.cap, nt_loads=case.nt), (sh, FC.expected_shape(case))
    panels, last_rows, tiles, live, uneven = FC.claimed_path(case)
    assert (sh.row_panels, sh.last_rows, sh.col_tiles, sh.last_live_lanes) == (panels, last_rows, tiles, live) and (sh.tiles_max != sh.tiles_min) == uneven
    return sh


# ---- one exact step ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FC.cases(), ids=FC.case_id)
def test_one_step_is_exact(case):
    """init -> fwd -> adj -> fwd_adj -> adj(accel, coef = 1/4) with tau = 1/2: every matrix, every scalar and the padding, bit for bit; the
    value-only pass gives the bits of f the value-and-gradient pass gave."""
    m, n, K = case.m, case.n, case.K
    S, Z0, G0 = FC.exact_inputs(m, n, K)
    want = FC.exact_model(m, n, K, case.kind)
    c = context(S, K, FC.tuning_of(case))
    try:
        assert_shape(c, case)
        assert c.shape() == (m + n, m + n) and c.rhs == K
        got = run_step(c, m, n, K, Z0, G0, FC.top_tag(case.kind), FC.BOTTOM, FC.TAU, FC.COEF)
        for name in FC.MATRICES:
            msg = first_bad(name, got[name], want[name])
            assert msg is None, msg
        for block in FC.BLOCKS:
            for slot, v in want[block].items():
                assert got[block][slot] == v, f"{block} scalar {slot}: {got[block][slot]!r} != {v!r}"
        # the elementwise launch leaves the forward half of the block alone; fh_fwd_adj is both launches under one synchronisation
        assert np.array_equal(got["adj"][:hip.S_DXDG], got["fwd"][:hip.S_DXDG])
        assert np.array_equal(got["pair"][:hip.S_ALPHA], np.concatenate([got["fwd"][:hip.S_DXDG], got["adj"][hip.S_DXDG:hip.S_ALPHA]]))
        assert np.array_equal(got["G1_pair"], want["G1"])
        assert np.array_equal(got["fwd_value_only"][:hip.S_DXDG], got["fwd"][:hip.S_DXDG])
        for which in (hip.VEC_G0, hip.VEC_XHAT, hip.VEC_XPROX, hip.VEC_X1, hip.VEC_G1):
            assert padding_is_zero(c, which, m + n, K), which
    finally:
        c.close()


# ---- unit-scale data ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,K,cap,nt", FC.unit_cases(), ids=lambda v: str(v))
def test_unit_scale_step_matches_the_extended_precision_model(m, n, K, cap, nt):
    S, Z0, G0, tau = FC.unit_problem(m, n, K)
    top, bottom = proximal.Shrink(0.3), FC.BOTTOM
    terms = {}
    want = FC.model_step(S, Z0, G0, m, top, bottom, tau=tau, coef=FC.COEF, dtype=np.longdouble, terms=terms)
    case = FC.Case(m, n, FC.lb_of(K), K, cap, nt, "shrink")
    c = context(S, K, FC.tuning_of(case))
    try:
        assert c.bilinear_shape() == FC.expected_shape(case)
        runs = [run_step(c, m, n, K, Z0, G0, top, bottom, tau, FC.COEF) for _ in range(2)]
        got = runs[0]
        for key in got:                                                   # bitwise repeatable
            assert np.array_equal(got[key], runs[1][key]), key
        # the value-only pass and the value-and-gradient pass: the same bits of f
        assert got["fwd_value_only"][hip.S_FSQ] == got["fwd"][hip.S_FSQ] and np.array_equal(got["fwd_value_only"][:hip.S_DXDG], got["fwd"][:hip.S_DXDG])
        d0, d1, d2 = (np.abs(d).astype(np.float64) for d in want["D"])
        absZ = lambda Z: np.abs(np.asarray(Z, dtype=np.float64))
        gbound = lambda d, Z: np.concatenate((d @ absZ(Z)[m:], d.T @ absZ(Z)[:m]))
        bounds = {"GINIT": gbound(d0, Z0), "G1": gbound(d1, want["XPROX"]), "G1A": gbound(d2, want["X1"])}
        for name in FC.MATRICES:
            rtol, atol = FC.UNIT_TOL[name]
            w = want[name].astype(np.float64)
            extra = 64 * EPS * bounds[name] if name in bounds else 0.0      # signed sums: the bound of a summation on the magnitudes of its terms
            assert np.all(np.abs(got[name] - w) <= rtol * np.abs(w) + atol + extra), name
        worst = 0.0
        for block in FC.BLOCKS:
            for slot, v in want[block].items():
                rtol, atol = FC.scalar_tol(block, slot)
                if slot in (hip.S_DXG0, hip.S_DXDG, hip.S_RDOT):
                    atol += 64 * EPS * float(np.sum(np.abs(terms[(block, slot)])))
                dev = abs(got[block][slot] - float(v))
                print(f"\n{m}x{n}x{K} {block}[{slot}]: device {got[block][slot]!r}, model {float(v)!r}", end="")
                assert dev <= rtol * abs(float(v)) + atol, (block, slot, got[block][slot], float(v))
                worst = max(worst, dev / max(abs(float(v)), 1e-300))
        print(f"\n{m}x{n}x{K}: worst relative deviation of a scalar {worst:.2e}", end="")
        for which in (hip.VEC_XPROX, hip.VEC_X1, hip.VEC_G1):
            assert padding_is_zero(c, which, m + n, K), which
    finally:
        c.close()


# ---- elementwise kinds: the bits of the multi-column dense form ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 5, 8, 9, 16])
def test_prox_outputs_and_n_side_sums_are_those_of_the_multi_column_dense_form(K):
    """With the same kind on all rows: xhat, xprox and the seven n-side sums of the forward launch, bit for bit those of the multi-column dense
    form on the same operands.  With FH_PROX_ROWSPLIT: each half bit-equal to the uniform kind on that half."""
    m, n = 120, 83
    rows = m + n
    rng = np.random.RandomState(60 + K)
    Z0, G0 = rng.randn(rows, K), rng.randn(rows, K)
    tau = 0.37
    bil = context(rng.randn(m, n), K, {})
    dense = fa.DenseMatrixMap(np.zeros((1, rows)), rhs=K)
    try:
        dense.ctx.set_loss_lsq(np.zeros((1, K)))
        uniform = {}
        for kind in FC.TOP_KINDS:
            tag = {"shrink": proximal.Shrink(0.8), "box": proximal.Box(-0.4, 0.6)}.get(kind) or FC.top_tag(kind)
            outs = []
            for c in (bil, dense.ctx):
                c.set_prox(tag.kind, tag.mu, tag.lo, tag.hi)
                c.set_vector(hip.VEC_X0, Z0)
                c.set_vector(hip.VEC_G0, G0)
                s = c.fwd(tau)
                outs.append((c.get_vector(hip.VEC_XHAT, rows * K), c.get_vector(hip.VEC_XPROX, rows * K), s[hip.S_DXG0:hip.S_RDOT + 1]))
            for a, b in zip(*outs):
                assert np.array_equal(a, b), kind
            assert np.array_equal(outs[0][1].reshape(rows, K), tag.prox(Z0 - tau * G0, tau)), kind
            uniform[kind] = (tag, outs[0][1].reshape(rows, K))
        for tk in FC.TOP_KINDS:
            for bk in ("none", "nonneg", "box"):
                top, bottom = uniform[tk][0], uniform[bk][0]
                bil.set_prox_split(m, top.kind, top.mu, top.lo, top.hi, bottom.kind, bottom.lo, bottom.hi)
                bil.set_vector(hip.VEC_X0, Z0)
                bil.set_vector(hip.VEC_G0, G0)
                s = bil.fwd(tau)
                xp = bil.get_vector(hip.VEC_XPROX, rows * K).reshape(rows, K)
                assert np.array_equal(xp[:m], uniform[tk][1][:m]) and np.array_equal(xp[m:], uniform[bk][1][m:]), (tk, bk)
                assert abs(s[hip.S_GSUM] - np.sum(np.abs(xp[:m]))) <= 1e-12 * np.sum(np.abs(xp[:m])) + 1e-300        # the top rows only
    finally:
        bil.close()
        dense.close()


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------------------
def solve(meta, d, **extra):
    ms = FC.capture_script()
    f, gradf, g, proxg, x0 = ms.operands(fa, meta["kind"], d)
    o = ms.resolve(meta["options"], fstop)
    o.update(extra)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fa.fasta(None, None, f, gradf, g, proxg, x0, verbose=False, backend="hip", **o)


_runs = {}


def library_run(name):
    """The library-driven device solve of a fixture (its compared prefix), computed once and shared by the tests below; never modified."""
    if name not in _runs:
        meta, z, d = FC.load(name)
        k, whole = FC.compared_prefix(meta, z)
        extra = {} if whole else dict(max_iters=k, tolerance=0.0)
        _runs[name] = (solve(meta, d, driver="library", **extra), k, whole, extra)
    return _runs[name]


def assert_same_bits(a, b):
    assert a.iteration_count == b.iteration_count and a.backtracks == b.backtracks
    for f in FC.HISTORIES:
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f
    assert np.array_equal(a.solution, b.solution)


@pytest.mark.parametrize("name", FC.EXPECTED)
def test_fixture_solves_on_the_device(name):
    meta, z, d = FC.load(name)
    lib, k, whole, extra = library_run(name)
    assert lib.library_steps == lib.iteration_count and lib.device_steps == 0
    print(f"\n{name}: device {lib.iteration_count} iterations / {lib.backtracks} backtracks, reference {int(z['iteration_count'])} / {int(z['backtracks'])}", end="")
    if whole:
        assert lib.iteration_count == int(z["iteration_count"]) and lib.backtracks == int(z["backtracks"])
    else:
        assert k >= FC.MIN_PREFIX and lib.iteration_count == k and lib.backtracks == meta["backtracks_at_divergence"]
    worst = G.compare_histories(lib, lambda f: z[f], k, rtol=1e-6, atol=1e-14)
    print(f"; {k} iterations compared, worst relative deviation of a history entry {worst:.2e}")
    if whole:
        np.testing.assert_allclose(lib.solution, z["solution"], rtol=1e-5, atol=1e-6 * float(np.max(np.abs(z["solution"]))))


@pytest.mark.parametrize("name", FC.EXPECTED)
def test_library_and_python_drivers_are_bit_identical_and_runs_repeat(name):
    meta, z, d = FC.load(name)
    lib, k, whole, extra = library_run(name)
    py = solve(meta, d, driver="python", **extra)
    assert py.library_steps == 0
    assert_same_bits(py, lib)
    assert_same_bits(solve(meta, d, driver="library", device_iters=7, **extra), lib)          # cut every 7 iterations, run again: the same bits


def test_the_six_argument_form_and_the_fallbacks_of_device_iters():
    name = "nnf_30x30x1_adaptive"
    meta, z, d = FC.load(name)
    ms = FC.capture_script()
    f, gradf, g, proxg, x0 = ms.operands(fa, meta["kind"], d)
    o = ms.resolve(meta["options"], fstop)
    lib = library_run(name)[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        six = fa.fasta(None, f, gradf, g, proxg, x0, verbose=False, **o)                          # operand types decide: the device loop
        dev = fa.fasta(None, None, f, gradf, g, proxg, x0, verbose=False, driver="device", **o)   # no device-side loop: the library's
        sep = fa.fasta(None, None, f, gradf, g, proxg, x0, verbose=False, fused=False, **o)       # fh_fwd / fh_adj instead of the pair
    for other in (six, dev, sep):
        assert_same_bits(other, lib)
    assert dev.device_steps == 0 and dev.library_steps == dev.iteration_count


# ---- the example ---------------------------------------------------------------------------------------------------------------------------------------
def test_example_agrees_between_the_backends():
    """120 x 80 x 10 in the three modes, L and tau0 given (the probes are random): the first 40 iterations, or the prefix on which a permuted
    twin of the NumPy run agrees with it where that is shorter."""
    from fasta_python_amd.examples.nn_factorization import NNFactorizationProblem
    from tests.helpers import first_divergence
    ms = FC.capture_script()
    ctor = lambda backend: NNFactorizationProblem.construct(M=120, N=80, K=10, seed=31, backend=backend)
    (pn, inits), (ph, _) = ctor("numpy"), ctor("hip")
    L = float(np.linalg.norm(pn.S, 2))
    twin = ms.permuted(dict(S=pn.S, x0=np.concatenate(inits), m=120))
    ptwin = NNFactorizationProblem(twin["S"], pn.mu, backend="numpy")
    for mode in (dict(adaptive=True, accelerate=False), dict(adaptive=False, accelerate=True), dict(adaptive=False, accelerate=False)):
        opts = dict(tolerance=1e-5, evaluate_objective=True, L=L, tau0=(2 / L) / 10, max_iters=60, **mode)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            (sn, cn), (sh, ch) = pn.solve(inits, opts), ph.solve(inits, opts)
            (_, ct) = ptwin.solve((twin["x0"][:120], twin["x0"][120:]), opts)
        k = min(cn.iteration_count, ch.iteration_count, 40)
        k = min(k, first_divergence(ct.stepsizes, cn.stepsizes, min(k, ct.iteration_count)))
        print(f"\nnn_factorization {mode}: numpy {cn.iteration_count} iterations, hip {ch.iteration_count}; {k} compared", end="")
        assert k >= 20, (mode, k)
        G.compare_histories(ch, lambda f: getattr(cn, f), k, rtol=1e-6, atol=1e-12)
    ph.close()


def test_example_command_line_runs_on_the_device():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "fasta.examples.nn_factorization", "--backend", "hip", "--rows", "150", "--cols", "90", "--rank", "4"],
                         cwd=root, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Iterations (adaptive, accelerated, plain):" in out.stdout


# ---- the C ABI says no with a sentence -------------------------------------------------------------------------------------------------------------------
def refusal(code, text):
    return pytest.raises(hip.HipError, match=rf"^\[{code}\].*{text}")


def test_refusals_of_the_c_abi():
    import ctypes as C
    S = np.arange(24.0).reshape(6, 4)
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    with hip.HipContext(0) as c:
        with refusal(hip.E_STATE, "no bilinear operator"):
            c.bilinear_shape()
        with refusal(hip.E_STATE, "bilinear operator only"):
            c.set_prox_split(6, hip.PROX_SHRINK, 1.0, 0, 0, hip.PROX_BOX, 0, 1)
        for K in (0, 17):
            with refusal(hip.E_ARG, "1 to 16 columns"):
                c.set_factorization(S, K)
        assert c.lib.fh_set_factorization(c._h, pd(S), 6, 4, 3, 1) == hip.E_ARG and b"ld_host" in c.lib.fh_last_error()
        assert c.lib.fh_set_factorization(c._h, None, 6, 4, 4, 1) == hip.E_ARG
        assert c.lib.fh_set_factorization(c._h, pd(S), 0, 4, 4, 1) == hip.E_ARG and b"non-empty" in c.lib.fh_last_error()
        assert c.lib.fh_set_factorization(c._h, pd(S), 1 << 27, 4, 4, 1) == hip.E_ARG and b"below 2^27" in c.lib.fh_last_error()
        assert c.lib.fh_set_factorization(c._h, pd(S), 1 << 26, 600, 600, 16) == hip.E_ARG and b"4 GiB" in c.lib.fh_last_error()
        c.set_matrix(np.eye(6))
        c.set_rhs(2)
        with refusal(hip.E_STATE, "bilinear operator only"):
            c.set_prox_split(6, hip.PROX_SHRINK, 1.0, 0, 0, hip.PROX_BOX, 0, 1)
        c.set_factorization(S, 3)
        assert c.rhs == 3 and c.shape() == (10, 10) and c.fused_supported() == 0 and c.fused_agree() == 0 and not c.run_supported()
        for kind in (hip.PROX_LINF, hip.PROX_L1BALL, hip.PROX_TVBALL, hip.PROX_GROUP, hip.PROX_ROWBALL):
            with refusal(hip.E_ARG, "has no bilinear form"):
                c.set_prox(kind, 1.0)
        with refusal(hip.E_ARG, "unknown prox kind 9 for fh_set_prox.*fh_set_prox_split"):
            c.set_prox(hip.PROX_ROWSPLIT, 1.0)
        with refusal(hip.E_ARG, "split must equal m = 6"):
            c.set_prox_split(5, hip.PROX_SHRINK, 1.0, 0, 0, hip.PROX_BOX, 0, 1)
        with refusal(hip.E_ARG, "top rows take IDENTITY, SHRINK, NONNEG or BOX"):
            c.set_prox_split(6, hip.PROX_GROUP, 1.0, 0, 0, hip.PROX_BOX, 0, 1)
        with refusal(hip.E_ARG, "bottom rows take IDENTITY, NONNEG or BOX"):
            c.set_prox_split(6, hip.PROX_SHRINK, 1.0, 0, 0, hip.PROX_SHRINK, 0, 1)
        with refusal(hip.E_ARG, "lo <= hi"):
            c.set_prox_split(6, hip.PROX_SHRINK, 1.0, 0, 0, hip.PROX_BOX, 1, 0)
        for call in (lambda: c.set_loss_lsq(np.zeros(30)), lambda: c.set_loss_logistic(np.ones(30))):
            with refusal(hip.E_STATE, "carries its own loss"):
                call()
        with refusal(hip.E_STATE, "fixed when it is set"):
            c.set_rhs(2)
        with refusal(hip.E_STATE, "fh_apply: the bilinear operator has no linear map to apply"):
            c.apply(np.ones((10, 3)))
        c.set_prox_split(6, hip.PROX_SHRINK, 1.0, 0, 0, hip.PROX_BOX, 0, 1)
        c.set_vector(hip.VEC_X0, np.ones((10, 3)))
        c.init()
        for call, who in ((lambda: c.step(0.1), "fh_step"), (lambda: c.step_begin(0.1), "fh_step"), (lambda: c.step_accel(0.1, 0.1, True), "fh_step_accel")):
            with refusal(hip.E_STATE, who + ": the bilinear operator has no one-pass kernel"):
                call()
        with refusal(hip.E_STATE, "fh_run: the bilinear operator has no device-side loop"):
            c.run(1, hip.RunOpts(window=1), hip.RunState())
        with refusal(hip.E_STATE, "cannot be row-sharded"):
            c.comm_init(1, 0, bytes(hip.UNIQUE_ID_BYTES))
        with refusal(hip.E_STATE, "not read back"):
            c.get_matrix_rows(0, 1)
        with refusal(hip.E_STATE, "stream-read"):
            c.stream_read_ms()
        # any other operator returns the context to its previous form: vector layout, least squares, and ROWSPLIT gives way to IDENTITY
        c.set_matrix(np.eye(6))
        assert c.rhs == 0
        c.set_loss_lsq(np.zeros(6))
        c.set_vector(hip.VEC_X0, np.full(6, 3.0))
        c.set_vector(hip.VEC_G0, np.zeros(6))
        c.fwd(1.0)
        assert np.array_equal(c.get_vector(hip.VEC_XPROX, 6), np.full(6, 3.0))
        with refusal(hip.E_STATE, "no bilinear operator"):
            c.bilinear_shape()
    for kwargs in (dict(storage="f32"), dict(devices=[0, 0])):
        with hip.HipContext(0, **kwargs) as c:
            with refusal(hip.E_STATE, "float32 storage has no bilinear operator" if "storage" in kwargs else "multi-device context has no bilinear operator"):
                c.set_factorization(S, 1)


def test_gradient_at_and_setup_take_two_gradient_passes():
    m, n, K = 70, 45, 5
    rng = np.random.RandomState(9)
    S = rng.randn(m, n)
    T0, T1, Z0 = rng.randn(m + n, K), rng.randn(m + n, K), rng.randn(m + n, K)
    fz = fa.Factorization(S)
    with context(S, K, {}) as c:
        c.timing_enable(True)
        c.set_vector(hip.VEC_T0, T0)
        c.set_vector(hip.VEC_T1, T1)
        c.set_vector(hip.VEC_X0, Z0)
        s = c.setup()
        np.testing.assert_allclose(c.get_vector(hip.VEC_T2, (m + n) * K).reshape(m + n, K), fz.gradf(T0), rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(np.sqrt(s[hip.S_DG2]), np.linalg.norm(fz.gradf(T0) - fz.gradf(T1)), rtol=1e-12)
        np.testing.assert_allclose(np.sqrt(s[hip.S_DX2]), np.linalg.norm(T0 - T1), rtol=1e-12)
        np.testing.assert_allclose(s[hip.S_FSQ], fz.f(Z0), rtol=1e-12)
        np.testing.assert_allclose(c.get_vector(hip.VEC_G0, (m + n) * K).reshape(m + n, K), fz.gradf(Z0), rtol=1e-11, atol=1e-11)
        assert c.timing_get(hip.K_FWD)[1] == 3 and c.timing_get(hip.K_ADJ)[1] == 3 and c.timing_get(hip.K_FUSED)[1] == 0
