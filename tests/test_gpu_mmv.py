"""GPU tests of the multi-column form (fh_set_rhs, csrc/fh_multi.h): a matrix unknown X (n, L) over one dense A, read once per pass for
all L columns, and the row-wise l2 shrink FH_PROX_GROUP -- through the C ABI and through fasta().

Tolerances are those of tests/test_gpu_dense.py for the same quantities: matvecs rtol 1e-12, one step's scalars rtol 1e-11 / 1e-10,
whole solves iterate-for-iterate rtol 1e-5 with equal iteration counts."""
import glob
import json
import os
import warnings

import numpy as np
import pytest

import fasta_python_amd as fa
from fasta_python_amd import hip, proximal
from fasta_python_amd import stopping as fstop
from tests import gpu_util as G
from tests import helpers as H

pytestmark = pytest.mark.gpu

MMV = os.path.join(H.GOLDEN, "mmv")
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(MMV, "*.npz")))
EPS = np.finfo(np.float64).eps


@pytest.fixture(autouse=True)
def no_scratch_contexts_left_behind():
    """device_prox caches a scratch context per shape; other test files count the entries."""
    yield
    proximal.release_scratch()


def load(name):
    z = np.load(os.path.join(MMV, name + ".npz"), allow_pickle=False)
    return json.loads(str(z["meta"])), z


def solve(z, meta, **extra):
    A, B, mu = z["in_A"], z["in_B"], float(z["in_mu"])
    op = fa.DenseMatrixMap(A, rhs=B.shape[1])
    try:
        ls, reg = fa.LeastSquares(B), fa.GroupShrink(mu)
        o = H.resolve_options(dict(meta["options"], **extra), fstop)
        np.random.seed(meta["solver_seed"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return fa.fasta(op, op.H, ls.f, ls.gradf, reg.g, reg.prox, np.zeros((A.shape[1], B.shape[1])), verbose=False, backend="hip", **o)
    finally:
        op.close()


def padding_is_zero(c, which, rows, L, m_side=False):
    """Sums see the padding: fh_diff_norm adds up the WHOLE device buffers -- padding columns and padding rows -- so against a buffer that
    holds the same logical entries and untouched (zero) padding the norm is exactly zero only if the padding of `which` is."""
    v = c.get_vector(which, rows * L)
    if m_side:
        c.set_vector(hip.VEC_B, v)
        return c.diff_norm(which, hip.VEC_B) == 0.0
    c.set_vector(hip.VEC_T0, v)
    return c.diff_norm(which, hip.VEC_T0) == 0.0


# ---- apply ---------------------------------------------------------------------------------------------------------------------------------
APPLY_SHAPES = [(1, 1), (17, 33), (64, 128), (200, 1000), (513, 300), (1030, 2049)]


@pytest.mark.parametrize("L", [1, 2, 3, 5, 8, 9, 16])
@pytest.mark.parametrize("m,n", APPLY_SHAPES)
def test_apply_matches_numpy(m, n, L):
    rng = np.random.RandomState(m * 1000 + n + L)
    A = rng.randn(m, n)
    X, Y = rng.randn(n, L), rng.randn(m, L)
    op = fa.DenseMatrixMap(A, rhs=L)
    try:
        assert op.Vshape == (n, L) and op.Wshape == (m, L) and op.ctx.rhs == L and op.ctx.shape() == (m, n)
        np.testing.assert_allclose(op.device_apply(X), A @ X, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(op.device_apply(Y, adjoint=True), A.T @ Y, rtol=1e-12, atol=1e-12)
        assert np.array_equal(op(X), A @ X) and np.array_equal(op.H(Y), A.T @ Y)          # host arrays: the reference's closures
        # padding columns and rows of what the two kernels wrote read back as exact zeros: the adjoint apply's result sits in VEC_T3; the
        # same products through the solver's entry points (tau = 0, no prox: z = A x0 by K-fwd, g0 = A^T (A x0 - Y) by K-adj) sit in VEC_Z / VEC_G0
        c = op.ctx
        assert padding_is_zero(c, hip.VEC_T3, n, L)
        c.set_loss_lsq(Y)
        c.set_prox(hip.PROX_IDENTITY)
        c.set_vector(hip.VEC_X0, X)
        c.init()
        c.fwd(0.0)
        np.testing.assert_allclose(c.get_vector(hip.VEC_Z, m * L).reshape(m, L), A @ X, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(c.get_vector(hip.VEC_G0, n * L).reshape(n, L), A.T @ (A @ X - Y), rtol=1e-11, atol=1e-11)
        assert padding_is_zero(c, hip.VEC_G0, n, L) and padding_is_zero(c, hip.VEC_XPROX, n, L)
        assert padding_is_zero(c, hip.VEC_Z, m, L, m_side=True)
    finally:
        op.close()


def test_apply_on_a_matrix_beyond_2_to_the_28_elements():
    """16400 x 16390 (ragged, 2.0 GiB): the 64-bit row offsets of both kernels; the device's own copy of A is the operand on the host side."""
    m, n, L = 16400, 16390, 5
    assert m * n >= 1 << 28
    op = fa.DenseMatrixMap.synthetic(m, n, seed=5, scale=1.0 / 128, rhs=L)
    try:
        A = op.host_rows(0, m)
        rng = np.random.RandomState(1)
        X, Y = rng.randn(n, L), rng.randn(m, L)
        np.testing.assert_allclose(op.device_apply(X), A @ X, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(op.device_apply(Y, adjoint=True), A.T @ Y, rtol=1e-12, atol=1e-12)
    finally:
        op.close()


# ---- prox ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 3, 5, 8, 9, 16])
def test_group_prox_pinned_to_the_numpy_formula(L):
    """Per entry |error| <= 32 eps ||X_j||: the norm is a sum of at most 16 positive terms in any order, then sqrt, one subtraction, one
    division and one product, each correctly rounded.  Rows clearly under the threshold come back exactly zero; a zero row stays zero."""
    rng = np.random.RandomState(40 + L)
    n, mu, t = 700, 0.8, 1.3
    X = rng.randn(n, L) * rng.uniform(0.05, 3.0, size=(n, 1))
    X[5] = 0.0
    X[11] = 1e-200
    tag = fa.GroupShrink(mu)
    got = proximal.device_prox(tag, X, t)
    want = tag.prox(X, t)
    norms = np.linalg.norm(X, axis=1)
    err = np.abs(got - want)
    worst = float(np.max(err / np.maximum(norms, 1e-300)[:, None]))
    print(f"\nGROUP prox L={L}: worst |error| / ||X_j|| = {worst / EPS:.2f} eps")
    assert np.all(err <= 32 * EPS * norms[:, None])
    small = norms < t * mu * (1 - 32 * EPS)
    assert small.sum() > 20 and np.all(got[small] == 0.0)
    assert np.all(got[5] == 0.0) and not np.isnan(got).any()


@pytest.mark.parametrize("tag", [fa.Shrink(0.3), fa.NonNeg(), fa.Box(-0.4, 0.7), fa.NoProx()], ids=lambda t: type(t).__name__)
def test_elementwise_prox_on_a_matrix_is_the_vector_kernels_bit_for_bit(tag):
    rng = np.random.RandomState(9)
    X = rng.randn(333, 5)
    got = proximal.device_prox(tag, X, 0.9)
    want = proximal.device_prox(tag, X.ravel(), 0.9).reshape(X.shape)
    assert np.array_equal(got, want)
    assert np.array_equal(got, np.asarray(tag.prox(X, 0.9)) * np.ones_like(X))


@pytest.mark.parametrize("shape", [(40, 20), (7, 3), (5, 4, 6)])
def test_arrays_the_matrix_form_does_not_serve_keep_the_flat_vector_path(shape):
    """device_prox on an array that is wider than 16 columns, not 2-D, or under a level-search tag is flattened, as before the matrix form existed."""
    rng = np.random.RandomState(len(shape) * 100 + shape[1])
    X = rng.randn(*shape)
    tags = [fa.LinfProx(0.4), fa.L1Ball(1.5)] + ([fa.Shrink(0.1), fa.NonNeg(), fa.Box(-0.2, 0.3)] if shape != (7, 3) else [])
    for tag in tags:
        got = proximal.device_prox(tag, X, 1.0)
        flat = proximal.device_prox(tag, X.ravel(), 1.0).reshape(X.shape)
        assert got.shape == X.shape and np.array_equal(got, flat), type(tag).__name__
        assert np.array_equal(tag.prox_on_device(X, 1.0), flat)
    np.testing.assert_allclose(proximal.device_prox(fa.Shrink(0.1), X, 1.0), fa.Shrink(0.1).prox(X, 1.0), rtol=0, atol=0)
    with pytest.raises(ValueError):
        proximal.device_prox(fa.GroupShrink(0.1), np.zeros((4, 20)), 1.0)
    with pytest.raises(ValueError):
        proximal.device_prox(fa.GroupShrink(0.1), np.zeros(8), 1.0)


# ---- one step ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,kind", [(5, "group"), (16, "group"), (3, "shrink"), (2, "nonneg"), (9, "group")])
def test_single_step_scalars_match_numpy(L, kind):
    rng = np.random.RandomState(3 + L)
    m, n, mu, tau = 96, 200, 0.05, 0.3
    A = rng.randn(m, n) / 10
    B = rng.randn(m, L)
    X0 = rng.randn(n, L) * 0.1
    tag = {"group": fa.GroupShrink(mu), "shrink": fa.Shrink(mu), "nonneg": fa.NonNeg()}[kind]
    op = fa.DenseMatrixMap(A, rhs=L)
    c = op.ctx
    try:
        c.set_loss_lsq(B)
        c.set_prox(tag.kind, tag.mu)
        c.set_vector(hip.VEC_X0, X0)
        s0 = c.init()
        G0 = A.T @ (A @ X0 - B)
        np.testing.assert_allclose(c.get_vector(hip.VEC_G0, n * L).reshape(n, L), G0, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(s0[hip.S_FSQ], np.sum((A @ X0 - B) ** 2), rtol=1e-12)
        gsum = (lambda V: np.sum(np.sqrt(np.sum(V * V, axis=1)))) if kind == "group" else (lambda V: np.abs(V).sum())
        np.testing.assert_allclose(s0[hip.S_GSUM], gsum(X0), rtol=1e-12)
        np.testing.assert_allclose(s0[hip.S_GMAX], np.abs(X0).max(), rtol=0)
        s = c.fwd(tau)
        Xh = X0 - tau * G0
        Xp = tag.prox(Xh, tau)
        np.testing.assert_allclose(c.get_vector(hip.VEC_XHAT, n * L).reshape(n, L), Xh, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(c.get_vector(hip.VEC_XPROX, n * L).reshape(n, L), Xp, rtol=1e-12, atol=1e-14)
        dX, Z = Xp - X0, A @ Xp
        np.testing.assert_allclose(c.get_vector(hip.VEC_Z, m * L).reshape(m, L), Z, rtol=1e-12, atol=1e-13)
        want = {hip.S_FSQ: np.sum((Z - B) ** 2), hip.S_DXG0: np.sum(dX * G0), hip.S_DX2: np.sum(dX * dX),
                hip.S_XH2: np.sum((Xp - Xh) ** 2), hip.S_G02: np.sum(G0 * G0), hip.S_GSUM: gsum(Xp), hip.S_GMAX: np.abs(Xp).max(),
                hip.S_RDOT: np.sum((X0 - Xp) * (Xp - X0))}                    # x_accel0 = x0 after init
        for k, v in want.items():
            np.testing.assert_allclose(s[k], v, rtol=1e-11, atol=1e-13, err_msg=str(k))
        a = c.adj(tau)
        G1 = A.T @ (Z - B)
        dG = G1 + (Xh - X0) / tau
        np.testing.assert_allclose(c.get_vector(hip.VEC_G1, n * L).reshape(n, L), G1, rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(a[hip.S_DXDG], np.sum(dX * dG), rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(a[hip.S_DG2], np.sum(dG * dG), rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(a[hip.S_FSQ_ADJ], np.sum((Z - B) ** 2), rtol=1e-11)
        np.testing.assert_allclose(a[hip.S_GSUM_ADJ], gsum(Xp), rtol=1e-11)
        np.testing.assert_allclose(a[hip.S_XH2_ADJ], np.sum((Xp - Xh) ** 2), rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(a[hip.S_GMAX_ADJ], np.abs(Xp).max(), rtol=1e-12)
        assert np.array_equal(a[:hip.S_DXDG], s[:hip.S_DXDG])                      # K-adj leaves the forward half of the block alone
        pair = c.fwd_adj(tau)                                                    # both launches under one synchronisation: the same block
        assert np.array_equal(pair[:hip.S_ALPHA], np.concatenate([s[:hip.S_DXDG], a[hip.S_DXDG:hip.S_ALPHA]]))
        # accelerated variant of the same step: extrapolated x1 / z1 (fasta/__init__.py:242-245)
        coef = 0.37
        a2 = c.adj(tau, accel=True, coef=coef)
        X1 = Xp + coef * (Xp - X0)
        Z1 = Z + coef * (Z - A @ X0)
        np.testing.assert_allclose(c.get_vector(hip.VEC_X1, n * L).reshape(n, L), X1, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(a2[hip.S_FSQ_ADJ], np.sum((Z1 - B) ** 2), rtol=1e-11)
        np.testing.assert_allclose(c.get_vector(hip.VEC_G1, n * L).reshape(n, L), A.T @ (Z1 - B), rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(a2[hip.S_XH2_ADJ], np.sum((X1 - Xh) ** 2), rtol=1e-11)
        np.testing.assert_allclose(a2[hip.S_GSUM_ADJ], gsum(X1), rtol=1e-11)
        np.testing.assert_allclose(a2[hip.S_GMAX_ADJ], np.abs(X1).max(), rtol=1e-12)
        # padding columns (and rows) of everything the kernels wrote are exact zeros
        for which in (hip.VEC_G0, hip.VEC_XHAT, hip.VEC_XPROX, hip.VEC_X1, hip.VEC_G1):
            assert padding_is_zero(c, which, n, L), which
        assert padding_is_zero(c, hip.VEC_Z, m, L, m_side=True)
    finally:
        op.close()


# ---- whole solves --------------------------------------------------------------------------------------------------------------------------
def prefix_of(meta, z):
    """Iterations compared: all of them, or -- the backtracking case -- up to where the oracle parts from a permuted copy of itself."""
    return min(int(meta.get("permuted_divergence", int(z["iteration_count"]))), int(z["iteration_count"]))


@pytest.mark.parametrize("fused", ["auto", False])
@pytest.mark.parametrize("name", CASES)
def test_fixture_solves_on_the_device(name, fused):
    meta, z = load(name)
    k = prefix_of(meta, z)
    full = k == int(z["iteration_count"])
    extra = {} if full else dict(max_iters=k, tolerance=0.0)
    lib = solve(z, meta, driver="library", fused=fused, **extra)
    py = solve(z, meta, driver="python", fused=fused, **extra)
    assert lib.library_steps == lib.iteration_count and py.library_steps == 0
    get = lambda f: z[f] if f in z.files else None
    if full:
        assert lib.iteration_count == int(z["iteration_count"]) and lib.backtracks == int(z["backtracks"])
    worst = G.compare_histories(lib, get, k, rtol=1e-5, atol=1e-14)
    print(f"\n{name} fused={fused}: {k} iterations compared, worst relative deviation of a history entry {worst:.2e}")
    if full:
        np.testing.assert_allclose(lib.solution, z["solution"], rtol=1e-5, atol=1e-9)
    # the two drivers take the same decisions from the same scalars: bit-identical
    assert py.iteration_count == lib.iteration_count and py.backtracks == lib.backtracks
    for f in ("residuals", "norm_residuals", "stepsizes", "objectives"):
        assert np.array_equal(getattr(py, f), getattr(lib, f), equal_nan=True), f
    assert np.array_equal(py.solution, lib.solution)


@pytest.mark.parametrize("name", ["mmv_20x30x10_adaptive", "mmv_20x30x10_accelerated"])
def test_device_driver_falls_back_to_the_library_loop(name):
    meta, z = load(name)
    lib = solve(z, meta, driver="library")
    dev = solve(z, meta, driver="device")
    assert dev.device_steps == 0 and dev.library_steps == dev.iteration_count == lib.iteration_count
    assert np.array_equal(dev.stepsizes, lib.stepsizes) and np.array_equal(dev.solution, lib.solution)


def test_mmv_example_runs_on_the_device():
    from fasta_python_amd.examples.mmv import MMVProblem
    meta, z = load("mmv_20x30x10_adaptive")
    P, X0 = MMVProblem.construct(seed=meta["problem_seed"], backend="hip")
    try:
        np.random.seed(meta["solver_seed"])
        sol, c = P.solve(X0, dict(meta["options"]))
    finally:
        P.close()
    assert c.iteration_count == int(z["iteration_count"])
    np.testing.assert_allclose(sol, z["solution"], rtol=1e-5, atol=1e-9)


# ---- columns are independent where they should be -------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [3, 8])
def test_columns_of_a_separable_problem_solve_as_single_column_solves(L):
    rng = np.random.RandomState(50 + L)
    m, n, mu, iters = 120, 90, 0.05, 30
    A = rng.randn(m, n) / np.sqrt(m)
    B = rng.randn(m, L)
    opts = dict(adaptive=False, backtrack=False, L=4.0, tau0=0.2, max_iters=iters, tolerance=0.0, verbose=False, backend="hip")
    reg = fa.Shrink(mu)
    ls = fa.LeastSquares(B)
    got = fa.fasta(A, A.T, ls.f, ls.gradf, reg.g, reg.prox, np.zeros((n, L)), **opts)
    assert got.iteration_count == iters and got.solution.shape == (n, L)
    for j in range(L):
        lj = fa.LeastSquares(B[:, j].copy())
        one = fa.fasta(A, A.T, lj.f, lj.gradf, reg.g, reg.prox, np.zeros(n), **opts)
        np.testing.assert_allclose(got.solution[:, j], one.solution, rtol=1e-12)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def status_of(fn, *args):
    with pytest.raises(hip.HipError) as e:
        fn(*args)
    text = str(e.value)
    code = int(text[1:text.index("]")])
    assert len(text) > len(f"[{code}] ") + 10, text                      # a sentence, not just a code
    return code


def test_refusals_return_their_code_and_leave_the_context_usable():
    rng = np.random.RandomState(0)
    A = rng.randn(40, 24)
    op = fa.DenseMatrixMap(A, rhs=4)
    c = op.ctx
    try:
        refused = (hip.E_ARG, hip.E_STATE)
        assert status_of(c.set_rhs, 17) == hip.E_ARG
        for kind in (hip.PROX_LINF, hip.PROX_L1BALL, hip.PROX_TVBALL):
            assert status_of(c.set_prox, kind, 1.0) in refused
        assert status_of(c.set_loss_logistic, np.ones(40 * 4)) in refused
        assert status_of(c.comm_init, 1, 0, bytes(hip.UNIQUE_ID_BYTES)) == hip.E_STATE
        c.set_loss_lsq(rng.randn(40, 4))
        c.set_prox(hip.PROX_GROUP, 0.1)
        c.set_vector(hip.VEC_X0, np.zeros((24, 4)))
        c.init()
        assert c.fused_supported() == 0 and c.fused_agree() == 0 and not c.run_supported()
        assert status_of(c.step, 0.1) == hip.E_STATE
        assert status_of(c.step_begin, 0.1) == hip.E_STATE
        assert status_of(c.step_accel, 0.1, 0.0, True) == hip.E_STATE
        o, st = hip.RunOpts(), hip.RunState()
        o.window, o.stop_rule = 10, 3
        with pytest.raises(hip.HipError) as e:
            c.run(4, o, st)
        assert str(e.value).startswith(f"[{hip.E_STATE}]")
        s = c.fwd(0.1)                                                   # still usable
        assert np.isfinite(s[hip.S_FSQ])
        assert status_of(c.set_vector, hip.VEC_X0, np.zeros(24)) == hip.E_ARG         # the vector form's length
    finally:
        op.close()
    for make in (lambda: hip.HipContext(0, storage="f32"), lambda: hip.HipContext(devices=[0, 0])):
        with make() as c:
            c.set_matrix(A)
            assert status_of(c.set_rhs, 2) == hip.E_STATE
    with hip.HipContext(0) as c:
        assert status_of(c.set_rhs, 2) == hip.E_STATE                    # no operator yet
        c.set_stencil(8, 8)
        assert status_of(c.set_rhs, 2) == hip.E_STATE
        c.set_matrix(A)
        assert status_of(c.set_prox, hip.PROX_GROUP, 1.0) == hip.E_ARG   # GROUP only in multi-column form
        c.set_prox(hip.PROX_LINF, 1.0)
        assert status_of(c.set_rhs, 2) == hip.E_STATE
        c.set_loss_logistic(np.ones(40))
        c.set_prox(hip.PROX_SHRINK, 1.0)
        assert status_of(c.set_rhs, 2) == hip.E_STATE


def test_set_rhs_is_refused_on_a_context_with_a_communicator(tmp_path):
    """A rank of a row-sharded run (fh_comm_init) has no multi-column form.  A fresh process with the test-only RCCL stand-in, one rank."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = str(tmp_path / "libmock_rccl.so")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", lib, os.path.join(root, "tests", "mock_rccl", "mock_rccl.cpp"), "-lrt"],
                   check=True, capture_output=True, timeout=300)
    script = (
        "import numpy as np\n"
        "from fasta_python_amd import hip\n"
        "with hip.HipContext(0) as c:\n"
        "    c.set_matrix(np.arange(24.0).reshape(6, 4))\n"
        "    c.comm_init(1, 0, hip.comm_unique_id())\n"
        "    try:\n"
        "        c.set_rhs(2)\n"
        "    except hip.HipError as e:\n"
        "        assert str(e).startswith('[%d]' % hip.E_STATE) and 'communicator' in str(e), str(e)\n"
        "    else:\n"
        "        raise SystemExit('fh_set_rhs accepted a context with a communicator')\n"
        "    assert c.rhs == 0\n"
        "    y = c.apply(np.ones(4))\n"                              # still usable, in the vector form
        "    assert np.allclose(y, np.arange(24.0).reshape(6, 4).sum(axis=1))\n"
        "    c.comm_destroy()\n"
        "    c.set_rhs(2)\n"
        "    assert c.rhs == 2\n"
        "print('refused')\n")
    r = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, FASTA_RCCL_LIB=lib), cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "refused" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def test_fasta_refuses_or_takes_the_host_loop_for_operands_without_a_matrix_form():
    rng = np.random.RandomState(1)
    A, B = rng.randn(30, 20), rng.randn(30, 3)
    X0 = np.zeros((20, 3))
    ls = fa.LeastSquares(B)
    for reg in (fa.LinfProx(0.1), fa.L1Ball(1.0)):
        with pytest.raises(TypeError, match="matrix"):
            fa.fasta(A, A.T, ls.f, ls.gradf, reg.g, reg.prox, X0, backend="hip", verbose=False)


def test_set_rhs_zero_restores_the_vector_form_bit_for_bit():
    name = "sparse_ls_64x128_adaptive"
    meta, z = H.load_case(name)
    data = H.case_data(meta, z)
    fresh = G.run_hip(meta["kind"], data, meta["options"], meta["solver_seed"])
    op = fa.DenseMatrixMap(np.asarray(data["A"]))
    try:
        c = op.ctx
        c.set_rhs(5)
        assert c.rhs == 5
        c.set_loss_lsq(np.ones((64, 5)))
        c.set_prox(hip.PROX_GROUP, 0.3)
        c.set_vector(hip.VEC_X0, np.ones((128, 5)))
        c.init()
        c.fwd(0.01)
        c.adj(0.01)
        c.set_rhs(0)
        assert c.rhs == 0
        ls, reg = fa.LeastSquares(data["b"]), fa.Shrink(float(data["mu"]))
        np.random.seed(meta["solver_seed"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            again = fa.fasta(op, op.H, ls.f, ls.gradf, reg.g, reg.prox, np.zeros(128), verbose=False, backend="hip",
                             **H.resolve_options(meta["options"], fstop))
    finally:
        op.close()
    assert again.iteration_count == fresh.iteration_count
    for f in ("residuals", "norm_residuals", "stepsizes", "objectives"):
        assert np.array_equal(getattr(again, f), getattr(fresh, f)), f
    assert np.array_equal(again.solution, fresh.solution)


# ---- worth having --------------------------------------------------------------------------------------------------------------------------
def median_pair_ms(c, tau, launches):
    """Median over `launches` of the HIP-event time of one K-fwd plus one K-adj (fh_timing_get), after a warm-up."""
    for _ in range(3):
        c.fwd(tau)
        c.adj(tau)
    c.timing_enable(True)
    ms = []
    for _ in range(launches):
        c.timing_reset()
        c.fwd(tau)
        c.adj(tau)
        ms.append(c.timing_get(hip.K_FWD)[0] + c.timing_get(hip.K_ADJ)[0])
    c.timing_enable(False)
    return float(np.median(ms))


def test_eight_columns_cost_less_than_eight_vector_passes():
    """16384^2 (A = 2 GiB, beyond the 256 MiB last-level cache), L = 8: the new K-fwd + K-adj pair against 8 x the unchanged vector pair
    on the same matrix in the same process.  The byte model predicts ~8x headroom: this only catches a design that fails to share the read."""
    n, L, tau = 16384, 8, 1e-3
    op = fa.DenseMatrixMap.synthetic(n, n, seed=3, scale=1.0 / 128)
    try:
        c = op.ctx
        rng = np.random.RandomState(0)
        c.set_loss_lsq(rng.randn(n))
        c.set_prox(hip.PROX_SHRINK, 0.01)
        c.set_vector(hip.VEC_X0, rng.randn(n) * 0.01)
        c.init()
        old = median_pair_ms(c, tau, 20)
        c.set_rhs(L)
        c.set_loss_lsq(rng.randn(n, L))
        c.set_prox(hip.PROX_GROUP, 0.01)
        c.set_vector(hip.VEC_X0, rng.randn(n, L) * 0.01)
        c.init()
        new = median_pair_ms(c, tau, 20)
    finally:
        op.close()
    print(f"\n16384^2: vector K-fwd + K-adj {old:.3f} ms, 8 columns {new:.3f} ms = {new / old:.2f} x one vector pass ({8 * old / new:.2f} x faster than 8 passes)")
    assert new < 8 * old
