"""GPU tests of the sparse operator (fh_set_matrix_csr, csrc/fh_sparse.h): A kept by rows and by columns on the device, both directions as
gathers -- through the C ABI and through fasta().

Tolerances: an apply is compared componentwise against SciPy with |error| <= 1e-12 * (|A| |v|) -- the project's apply tolerance; a row's
rounding bound k * u * sum |a v| stays under it for k <= 9000 entries -- whole solves with those of DESIGN section 2: equal iteration and
backtrack counts, histories rtol 1e-6, solution rtol 1e-5 with a floor of 1e-6 of its largest entry."""
import glob
import json
import os
import warnings

import numpy as np
import pytest
from scipy import sparse as sp

import fasta_python_amd as fa
from fasta_python_amd import hip
from fasta_python_amd import stopping as fstop
from tests import gpu_util as G
from tests import helpers as H
from tests import sparse_lanes as SL
from tests.test_sparse_cpu import capture_script

pytestmark = pytest.mark.gpu

SPARSE = os.path.join(H.GOLDEN, "sparse")
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(SPARSE, "*.npz")))
FIELDS = ("residuals", "norm_residuals", "stepsizes", "objectives")


def load(name):
    z = np.load(os.path.join(SPARSE, name + ".npz"), allow_pickle=False)
    return json.loads(str(z["meta"])), z, {k[3:]: z[k] for k in z.files if k.startswith("in_")}


def tags(kind, d):
    """(loss, prox tag or None) of a fixture kind: the device-tagged twins of scripts/make_sparse_golden.py:closures."""
    loss = fa.LogisticLoss(d["b"]) if kind == "logistic" else fa.LeastSquares(d["b"])
    reg = {"lasso": lambda: fa.Shrink(float(d["mu"])), "logistic": lambda: fa.Shrink(float(d["mu"])), "skewed": lambda: fa.Shrink(float(d["mu"])),
           "nnls": fa.NonNeg, "box": lambda: fa.Box(float(d["lo"]), float(d["hi"])), "gnone": lambda: None}[kind]()
    return loss, reg


def solve(meta, d, op=None, **extra):
    S = capture_script().matrix_of(d)
    own = op is None
    op = fa.SparseMatrixMap(S) if own else op
    try:
        loss, reg = tags(meta["kind"], d)
        g, proxg = (None, None) if reg is None else (reg.g, reg.prox)
        o = H.resolve_options(dict(meta["options"], **extra), fstop)
        np.random.seed(meta["solver_seed"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return fa.fasta(op, op.H, loss.f, loss.gradf, g, proxg, np.zeros(S.shape[1]), verbose=False, backend="hip", **o)
    finally:
        if own:
            op.close()


def random_sparse(m, n, density, seed):
    rng = np.random.RandomState(seed)
    S = sp.random(m, n, density=density, format="csr", random_state=rng, data_rvs=rng.standard_normal)
    S.sort_indices()
    return S


def skewed():
    return capture_script().matrix_of(load("skewed_257x515")[2])


def long_col():
    """9000 x 51: one fully dense column (9000 entries) next to columns of about 9 -- the A^T copy hands it to a workgroup of its own."""
    return sp.vstack([random_sparse(50, 9000, 0.001, 5), sp.csr_matrix(np.random.RandomState(6).randn(1, 9000))]).T.tocsr()


def long_both():
    """5000 x 6000 with about 3 entries per row, one fully dense row and one fully dense column: whole-workgroup rows on both copies."""
    S = random_sparse(5000, 6000, 0.0005, 51).tolil()
    rng = np.random.RandomState(52)
    S[1234, :] = rng.randn(6000)
    S[:, 4321] = rng.randn(5000).reshape(-1, 1)
    S = S.tocsr()
    S.sort_indices()
    return S


def long_rows_of(S):
    """(rows of A, rows of A^T) the host hands to whole workgroups: its rule as tests/sparse_lanes.py restates it (csrc/fasta_hip.hip: sp_upload_side)."""
    return tuple(int(la.long_rows.size) for la in SL.both_lanes(S, 0))


def test_the_long_row_cases_reach_the_whole_workgroup_path_on_both_copies():
    assert long_rows_of(APPLY["one_long_row"]()) == (1, 0) and long_rows_of(long_col()) == (0, 1) and long_rows_of(long_both()) == (1, 1)
    assert long_rows_of(skewed()) == (1, 0)


# ---- apply ---------------------------------------------------------------------------------------------------------------------------------
APPLY = {
    "1xn": lambda: random_sparse(1, 300, 0.3, 1), "mx1": lambda: random_sparse(300, 1, 0.3, 2), "1x1": lambda: sp.csr_matrix(np.array([[2.5]])),
    "empty": lambda: sp.csr_matrix((37, 53)), "ragged": lambda: random_sparse(203, 1001, 0.02, 3), "tall": lambda: random_sparse(1030, 17, 0.2, 4),
    "skewed": skewed, "one_long_row": lambda: sp.vstack([random_sparse(50, 9000, 0.001, 5), sp.csr_matrix(np.random.RandomState(6).randn(1, 9000))]).tocsr(),
    "one_long_col": lambda: long_col(), "long_row_and_col": lambda: long_both(),
    "4096_0.1%": lambda: random_sparse(4096, 4096, 0.001, 7), "4096_1%": lambda: random_sparse(4096, 4096, 0.01, 8),
    "4096_10%": lambda: random_sparse(4096, 4096, 0.1, 9),
}


def assert_apply(got, S, v):
    want = S @ v
    bound = 1e-12 * (abs(S) @ np.abs(v))
    err = np.abs(got - want)
    worst = float(np.max(err / np.maximum(bound, 1e-300))) if err.size and err.max() > 0 else 0.0
    print(f" worst |error| / (1e-12 |A||v|) = {worst:.3e}", end="")
    assert np.all(err <= bound)


@pytest.mark.parametrize("nt", [None, 0, 1], ids=["nt_auto", "nt0", "nt1"])
@pytest.mark.parametrize("shape", list(APPLY))
def test_apply_matches_scipy_in_both_directions(shape, nt):
    """nt: the streaming loads of values and indices as the size rule picks them, plain, or non-temporal (FH_TUNE_NT_LOADS)."""
    S = APPLY[shape]()
    m, n = S.shape
    rng = np.random.RandomState(11)
    v, w = rng.randn(n), rng.randn(m)
    op = fa.SparseMatrixMap(S, tuning=None if nt is None else {hip.TUNE_NT_LOADS: nt})
    try:
        c = op.ctx
        assert c.shape() == (m, n) and c.nnz() == S.nnz == op.nnz
        print(f"\n{shape}: nnz {S.nnz}", end="")
        assert_apply(op.device_apply(v), S, v)
        assert_apply(op.device_apply(w, adjoint=True), S.T.tocsr(), w)
        # the adjointness identity <A u, v> = <u, A^T v> on the device's own products
        lhs, rhs = float(np.dot(op.device_apply(v), w)), float(np.dot(v, op.device_apply(w, adjoint=True)))
        print(f"; <Au,v> - <u,A^T v> = {lhs - rhs:.3e} of {lhs:.6e}")
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))
        assert np.array_equal(op(v), S @ v) and np.array_equal(op.H(w), S.T @ w)          # host arrays: the reference's closures
    finally:
        op.close()


def test_apply_is_bitwise_repeatable_and_the_same_on_a_second_context():
    S = random_sparse(3000, 2000, 0.01, 21)
    v, w = np.random.RandomState(1).randn(2000), np.random.RandomState(2).randn(3000)
    outs = []
    for _ in range(2):
        op = fa.SparseMatrixMap(S)
        try:
            outs.append((op.device_apply(v), op.device_apply(w, adjoint=True), op.device_apply(v), op.device_apply(w, adjoint=True)))
        finally:
            op.close()
    for a in outs:
        assert np.array_equal(a[0], a[2]) and np.array_equal(a[1], a[3])
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


# ---- one step ------------------------------------------------------------------------------------------------------------------------------
STEP_MATRICES = {"uniform": lambda: random_sparse(190, 333, 0.06, 14), "long_col": lambda: long_col() * 0.05,
                 "long_both": lambda: long_both() * 0.05}


@pytest.mark.parametrize("nt", [0, 1], ids=["nt0", "nt1"])
@pytest.mark.parametrize("kind,matrix", [("shrink", "uniform"), ("nonneg", "uniform"), ("box", "uniform"), ("none", "uniform"), ("logistic", "uniform"),
                                         ("shrink", "long_col"), ("logistic", "long_col"), ("shrink", "long_both"), ("none", "long_both")])
def test_single_step_scalars_match_numpy(kind, matrix, nt):
    """One K-fwd, one K-adj (mode 0, plain and accelerated), fh_init's mode-1 adjoint: vectors and all scalars against NumPy.  On the long_*
    matrices the dense column's g1 and its n-side epilogue come from the whole-workgroup block of k_sp_adj."""
    rng = np.random.RandomState(13)
    S = STEP_MATRICES[matrix]()
    (m, n), mu, tau = S.shape, 0.05, 0.3
    x0 = rng.randn(n) * 0.1
    b = np.sign(rng.randn(m)) if kind == "logistic" else rng.randn(m)
    tag = {"shrink": fa.Shrink(mu), "logistic": fa.Shrink(mu), "nonneg": fa.NonNeg(), "box": fa.Box(-0.05, 0.08), "none": fa.NoProx()}[kind]
    if kind == "logistic":
        floss, grad = (lambda z: np.sum(np.log(1 + np.exp(z)) - (b == 1) * z)), (lambda z: -b / (1 + np.exp(b * z)))
    else:
        floss, grad = (lambda z: np.sum((z - b) ** 2)), (lambda z: z - b)
    op = fa.SparseMatrixMap(S, tuning={hip.TUNE_NT_LOADS: nt})
    c = op.ctx
    try:
        (c.set_loss_logistic if kind == "logistic" else c.set_loss_lsq)(b)
        c.set_prox(tag.kind, tag.mu, tag.lo, tag.hi)
        c.set_vector(hip.VEC_X0, x0)
        s0 = c.init()
        g0 = S.T @ grad(S @ x0)
        np.testing.assert_allclose(c.get_vector(hip.VEC_G0, n), g0, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(s0[hip.S_FSQ], floss(S @ x0), rtol=1e-12)
        np.testing.assert_allclose(s0[hip.S_GSUM], np.abs(x0).sum(), rtol=1e-12)
        s = c.fwd(tau)
        xh = x0 - tau * g0
        xp = np.asarray(tag.prox(xh, tau))
        np.testing.assert_allclose(c.get_vector(hip.VEC_XHAT, n), xh, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(c.get_vector(hip.VEC_XPROX, n), xp, rtol=1e-12, atol=1e-14)
        dx, z = xp - x0, S @ xp
        np.testing.assert_allclose(c.get_vector(hip.VEC_Z, m), z, rtol=1e-12, atol=1e-13)
        want = {hip.S_FSQ: floss(z), hip.S_DXG0: np.sum(dx * g0), hip.S_DX2: np.sum(dx * dx), hip.S_XH2: np.sum((xp - xh) ** 2),
                hip.S_G02: np.sum(g0 * g0), hip.S_GSUM: np.abs(xp).sum(), hip.S_GMAX: np.abs(xp).max(), hip.S_RDOT: np.sum((x0 - xp) * (xp - x0))}
        for k, v in want.items():
            np.testing.assert_allclose(s[k], v, rtol=1e-11, atol=1e-13, err_msg=str(k))
        a = c.adj(tau)
        g1 = S.T @ grad(z)
        dg = g1 + (xh - x0) / tau
        np.testing.assert_allclose(c.get_vector(hip.VEC_G1, n), g1, rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(a[hip.S_DXDG], np.sum(dx * dg), rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(a[hip.S_DG2], np.sum(dg * dg), rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(a[hip.S_FSQ_ADJ], floss(z), rtol=1e-11)
        np.testing.assert_allclose(a[hip.S_GSUM_ADJ], np.abs(xp).sum(), rtol=1e-11)
        np.testing.assert_allclose(a[hip.S_XH2_ADJ], np.sum((xp - xh) ** 2), rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(a[hip.S_GMAX_ADJ], np.abs(xp).max(), rtol=1e-12)
        assert np.array_equal(a[:hip.S_DXDG], s[:hip.S_DXDG])                      # K-adj leaves the forward half of the block alone
        pair = c.fwd_adj(tau)                                                    # both launches under one synchronisation: the same block
        assert np.array_equal(pair[:hip.S_ALPHA], np.concatenate([s[:hip.S_DXDG], a[hip.S_DXDG:hip.S_ALPHA]]))
        coef = 0.37                                                              # accelerated variant (fasta/__init__.py:242-245)
        a2 = c.adj(tau, accel=True, coef=coef)
        x1, z1 = xp + coef * (xp - x0), z + coef * (z - S @ x0)
        np.testing.assert_allclose(c.get_vector(hip.VEC_X1, n), x1, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(a2[hip.S_FSQ_ADJ], floss(z1), rtol=1e-11)
        np.testing.assert_allclose(c.get_vector(hip.VEC_G1, n), S.T @ grad(z1), rtol=1e-11, atol=1e-13)
        np.testing.assert_allclose(a2[hip.S_XH2_ADJ], np.sum((x1 - xh) ** 2), rtol=1e-11)
        np.testing.assert_allclose(a2[hip.S_GSUM_ADJ], np.abs(x1).sum(), rtol=1e-11)
        # timing runs under the existing kernel ids
        c.timing_enable(True)
        c.fwd(tau), c.adj(tau), c.init()
        assert c.timing_get(hip.K_FWD)[1] >= 2 and c.timing_get(hip.K_ADJ)[1] >= 2 and c.timing_get(hip.K_AUX)[1] >= 1
        assert c.timing_get(hip.K_FUSED)[1] == 0
    finally:
        op.close()


@pytest.mark.parametrize("tag", [fa.Shrink(0.3), fa.NonNeg(), fa.Box(-0.4, 0.7), fa.NoProx()], ids=lambda t: type(t).__name__)
def test_elementwise_prox_outputs_are_the_vector_kernels_bit_for_bit(tag):
    """Same x0, same g0 (set, not computed), same tau: xhat and xprox of the sparse prologue == those of k_fwd_dense."""
    n, tau = 1003, 0.9
    rng = np.random.RandomState(17)
    x0, g0 = rng.randn(n), rng.randn(n)
    outs = []
    for op in (fa.SparseMatrixMap(random_sparse(40, n, 0.05, 18)), fa.DenseMatrixMap(rng.randn(24, n))):
        try:
            c = op.ctx
            c.set_loss_lsq(np.zeros(op.Wshape[0]))
            c.set_prox(tag.kind, tag.mu, tag.lo, tag.hi)
            c.set_vector(hip.VEC_X0, x0)
            c.init()
            c.set_vector(hip.VEC_G0, g0)
            c.fwd(tau)
            outs.append((c.get_vector(hip.VEC_XHAT, n), c.get_vector(hip.VEC_XPROX, n)))
        finally:
            op.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[0][1], np.asarray(tag.prox(x0 - tau * g0, tau)) * np.ones(n))


# ---- whole solves --------------------------------------------------------------------------------------------------------------------------
def prefix_of(meta, z):
    """Iterations compared: all of them, or -- the forced-backtracking case -- up to where the oracle parts from a permuted copy of itself."""
    return min(int(meta.get("permuted_divergence", int(z["iteration_count"]))), int(z["iteration_count"]))


def assert_solution(got, want):
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6 * float(np.max(np.abs(want))))


@pytest.mark.parametrize("name", CASES)
def test_fixture_solves_on_the_device(name):
    meta, z, d = load(name)
    k = prefix_of(meta, z)
    full = k == int(z["iteration_count"])
    extra = {} if full else dict(max_iters=k, tolerance=0.0)
    lib = solve(meta, d, driver="library", **extra)
    py = solve(meta, d, driver="python", **extra)
    assert lib.library_steps == lib.iteration_count and lib.device_steps == 0 and py.library_steps == 0
    print(f"\n{name}: device {lib.iteration_count} iterations / {lib.backtracks} backtracks, reference {int(z['iteration_count'])} / {int(z['backtracks'])}", end="")
    if full:
        assert lib.iteration_count == int(z["iteration_count"]) and lib.backtracks == int(z["backtracks"])
    else:
        assert lib.iteration_count == k and lib.backtracks == meta["backtracks_at_divergence"]
    worst = G.compare_histories(lib, lambda f: z[f] if f in z.files else None, k, rtol=1e-6, atol=1e-14)
    print(f"; {k} iterations compared, worst relative deviation of a history entry {worst:.2e}")
    if full:
        assert_solution(lib.solution, z["solution"])
    # the two drivers take the same decisions from the same scalars: bit-identical
    assert py.iteration_count == lib.iteration_count and py.backtracks == lib.backtracks
    for f in FIELDS:
        if getattr(lib, f) is not None:
            assert np.array_equal(getattr(py, f), getattr(lib, f), equal_nan=True), f
    assert np.array_equal(py.solution, lib.solution)


@pytest.mark.parametrize("name", ["lasso_200x400_adaptive", "lasso_200x400_accelerated", "logistic_150x240_adaptive", "nnls_300x150", "skewed_257x515"])
def test_two_runs_are_bitwise_equal_and_a_raw_matrix_is_the_map(name):
    meta, z, d = load(name)
    a, b = solve(meta, d), solve(meta, d)
    S = capture_script().matrix_of(d)
    loss, reg = tags(meta["kind"], d)
    np.random.seed(meta["solver_seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        raw = fa.fasta(S.tocoo(), S.T, loss.f, loss.gradf, reg.g, reg.prox, np.zeros(S.shape[1]), verbose=False, **H.resolve_options(meta["options"], fstop))
    for other in (b, raw):
        assert other.iteration_count == a.iteration_count and other.backtracks == a.backtracks
        for f in FIELDS:
            assert np.array_equal(getattr(other, f), getattr(a, f), equal_nan=True), f
        assert np.array_equal(other.solution, a.solution)
    assert raw.library_steps == raw.iteration_count


@pytest.mark.parametrize("name", ["lasso_200x400_adaptive", "lasso_200x400_accelerated", "lasso_200x400_plain", "logistic_150x240_adaptive",
                                  "nnls_300x150", "box_300x150", "skewed_257x515"])
def test_the_densified_matrix_agrees(name):
    """The same matrix as a DenseMatrixMap on the two-launch path: equal counts, the first 40 iterations of every history at rtol 1e-6."""
    meta, z, d = load(name)
    S = capture_script().matrix_of(d)
    sparse = solve(meta, d)
    dense_op = fa.DenseMatrixMap(S.toarray())
    try:
        dense = solve(meta, d, op=dense_op, fused=False)
    finally:
        dense_op.close()
    print(f"\n{name}: sparse {sparse.iteration_count} / {sparse.backtracks}, dense {dense.iteration_count} / {dense.backtracks}")
    assert sparse.iteration_count == dense.iteration_count and sparse.backtracks == dense.backtracks
    k = min(40, sparse.iteration_count)
    G.compare_histories(sparse, lambda f: getattr(dense, f), k, rtol=1e-6, atol=1e-14)


@pytest.mark.parametrize("name", ["lasso_200x400_adaptive", "lasso_200x400_accelerated"])
def test_device_driver_falls_to_the_library_loop(name):
    meta, z, d = load(name)
    want = solve(meta, d, driver="library")
    for extra in (dict(driver="device"), dict(device_iters=7)):
        c = solve(meta, d, **extra)
        assert c.device_steps == 0 and c.library_steps == c.iteration_count == want.iteration_count
        assert np.array_equal(c.stepsizes, want.stepsizes) and np.array_equal(c.solution, want.solution)


@pytest.mark.parametrize("mode", ["adaptive", "accelerated"])
def test_whole_solve_on_a_matrix_with_a_dense_row_and_a_dense_column(mode):
    """LASSO on the long_both matrix (whole-workgroup rows on both copies) against the host loop over the same closures."""
    S = long_both() * 0.05
    rng = np.random.RandomState(61)
    x = np.zeros(S.shape[1])
    x[rng.permutation(S.shape[1])[:20]] = rng.randn(20)
    b = S @ x + 0.01 * rng.randn(S.shape[0])
    ls, reg = fa.LeastSquares(b), fa.Shrink(0.05)
    runs = []
    for backend in ("numpy", "hip"):
        np.random.seed(62)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            runs.append(fa.fasta(S, ls.f, ls.gradf, reg.g, reg.prox, np.zeros(S.shape[1]), backend=backend, verbose=False, max_iters=60, tolerance=1e-5,
                                 evaluate_objective=True, adaptive=mode == "adaptive", accelerate=mode == "accelerated"))
    host, dev = runs
    print(f"\nlong_both {mode}: device {dev.iteration_count} / {dev.backtracks}, host {host.iteration_count} / {host.backtracks}", end="")
    assert dev.iteration_count == host.iteration_count and dev.backtracks == host.backtracks
    worst = G.compare_histories(dev, lambda f: getattr(host, f), dev.iteration_count, rtol=1e-6, atol=1e-14)
    print(f"; worst relative deviation of a history entry {worst:.2e}")
    assert_solution(dev.solution, host.solution)


def test_the_example_prints_the_same_iteration_counts_on_both_backends(capsys):
    from fasta_python_amd.examples import test_modes
    from fasta_python_amd.examples.sparse_design import SparseDesignProblem
    for logistic in (False, True):
        counts = {}
        for backend in ("numpy", "hip"):
            problem, x0 = SparseDesignProblem.construct(M=600, N=1200, density=0.02, logistic=logistic, backend=backend)
            np.random.seed(1)
            counts[backend] = [c.iteration_count for _, c in test_modes(problem, x0)]
            problem.close()
        assert counts["hip"] == counts["numpy"], (logistic, counts)
    assert capsys.readouterr().out.count("Completed in") == 12          # print_info, once per mode and solve


def test_spectral_norm_squared():
    S = random_sparse(400, 300, 0.05, 23)
    op = fa.SparseMatrixMap(S)
    try:
        lam = op.spectral_norm_squared(iters=300, rtol=1e-12, seed=1)
    finally:
        op.close()
    true = np.linalg.norm(S.toarray(), 2) ** 2              # a Rayleigh quotient of A^T A: never above, and after 300 iterations close below
    assert 0.98 * true <= lam <= true * (1 + 1e-9)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def status_of(call):
    with pytest.raises(hip.HipError) as e:
        call()
    assert len(str(e.value)) > 20                             # a sentence, not just a code
    return int(str(e.value).split("]")[0][1:])


def test_what_the_sparse_operator_does_not_serve_is_refused_with_its_code():
    S = random_sparse(64, 96, 0.1, 31)
    op = fa.SparseMatrixMap(S)
    try:
        c = op.ctx
        c.set_loss_lsq(np.ones(64))
        c.set_prox(hip.PROX_SHRINK, 0.1)
        c.set_vector(hip.VEC_X0, np.zeros(96))
        c.init()
        assert c.fused_supported() == 0 and c.fused_agree() == 0 and not c.run_supported() and c.rhs == 0
        assert status_of(lambda: c.step(0.1)) == hip.E_STATE
        assert status_of(lambda: c.step_begin(0.1)) == hip.E_STATE
        assert status_of(lambda: c.step_accel(0.1, 0.5, True)) == hip.E_STATE
        assert status_of(lambda: c.run(4, hip.RunOpts(window=10, stepsize_shrink=0.5), hip.RunState(tau_next=0.1, alpha1=1.0))) == hip.E_STATE
        assert status_of(lambda: c.set_rhs(2)) == hip.E_STATE
        assert status_of(lambda: c.comm_init(1, 0, bytes(hip.UNIQUE_ID_BYTES))) == hip.E_STATE
        assert status_of(lambda: c.get_matrix_rows(0, 1)) == hip.E_STATE
        assert status_of(lambda: c.stream_read_ms()) == hip.E_STATE
        for kind in (hip.PROX_LINF, hip.PROX_L1BALL, hip.PROX_TVBALL, hip.PROX_GROUP):
            assert status_of(lambda: c.set_prox(kind, 0.1)) == hip.E_ARG
        c.fwd(0.1)                                                # ... and the context still works
    finally:
        op.close()
    data, indices, indptr = S.data, S.indices, S.indptr
    with hip.HipContext(0, storage="f32") as c32:
        assert status_of(lambda: c32.set_matrix_csr(indptr, indices, data, S.shape)) == hip.E_STATE
    with hip.HipContext(devices=[0, 0]) as shell:
        assert status_of(lambda: shell.set_matrix_csr(indptr, indices, data, S.shape)) == hip.E_STATE
    with hip.HipContext(0) as c:
        # not canonical: the first offending row is named
        bad = indices.copy()
        lo = int(indptr[5])
        assert indptr[6] - lo >= 2
        bad[lo], bad[lo + 1] = bad[lo + 1], bad[lo]
        with pytest.raises(hip.HipError, match="row 5"):
            c.set_matrix_csr(indptr, bad, data, S.shape)
        bad = indices.copy()
        bad[int(indptr[9])] = 96
        with pytest.raises(hip.HipError, match="row 9"):
            c.set_matrix_csr(indptr, bad, data, S.shape)
        ptr = indptr.copy()
        ptr[3] = ptr[4] + 1
        with pytest.raises(hip.HipError, match="row"):
            c.set_matrix_csr(ptr, indices, data, S.shape)
        assert c.nnz() == 0
        c.set_matrix(np.eye(4))
        assert c.nnz() == 0
        c.set_matrix_csr(indptr, indices, data, S.shape)          # a dense context becomes a sparse one and back
        assert c.nnz() == S.nnz and c.shape() == S.shape
        np.testing.assert_allclose(c.apply(np.ones(96)), S @ np.ones(96), rtol=1e-12, atol=1e-13)
        c.set_matrix(np.eye(4))
        assert c.nnz() == 0 and np.array_equal(c.apply(np.arange(4.0)), np.arange(4.0))


# ---- a size beyond any dense matrix ------------------------------------------------------------------------------------------------------------
def banded_random(n, per_row, seed):
    """n x n, `per_row` entries per row from a seeded generator: one column out of each of `per_row` equal stretches of the row."""
    rng = np.random.RandomState(seed)
    stretch = n // per_row
    cols = (rng.randint(0, stretch, size=(n, per_row)) + np.arange(per_row) * stretch).astype(np.int32)
    data = rng.standard_normal(n * per_row) / np.sqrt(per_row)
    return sp.csr_matrix((data, cols.ravel(), np.arange(n + 1, dtype=np.int64) * per_row), shape=(n, n))


def test_lasso_on_a_million_squared():
    """1 048 576^2 with 16 entries per row (8 TB as a dense matrix): the first 5 iterations against SciPy on the host."""
    n = 1 << 20
    S = banded_random(n, 16, 41)
    rng = np.random.RandomState(42)
    x = np.zeros(n)
    x[rng.permutation(n)[:1000]] = rng.randn(1000)
    b = S @ x + 0.01 * rng.randn(n)
    ls, reg = fa.LeastSquares(b), fa.Shrink(0.05)
    runs = []
    for backend in ("numpy", "hip"):
        np.random.seed(43)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            runs.append(fa.fasta(S, ls.f, ls.gradf, reg.g, reg.prox, np.zeros(n), backend=backend, verbose=False, max_iters=5, tolerance=0.0,
                                 evaluate_objective=True))
    host, dev = runs
    assert dev.iteration_count == host.iteration_count == 5 and dev.backtracks == host.backtracks
    worst = G.compare_histories(dev, lambda f: getattr(host, f), 5, rtol=1e-6, atol=1e-14)
    print(f"\n1048576^2, 16 per row: worst relative deviation of a history entry over 5 iterations {worst:.2e}")
    assert_solution(dev.solution, host.solution)
