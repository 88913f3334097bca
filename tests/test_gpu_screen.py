"""GPU tests of gap-safe screening on the device (fh_column_norms, fh_screen, fh_gather_columns: csrc/fh_screen.h) against the host statement
(fasta_python_amd/certificates.py: screen).  Shapes, dyadic data, the exact evaluation and the path problems: tests/screen_cases.py.

Bounds.  Dyadic data: the norms, the certificate and therefore the whole test are exact or chains of single correctly rounded operations spelled alike
on both sides -- every comparison is `==`.  At x0 = 0 the host statement is formed from the host's A; at an iterate reached by the device's steps the
host forms the test from the device's own certificate, g0 and norms (screen_from_parts): the host's A x0 differs from the device's in the last bits,
which tests/test_gpu_gap.py bounds and which is not what is under test here.  Seeded non-dyadic norms: (m + 2) eps norms2_j, the bound of a chain of
m fused multiply-adds (slab partials added in slab order shorten the chain, never lengthen it).  A gathered context against one that received
A[:, idx] through fh_set_matrix: bit for bit, rows, vectors and scalars -- a padding column that was not zero would show in every scalar.  The path:
the bounds of tests/test_screen_cpu.py."""
import math
import warnings

import numpy as np
import pytest

import fasta_python_amd as fa
from fasta_python_amd import certificates as ce
from fasta_python_amd import hip, stopping
from tests import screen_cases as S

pytestmark = pytest.mark.gpu

VECS = ("VEC_X0", "VEC_G0", "VEC_XHAT", "VEC_XPROX", "VEC_X1", "VEC_G1", "VEC_BEST", "VEC_B", "VEC_Z", "VEC_T0", "VEC_T1", "VEC_T2", "VEC_T3")
EPS = 2.0 ** -52


def snapshot(c, n_len, m_len):
    return {v: c.get_vector(getattr(hip, v), m_len if v in ("VEC_B", "VEC_Z") else n_len) for v in VECS}


def at_init(c, loss, reg, x):
    loss.bind(c)
    c.set_prox(reg.kind, reg.mu, 0.0, 0.0)
    c.set_vector(hip.VEC_X0, x)
    c.init()
    return c


def aux_launches(c):
    return c.timing_get(hip.K_AUX)[1]


def sparse_twin(A, seed):
    from scipy import sparse as sp
    return sp.csr_matrix(A * (np.random.RandomState(seed).rand(*A.shape) < 0.3))


def forms_of(A, L):
    """(name, make an operator) for the dense operator in both storages and the sparse one (where its dense host twin stays small)."""
    rhs = None if L == 1 else L
    out = [("f64", A, lambda: fa.DenseMatrixMap(A, rhs=rhs)), ("f32", A, lambda: fa.DenseMatrixMap(A, storage="f32"))]
    if A.size <= 1 << 18:
        Sp = sparse_twin(A, L)
        out.append(("csr", Sp.toarray(), lambda: fa.SparseMatrixMap(Sp, rhs=rhs)))
    return out


# ---- the norms ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", S.SHAPES, ids=S.IDS)
def test_column_norms_on_dyadic_data_are_the_hosts_bit_for_bit(shape):
    m, n, L = shape
    A, _, _ = S.dyadic_problem(m, n, L, seed=m + 3 * n + L)
    B = np.roll(A, 1, axis=1) * 0.5 if n > 1 else A * 0.5
    for name, host, make in forms_of(A, L):
        op = make()
        try:
            c = op.ctx
            c.timing_enable()
            c.timing_reset()
            got = c.column_norms()
            first = aux_launches(c)
            np.testing.assert_array_equal(got, ce.column_norms2(host), err_msg=name)
            np.testing.assert_array_equal(c.column_norms(), got)                     # two calls: bit-identical
            assert first >= 1 and aux_launches(c) == first, name                     # ... and the second launches nothing
            if name != "csr":                                                        # a second matrix: the norms are the new matrix's
                c.set_matrix(B)
                np.testing.assert_array_equal(c.column_norms(), ce.column_norms2(B), err_msg=name)
                assert aux_launches(c) > first
        finally:
            op.close()


@pytest.mark.parametrize("m,n", [(17, 257), (257, 17), (1000, 65), (3, 65537), (65537, 3)])
def test_column_norms_of_seeded_data_are_within_the_fma_chains_bound(m, n):
    rng = np.random.RandomState(m + n)
    A = rng.randn(m, n)
    for name, host, make in forms_of(A, 1):
        if name == "f32":
            host = A.astype(np.float32).astype(np.float64)
        op = make()
        try:
            got = op.ctx.column_norms()
            want = np.array([math.fsum(v * v for v in host[:, j]) for j in range(n)])
            err = np.abs(got - want)
            print(name, m, n, "largest error / bound", float(np.max(err / np.maximum((m + 2) * EPS * want, 1e-300))))
            assert np.all(err <= (m + 2) * EPS * want), name
            if name == "csr":                                                        # after a second sparse matrix the norms are the new one's
                S2 = sparse_twin(2.0 * A, 7)
                op.ctx.set_matrix_csr(S2.indptr, S2.indices, S2.data, S2.shape)
                got2, want2 = op.ctx.column_norms(), ce.column_norms2(S2)
                assert np.all(np.abs(got2 - want2) <= (m + 2) * EPS * want2) and (n < 8 or np.any(got2 != got))
        finally:
            op.close()


def test_a_long_sparse_column_takes_the_workgroup_path():
    from scipy import sparse as sp
    rng = np.random.RandomState(4)
    A = (rng.randint(-8, 9, size=(5000, 40)) / 8.0) * (rng.rand(5000, 40) < 0.01)
    A[:, 7] = rng.randint(-8, 9, size=5000) / 8.0                                    # one dense column among short ones
    op = fa.SparseMatrixMap(sp.csr_matrix(A))
    try:
        assert op.ctx.sparse_lanes(1)[2] >= 1
        np.testing.assert_array_equal(op.ctx.column_norms(), ce.column_norms2(A))
    finally:
        op.close()


# ---- the test ----------------------------------------------------------------------------------------------------------------------------------
def assert_screen_equals(c, want_keep, want_rho, want_gap_safe, mu, tag):
    keep, report = c.screen()
    np.testing.assert_array_equal(keep, want_keep, err_msg=str(tag))
    assert (report[0], report[1], report[2], report[3]) == (want_rho, float(np.count_nonzero(want_keep)), want_gap_safe, mu), (tag, report)
    return keep


@pytest.mark.parametrize("shape", S.SHAPES, ids=S.IDS)
def test_the_mask_at_zero_on_dyadic_data_is_the_host_statements(shape):
    m, n, L = shape
    A, b, _ = S.dyadic_problem(m, n, L, seed=m + 3 * n + L)
    cols = () if L == 1 else (L,)
    x = np.zeros((n,) + cols)
    discarded = kept = 0
    for name, host, make in forms_of(A, L):
        if name == "f32" and L > 1:
            continue
        op = make()
        try:
            c = op.ctx
            loss = fa.LeastSquares(b)
            dn = at_init(c, loss, fa.Shrink(1.0), x).dual_gap().dual_norm
            if dn == 0.0:
                continue
            for prox_class in ((fa.Shrink, fa.GroupShrink) if L > 1 else (fa.Shrink,)):
                dn = ce.critical_mu(host, loss, prox_class, x.shape)
                for mu in (dn * 63 / 64, dn * 3 / 4, dn, 2.0 * dn, dn / 16):
                    reg = prox_class(mu)
                    at_init(c, loss, reg, x)
                    want = ce.screen(host, loss, reg, x)
                    keep = assert_screen_equals(c, want.keep, want.radius, ce.gap_safe(want.certificate, ce.screen_kappa(m, n, L)), mu, (name, mu))
                    assert tuple(c.dual_gap()) == tuple(want.certificate)
                    discarded += int(np.count_nonzero(~keep))
                    kept += int(np.count_nonzero(keep))
        finally:
            op.close()
    assert kept > 0 and (discarded > 0 or n == 1)


@pytest.mark.parametrize("driver", ["library", "device", "python"])
@pytest.mark.parametrize("group", [False, True], ids=["shrink", "group"])
def test_the_mask_after_plain_iterations_under_each_driver(driver, group):
    m, n, L = 65, 257, (3 if group else 1)
    A, b, _ = S.dyadic_problem(m, n, L, seed=11)
    A = A / 4.0
    cols = () if L == 1 else (L,)
    loss = fa.LeastSquares(b)
    prox_class = fa.GroupShrink if group else fa.Shrink
    reg = prox_class(0.5 * ce.critical_mu(A, loss, prox_class, (n,) + cols))
    kappa = ce.screen_kappa(m, n, L)
    op = fa.DenseMatrixMap(A, rhs=None if L == 1 else L)
    try:
        c = op.ctx
        np.random.seed(1)
        solver = fa.FBSolver(op, loss, reg, np.zeros((n,) + cols), verbose=False, max_iters=10, tolerance=0.0, stop_rule=stopping.residual,
                             adaptive=False, driver=driver).setup()
        norms2 = c.column_norms()
        np.testing.assert_array_equal(norms2, ce.column_norms2(A))
        masks = []
        for steps in (1, 9):
            solver.advance(steps)
            before, scal, cert = snapshot(c, n * L, m * L), c.last_scalars(), c.dual_gap()
            g0 = before["VEC_G0"].reshape((n,) + cols)
            want_keep, want_rho = ce.screen_from_parts(cert, g0, norms2, reg, kappa)
            masks.append(assert_screen_equals(c, want_keep, want_rho, ce.gap_safe(cert, kappa), reg.mu, (driver, steps)))
            after = snapshot(c, n * L, m * L)
            for v in VECS:                                                           # vectors, scalars and a following dual_gap(): unchanged
                np.testing.assert_array_equal(before[v], after[v], err_msg=v)
            np.testing.assert_array_equal(c.last_scalars(), scal)
            assert c.dual_gap() == cert
            # safety against the host's solution of the same problem is the CPU suite's; here: the support of the iterate's prox image stays
            assert want_rho > 0
        assert solver.i == 10
    finally:
        op.close()


# ---- the gather --------------------------------------------------------------------------------------------------------------------------------
def keep_sets(n, seed):
    rng = np.random.RandomState(seed)
    sets = {"one": [n // 2], "15": range(1, 16), "16": range(0, 16), "17": range(2, 19), "all-but-one": [j for j in range(n) if j != 3],
            "all": range(n), "every-second": range(0, n, 2), "seeded": np.flatnonzero(rng.rand(n) < 0.3)}
    return {k: np.asarray(list(v), dtype=np.int32) for k, v in sets.items()}


def one_step(c, loss, reg, x, tau):
    """vectors and scalars of fh_init + fh_step, then of an fh_fwd + fh_adj pair, on a context that holds its matrix"""
    out = []
    at_init(c, loss, reg, x)
    if c.fused_supported():                             # (the same answer on both contexts: it depends on the shape alone)
        out.append(c.step(tau))
        c.commit()
    out.append(c.fwd(tau))
    out.append(c.adj(tau))
    c.commit()
    n, m = x.size, loss.b.size
    return out, snapshot(c, n, m)


@pytest.mark.parametrize("storage,m,n", [("f64", 17, 257), ("f64", 257, 65), ("f32", 65, 1000), ("f64", 1, 33), ("f32", 1000, 40)])
def test_gathered_columns_are_the_matrix_a_setter_would_have_given(storage, m, n):
    rng = np.random.RandomState(m + n)
    A = rng.randint(-8, 9, size=(m, n)) / 8.0 + (rng.randint(-8, 9, size=(m, n)) / 1024.0 if storage == "f64" else 0.0)
    b = rng.randn(m)
    loss = fa.LeastSquares(b)
    src = fa.DenseMatrixMap(A, storage=storage)
    dst = hip.HipContext(0, storage=storage)
    ref = hip.HipContext(0, storage=storage)
    try:
        s = src.ctx
        reg_src = fa.Shrink(0.25)
        at_init(s, loss, reg_src, np.zeros(n))
        rows_before, cert_before, norms_before = s.get_matrix_rows(0, m), s.dual_gap(), s.column_norms()
        for name, idx in keep_sets(n, m).items():
            dst.gather_columns(s, idx)
            assert dst.shape() == (m, idx.size) and dst.rhs == 0
            np.testing.assert_array_equal(dst.get_matrix_rows(0, m), A[:, idx], err_msg=name)
            np.testing.assert_array_equal(dst.column_norms(), ce.column_norms2(A[:, idx]), err_msg=name)
            ref.set_matrix(np.ascontiguousarray(A[:, idx]))
            x = rng.randn(idx.size) * (rng.rand(idx.size) < 0.5)
            reg = fa.Shrink(0.05)
            tau = 0.5 / max(np.linalg.norm(A[:, idx], 2) ** 2, 1e-3)
            got_scal, got_vec = one_step(dst, loss, reg, x, tau)
            want_scal, want_vec = one_step(ref, loss, reg, x, tau)
            for g, w in zip(got_scal, want_scal):
                np.testing.assert_array_equal(g, w, err_msg=name)
            for v in VECS:
                np.testing.assert_array_equal(got_vec[v], want_vec[v], err_msg=name + " " + v)
            np.testing.assert_array_equal(s.get_matrix_rows(0, m), rows_before)      # the source: rows, certificate and norms as before
            assert s.dual_gap() == cert_before
            np.testing.assert_array_equal(s.column_norms(), norms_before)
        dst.gather_columns(s, np.arange(n, dtype=np.int32))
        dst.set_rhs(2) if storage == "f64" else None                                 # like any context: a column count, then another operator
        assert dst.rhs == (2 if storage == "f64" else 0) and dst.shape() == (m, n)
        dst.set_stencil(4, 5)
        assert dst.shape() == (20, 40)
    finally:
        src.close()
        dst.close()
        ref.close()


def test_a_multi_column_source_gives_the_same_matrix():
    rng = np.random.RandomState(2)
    A = rng.randn(33, 70)
    src = fa.DenseMatrixMap(A, rhs=3)
    dst = hip.HipContext(0)
    try:
        idx = np.arange(5, 70, 3, dtype=np.int32)
        dst.set_matrix(rng.randn(8, 8))
        dst.set_rhs(4)
        dst.set_prox(hip.PROX_GROUP, 0.5)
        dst.gather_columns(src.ctx, idx)                                             # comes out in vector form, as after a dense setter
        assert dst.rhs == 0 and dst.shape() == (33, idx.size) and src.ctx.rhs == 3
        np.testing.assert_array_equal(dst.get_matrix_rows(0, 33), A[:, idx])
    finally:
        src.close()
        dst.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def refused(call, status, sentence):
    with pytest.raises(hip.HipError) as err:
        call()
    assert str(err.value) == "[%d] %s" % (status, sentence), str(err.value)


SERVED = "(served: the dense and the sparse operator, vector and multi-column)"
IN_FLIGHT = "a step issued by fh_step_begin is still in flight on this context: call fh_step_end first"


def unserved_forms():
    rng = np.random.RandomState(1)
    B = rng.randn(4, 5)
    Q = rng.randn(5, 5)
    quad = fa.Quadratic(Q + Q.T)
    fz = fa.Factorization(np.abs(rng.randn(3, 4)))
    mask = (rng.rand(16) < 0.6).astype(float)
    return [("identity operator", fa.IdentityMap((4, 5)), fa.LeastSquares(B), np.zeros((4, 5)), False),
            ("stencil operator", fa.GradDivMap((4, 5)), fa.LeastSquares(B), np.zeros((4, 5, 2)), False),
            ("3-D stencil operator", fa.GradDivMap((2, 4, 5)), fa.LeastSquares(rng.randn(2, 4, 5)), np.zeros((2, 4, 5, 3)), False),
            ("quadratic operator", fa.QuadraticMap(quad, (5,)), quad, np.zeros(5), False),
            ("bilinear operator", fa.BilinearMap(fz, (7, 2)), fz, np.ones((7, 2)), False),
            ("DCT operator", fa.DCTMap(16, mask=mask), fa.LeastSquares(rng.randn(16)), np.zeros(16), True),
            ("convolution operator", fa.ConvMap((8, 8), rng.randn(3, 3)), fa.LeastSquares(rng.randn(8, 8)), np.zeros((8, 8)), True)]


def test_every_unserved_form_is_refused_by_name():
    for noun, op, loss, x0, certifies in unserved_forms():
        try:
            c = op.ctx
            if certifies:
                loss.bind(c)
                c.set_prox(hip.PROX_SHRINK, 0.5)
                c.set_vector(hip.VEC_X0, x0)
                c.init()
            refused(c.column_norms, hip.E_STATE, "fh_column_norms: the %s stores no columns %s" % (noun, SERVED))
            if certifies:                      # the certificate is served, the columns are not
                assert c.dual_gap().gap >= 0
                refused(c.screen, hip.E_STATE, "fh_screen: the %s stores no columns %s" % (noun, SERVED))
            else:
                refused(c.screen, hip.E_ARG, "fh_screen: the %s has no duality-gap certificate (served: the dense and the sparse operator, vector and "
                        "multi-column, the DCT and the convolution operator)" % noun)
        finally:
            op.close()
    with hip.HipContext(0) as c:
        refused(c.column_norms, hip.E_STATE, "fh_column_norms: no operator set")
        refused(c.screen, hip.E_ARG, "fh_screen: the operator has no duality-gap certificate (served: the dense and the sparse operator, vector and "
                "multi-column, the DCT and the convolution operator)")


def test_the_states_fh_screen_and_fh_column_norms_refuse():
    rng = np.random.RandomState(1)
    A, b = rng.randn(6, 10), rng.randn(6)
    ls = fa.LeastSquares(b)
    op = fa.DenseMatrixMap(A)
    try:
        c = op.ctx
        refused(c.screen, hip.E_ARG, "fh_screen: no loss set (fh_set_loss_lsq / fh_set_loss_logistic)")
        ls.bind(c)
        c.set_prox(hip.PROX_SHRINK, 0.5)
        refused(c.screen, hip.E_ARG, "fh_screen: no committed state: call fh_init or fh_setup first (after the operator, the loss and x0 are set)")
        c.set_vector(hip.VEC_X0, np.zeros(10))
        c.init()
        assert c.screen()[0].shape == (10,)
        for kind in (hip.PROX_IDENTITY, hip.PROX_NONNEG, hip.PROX_BOX):
            c.set_prox(kind, 0.5, -1.0, 1.0)
            refused(c.screen, hip.E_ARG, "fh_screen: the certificate is implemented for FH_PROX_SHRINK and FH_PROX_GROUP (the context holds prox kind %d)" % kind)
        for mu in (0.0, -1.0):
            c.set_prox(hip.PROX_SHRINK, mu)
            refused(c.screen, hip.E_ARG, "fh_screen: the certificate needs mu > 0 (the context holds mu = %g)" % mu)
        c.set_prox(hip.PROX_SHRINK, 0.5)
        c.step_begin(1e-3)
        refused(c.screen, hip.E_ARG, "fh_screen: " + IN_FLIGHT)
        refused(c.column_norms, hip.E_STATE, "fh_column_norms: " + IN_FLIGHT)
        c.step_end()
        c.commit()
        assert c.screen()[0].shape == (10,)
        c.fwd(1e-3)
        c.adj(1e-3, accel=True, coef=0.3)
        c.commit()
        refused(c.screen, hip.E_ARG, "fh_screen: the latest step was accelerated: x0 is the extrapolated iterate and A x0 is formed inside the adjoint "
                "launch, never stored (Z holds A xprox): the certificate is served after fh_init, fh_setup and steps without acceleration")
        assert c.column_norms().shape == (10,)                                      # the norms ask for no committed state
        fa.LogisticLoss(np.where(b > 0, 1.0, -1.0)).bind(c)
        c.init()
        assert c.dual_gap().gap >= 0
        refused(c.screen, hip.E_ARG, "fh_screen: the screening radius is stated for the least-squares loss (the constant of the logistic loss differs)")
    finally:
        op.close()
    idm = fa.IdentityMap((2, 3))
    try:
        c = idm.ctx
        fa.LeastSquares(np.ones((2, 3)), weights=np.ones((2, 3))).bind(c)
        c.set_prox(hip.PROX_SHRINK, 0.5)
        c.set_vector(hip.VEC_X0, np.zeros((2, 3)))
        c.init()
        refused(c.screen, hip.E_ARG, "fh_screen: a context that holds observation weights has no duality-gap certificate")
    finally:
        idm.close()
    shell = fa.ShardedDenseMatrixMap(A, devices=(0, 0))
    try:
        c = shell.ctx
        ls.bind(c)
        c.set_prox(hip.PROX_SHRINK, 0.5)
        c.set_vector(hip.VEC_X0, np.zeros(10))
        c.init()
        refused(c.screen, hip.E_ARG, "fh_screen: a multi-device context or a context with a communicator holds a row block of z = A x0, not z: the "
                "certificate is served on a plain context")
        refused(c.column_norms, hip.E_STATE, "fh_column_norms: a multi-device context holds row blocks of A, not its columns: the norms are served on a plain context")
        with hip.HipContext(0) as dst:
            refused(lambda: dst.gather_columns(c, np.arange(3)), hip.E_STATE,
                    "fh_gather_columns: the source is a multi-device context: columns are gathered between plain contexts")
        with hip.HipContext(0) as src:
            src.set_matrix(A)
            refused(lambda: c.gather_columns(src, np.arange(3)), hip.E_STATE,
                    "fh_gather_columns: the destination is a multi-device context: columns are gathered between plain contexts")
    finally:
        shell.close()


def test_a_context_with_a_communicator_is_refused():
    A = np.random.RandomState(1).randn(6, 10)
    with hip.HipContext(0) as c, hip.HipContext(0) as other:
        c.set_matrix(A)
        other.set_matrix(A)
        c.comm_init(1, 0, hip.comm_unique_id())
        fa.LeastSquares(np.ones(6)).bind(c)
        c.set_prox(hip.PROX_SHRINK, 0.5)
        c.set_vector(hip.VEC_X0, np.zeros(10))
        c.init()
        refused(c.column_norms, hip.E_STATE, "fh_column_norms: a context with a communicator (row-sharded run) holds a row block of A, not its columns")
        refused(c.screen, hip.E_ARG, "fh_screen: a multi-device context or a context with a communicator holds a row block of z = A x0, not z: the "
                "certificate is served on a plain context")
        refused(lambda: other.gather_columns(c, np.arange(3)), hip.E_STATE,
                "fh_gather_columns: the source holds a communicator (row-sharded run): columns are gathered between plain contexts")
        refused(lambda: c.gather_columns(other, np.arange(3)), hip.E_STATE,
                "fh_gather_columns: the destination holds a communicator (row-sharded run): columns are gathered between plain contexts")
        c.comm_destroy()


def test_what_fh_gather_columns_refuses():
    rng = np.random.RandomState(1)
    A = rng.randn(6, 10)
    g = lambda d, s, idx: (lambda: d.gather_columns(s, np.asarray(idx, dtype=np.int32)))
    with hip.HipContext(0) as src, hip.HipContext(0) as dst, hip.HipContext(0, storage="f32") as narrow:
        refused(g(dst, src, [0, 1]), hip.E_STATE, "fh_gather_columns: the source holds no dense matrix (fh_set_matrix / fh_generate_matrix)")
        src.set_matrix(A)
        refused(g(src, src, [0, 1]), hip.E_ARG, "fh_gather_columns: the destination is the source: the kept columns go into a second context")
        refused(g(dst, src, []), hip.E_ARG, "fh_gather_columns: every feature is screened: the solution is zero")
        refused(g(dst, src, [3, 2]), hip.E_ARG, "fh_gather_columns: the column indices are not strictly increasing at position 1")
        refused(g(dst, src, [1, 4, 4]), hip.E_ARG, "fh_gather_columns: the column indices are not strictly increasing at position 2")
        refused(g(dst, src, [0, 10]), hip.E_ARG, "fh_gather_columns: column index 10 at position 1 is out of range (n = 10)")
        refused(g(dst, src, [-1, 2]), hip.E_ARG, "fh_gather_columns: column index -1 at position 0 is out of range (n = 10)")
        refused(g(dst, src, range(11)), hip.E_ARG, "fh_gather_columns: 11 columns asked of a matrix that has 10")
        refused(g(narrow, src, [0, 1]), hip.E_ARG, "fh_gather_columns: the destination stores A in float32, the source in float64: the copy does not convert")
        narrow.set_matrix(A)
        refused(g(dst, narrow, [0, 1]), hip.E_ARG, "fh_gather_columns: the destination stores A in float64, the source in float32: the copy does not convert")
        with pytest.raises(hip.HipError, match="no operator set"):                    # nothing of it reached the destination
            dst.shape()
        fa.LeastSquares(np.ones(6)).bind(src)
        src.set_prox(hip.PROX_SHRINK, 0.5)
        src.set_vector(hip.VEC_X0, np.zeros(10))
        src.init()
        src.step_begin(1e-3)
        refused(g(dst, src, [0, 1]), hip.E_STATE, "fh_gather_columns: on the source, " + IN_FLIGHT)
        src.step_end()
        dst.set_matrix(A)
        fa.LeastSquares(np.ones(6)).bind(dst)
        dst.set_vector(hip.VEC_X0, np.zeros(10))
        dst.init()
        dst.step_begin(1e-3)
        refused(g(dst, src, [0, 1]), hip.E_STATE, "fh_gather_columns: on the destination, " + IN_FLIGHT)
        dst.step_end()
        dst.set_identity(2, 3)
        fa.LeastSquares(np.ones((2, 3)), weights=np.ones((2, 3))).bind(dst)
        refused(g(dst, src, [0, 1]), hip.E_STATE, "fh_gather_columns: the destination holds observation weights (fh_set_loss_weights): remove them "
                "before an operator is set")
        dst.set_loss_weights(None)
        dst.gather_columns(src, np.array([0, 9], dtype=np.int32))
        assert dst.shape() == (6, 2)
    if hip.device_count() > 1:
        with hip.HipContext(0) as src, hip.HipContext(1) as far:
            src.set_matrix(A)
            refused(g(far, src, [0, 1]), hip.E_ARG, "fh_gather_columns: the destination lives on device 1, the source on device 0: the copy stays on one device")


# ---- the path ----------------------------------------------------------------------------------------------------------------------------------
def run_path(A, loss, prox_class, x0=None, **kw):
    np.random.seed(2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fa.path(A, loss, prox_class, x0=x0, **S.PATH_OPTS, **kw)


def mmv_problem():
    rng = np.random.RandomState(21)
    A = rng.randn(48, 160) / 7.0
    X = np.zeros((160, 3))
    X[rng.permutation(160)[:5]] = rng.randn(5, 3)
    return A, A @ X + 0.01 * rng.randn(48, 3)


@pytest.mark.parametrize("name", ["sparse_ls_64x128", "dense64x128", "csr40x60", "mmv48x160x3"])
def test_the_screened_path_on_the_device(name):
    if name.startswith("mmv"):
        A, b = mmv_problem()
        prox_class, x0 = fa.GroupShrink, np.zeros((160, 3))
    else:
        A, b = S.path_problems()[name]
        prox_class, x0 = fa.Shrink, None
    loss = fa.LeastSquares(b)
    got = run_path(A, loss, prox_class, x0, backend="hip", screen=True)
    host = run_path(A, loss, prox_class, x0, backend="numpy", screen=True)
    tol, f0, n = S.PATH_OPTS["gap_tolerance"], 0.5 * float(np.sum(b * b)), A.shape[1]
    assert len(got) == len(host) == S.PATH_OPTS["n_mus"]
    np.testing.assert_allclose([p.mu for p in got], [p.mu for p in host], rtol=1e-13)
    for p, q in zip(got, host):
        full = ce.duality_gap(A, loss, prox_class(p.mu), p.solution)
        print(name, "mu %.3e kept %d / %d rounds %d iterations %d (host: kept %d rounds %d iterations %d) gap/f0 %.2e" %
              (p.mu, p.kept, n, p.rounds, p.iteration_count, q.kept, q.rounds, q.iteration_count, full.gap / f0))
        assert p.solution.shape == q.solution.shape and abs(p.certificate.f0 - f0) <= 1e-12 * f0
        assert p.certificate.gap <= tol * f0 and full.gap <= tol * f0               # the full problem's certificate, on the device and from the host
        rows = lambda x: np.any(np.reshape(x, (n, -1)) != 0, axis=1)
        np.testing.assert_array_equal(rows(p.solution), rows(q.solution))
        assert np.linalg.norm(A @ p.solution - A @ q.solution) <= 2.0 * math.sqrt(2.0 * tol * f0)
        assert p.kept >= np.count_nonzero(rows(p.solution)) and 0 <= p.rounds <= 8
    assert any(p.kept < n for p in got)


@pytest.mark.parametrize("name", ["dense64x128", "csr40x60"])
def test_without_screening_the_path_is_the_plain_loop_of_solves(name):
    A, b = S.path_problems()[name]
    loss = fa.LeastSquares(b)
    got = run_path(A, loss, fa.Shrink, backend="hip")
    from scipy import sparse as sp
    op = fa.SparseMatrixMap(A) if sp.issparse(A) else fa.DenseMatrixMap(A)
    try:
        np.random.seed(2)
        x, L, tau0 = np.zeros(A.shape[1]), None, None
        rule = stopping.DualityGap(S.PATH_OPTS["gap_tolerance"], 10)
        for p in got:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                solver = fa.FBSolver(op, loss, fa.Shrink(p.mu), x, L=L, tau0=tau0, stop_rule=rule, verbose=False, max_iters=S.PATH_OPTS["max_iters"]).setup()
                L, tau0 = solver.L, solver.tau0
                want = solver.run()
            x = np.array(want.solution)
            assert p.iteration_count == want.iteration_count and tuple(p.certificate) == tuple(want.certificate) and p.gaps == want.gaps
            np.testing.assert_array_equal(p.solution, want.solution)
            np.testing.assert_array_equal(p.residuals, want.residuals)
            np.testing.assert_array_equal(p.stepsizes, want.stepsizes)
            assert not hasattr(p, "kept")
    finally:
        op.close()


def test_the_example_prints_the_columns_kept(capsys):
    from fasta_python_amd.examples import lasso_path
    out = lasso_path.main(["--backend", "hip", "--rows", "40", "--features", "80", "--screen"])
    text = capsys.readouterr().out
    assert "kept" in text and "rounds" in text
    pts = out["adaptive"]
    assert len(pts) == 10 and all(hasattr(p, "kept") for p in pts) and any(p.kept < 80 for p in pts)
    assert all(p.certificate.relative <= 1e-6 or p.iteration_count >= 5000 for p in pts)
