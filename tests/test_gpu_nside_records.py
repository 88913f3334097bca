"""GPU tests of the shared n-side sums and record finaliser (csrc/fh_nside.h) through every operator form that ends a launch with
finish_records: sparse, sparse multi-column, dense multi-column, quadratic, bilinear, 3-D stencil, DCT (one-row and tiled), convolution
(image and flat signal) and the identity operator.

Per form one shape per GRID CLASS of each record array -- the finaliser can only go wrong at those boundaries:
  one    1 workgroup / record;
  few    2 .. 256: one trip of the `i += 256` loop of the last workgroup, with idle lanes;
  many   more than 256: a second trip.
The grid of every case is asserted through the form's shape call (or, where the library has none for it, through the stated rule).  Classes a
form cannot reach in a case of a few seconds are left out, with the reason, in CASES below.

Per case: one fwd and one adj (mode 0; adj without and with acceleration), then
  * every returned scalar against float64 NumPy ON THE HOST COPIES of the device's vectors: |device - numpy| <= 2 n 2^-52 sum|t_i|, n the
    number of terms t_i of that sum -- the rigorous bound for two summations of the same terms in any order (each at most (n - 1) u sum|t_i|
    off the exact sum, u = 2^-53, and the one rounding of a term inside an fma against NumPy's rounded product is covered by the factor 2);
  * FH_S_GMAX / FH_S_GMAX_ADJ exactly; FH_S_ALPHA == 0 and no timeout word;
  * a second identical call returns the same bits: records are added in index order.
The terms are formed on the host with the kernels' own two-rounding expressions (fasta/__init__.py:181-270), so they are the device's terms
bit for bit.  ONE exception, the bilinear form's f = .5 ||S - X Y^T||^2: its terms contain a K-term dot product whose order differs between
the device and NumPy, so each residual e_ij is only known to d_ij = (K + 2) u (|S_ij| + sum_k |X_ik| |Y_jk|) on either side, each term to
2 |e_ij| (2 d_ij) + (2 d_ij)^2, and the sum of those allowances is added to the bound above (bilinear_f)."""
import numpy as np
import pytest

from fasta_python_amd import hip

pytestmark = pytest.mark.gpu

TAU0, TAU, COEF, MU = 0.7, 0.4, 0.37, 0.2
U = 2.0 ** -53


def bound(terms):
    return 2.0 * terms.size * 2.0 ** -52 * float(np.abs(terms).sum())


def held(name, got, terms, extra=0.0):
    ref, lim = float(np.sum(terms)), bound(terms) + extra
    print(f"    {name:9s} device {got!r} numpy {ref!r} |diff| {abs(got - ref):.3e} bound {lim:.3e} ({terms.size} terms)")
    assert abs(got - ref) <= lim, name


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ---- the forms: build(cls) -> (context, n-side length, m-side length, kind of f, extras); every builder asserts its grids ------------------------
def csr(m, n, rng):
    """three entries per row, sorted distinct columns: mean row length 3 on both sides' rule (G = 4 lanes per row, 64 rows per workgroup)"""
    r = np.arange(m)[:, None]
    cols = np.sort((r * 7 + np.array([0, 5, 11])[None, :]) % n, axis=1)
    assert np.all(np.diff(cols, axis=1) > 0)
    return np.arange(m + 1, dtype=np.int64) * 3, cols.ravel().astype(np.int32), rng.randn(m * 3)


SPARSE_SHAPES = {"one": (48, 48), "few": (1000, 1500), "many": (16500, 66000)}      # rows / 64 workgroups per side; n / 256 prologue records


def sparse_grids(c, m, n, cls):
    """sp_upload_side's rule: nwg = min(ceil(rows / (256 / G)), 8 per CU), no long rows here"""
    cap = 8 * c.cu_count()[0]
    for side, rows in ((0, m), (1, n)):
        G, nwg, nlong = c.sparse_lanes(side)
        assert (G, nlong) == (4, 0) and nwg == min(-(-rows // 64), cap)
    fwd, adj, pro = c.sparse_lanes(0)[1], c.sparse_lanes(1)[1], -(-n // 256)
    want = {"one": lambda g: g == 1, "few": lambda g: 2 <= g <= 256, "many": lambda g: g > 256}[cls]
    assert want(fwd) and want(adj) and want(pro), (fwd, adj, pro)


def build_sparse(cls, rng, L=0):
    m, n = SPARSE_SHAPES[cls]
    c = hip.HipContext(0)
    indptr, indices, data = csr(m, n, rng)
    c.set_matrix_csr(indptr, indices, data, (m, n), rhs=L or None)
    sparse_grids(c, m, n, cls)
    k = L or 1
    c.set_loss_lsq(rng.randn(m * k))
    return c, n * k, m * k, "lsq", {}


def build_spmulti(cls, rng):
    return build_sparse(cls, rng, L=3)                       # LB = 4: two column lanes per row of X, G = 4 still (2 entries per trip >= mean / 2)


# dense multi-column: fwd_grid records of K-fwd, npro of the prologue, ncc of K-adj's column chunks, nslab loss sums
MULTI_SHAPES = {"one": ((16, 32, 2), dict(fwd_grid=1, npro=1, ncc=1, nslab=1)),
                "few": ((200, 1500, 3), dict(fwd_grid=13, npro=6, ncc=2, nslab=7)),
                "many_fwd": ((4128, 32, 2), dict(fwd_grid=258, npro=1, ncc=1, nslab=104)),       # (both at once would be a 8.7 GB matrix)
                "many_adj": ((16, 263168, 2), dict(fwd_grid=1, npro=1028, ncc=257, nslab=1))}


def build_multi(cls, rng):
    (m, n, L), grids = MULTI_SHAPES[cls]
    c = hip.HipContext(0)
    c.set_matrix(rng.randn(m, n))
    c.set_rhs(L)
    sh = c.multi_shape()
    assert {k: getattr(sh, k) for k in grids} == grids, sh
    c.set_loss_lsq(rng.randn(m * L))
    return c, n * L, m * L, "lsq", {}


# quadratic: fwd_grid of k_qd_fwd, npro of the prologue, ngrad of k_qd_grad.  ngrad > 256 needs n > 65536, a 34 GB Q: left out.
QUAD_SHAPES = {"one": ((16, 2), dict(fwd_grid=1, npro=1, ngrad=1)),
               "few": ((600, 3), dict(fwd_grid=38, npro=3, ngrad=3)),
               "many": ((4200, 2), dict(fwd_grid=263, npro=17, ngrad=17))}


def build_quad(cls, rng):
    (n, L), grids = QUAD_SHAPES[cls]
    c = hip.HipContext(0)
    A = rng.randn(n, n)
    cvec = rng.randn(n * L)
    c.set_quadratic(A + A.T, cvec, L)
    sh = c.quad_shape()
    assert {k: getattr(sh, k) for k in grids} == grids, sh
    return c, n * L, n * L, "quad", {"c": cvec}


# bilinear: grid of k_bl_pass, nelem of k_bl_prologue / k_bl_grad
BILINEAR_SHAPES = {"one": ((16, 30, 2), dict(grid=1, nelem=1)),
                   "few": ((300, 200, 3), dict(grid=19, nelem=2)),
                   "many": ((65600, 16, 2), dict(grid=456, nelem=257))}


def build_bilinear(cls, rng):
    (m, n, K), grids = BILINEAR_SHAPES[cls]
    c = hip.HipContext(0)
    S = rng.randn(m, n)
    c.set_factorization(S, K)
    sh = c.bilinear_shape()
    assert {k: getattr(sh, k) for k in grids} == grids, sh
    return c, (m + n) * K, 0, "bilinear", {"S": S, "m": m, "K": K}


TV3_SHAPES = {"one": ((2, 4, 5), 1), "few": ((6, 20, 40), 3), "many": ((72, 128, 128), 288)}


def build_tv3d(cls, rng):
    (D, H, W), grid = TV3_SHAPES[cls]
    c = hip.HipContext(0)
    c.set_stencil3d(D, H, W)
    assert c.tv3d_shape().grid == grid
    c.set_loss_lsq(rng.randn(D * H * W))
    return c, 3 * D * H * W, D * H * W, "lsq", {}


# DCT: the one-row form is ONE workgroup whatever N (no other class exists); the tiled form finalises over `tiles` workgroups, and its one-tile
# class needs FH_TUNE_DCT_ROW_CAP lowered (N > 2048 has 34 tiles at least)
DCT_SHAPES = {"row_one": ((60, 0), dict(levels=1, grid1=1)),
              "tiled_one": ((720, 32), dict(levels=2, tiles=1)),
              "tiled_few": ((4000, 0), dict(levels=2, tiles=63)),
              "tiled_many": ((360000, 0), dict(levels=2, tiles=378))}


def build_dct(cls, rng):
    (N, cap), grids = DCT_SHAPES[cls]
    c = hip.HipContext(0)
    if cap:
        c.set_tuning(hip.TUNE_DCT_ROW_CAP, cap)
    c.set_dct(N, rng.rand(N) + 0.5)
    sh = c.dct_shape()
    assert {k: getattr(sh, k) for k in grids} == grids, sh
    c.set_loss_lsq(rng.randn(N))
    return c, N, N, "lsq", {}


CONV_SHAPES = {"image_one": ((8, 9), (3, 3), 1), "image_few": ((40, 70), (3, 5), 4), "image_many": ((544, 1024), (3, 3), 272),
               "signal_one": ((1, 200), (1, 5), 1), "signal_few": ((1, 3000), (1, 5), 2), "signal_many": ((1, 2048 * 257), (1, 5), 257)}


def build_conv(cls, rng):
    shape, kshape, grid = CONV_SHAPES[cls]
    c = hip.HipContext(0)
    c.set_conv2d(shape, rng.randn(*kshape))
    assert c.conv_shape().grid == grid
    n = shape[0] * shape[1]
    c.set_loss_lsq(rng.randn(n))
    return c, n, n, "lsq", {}


IDENTITY_SHAPES = {"one": (9, 7), "few": (40, 50), "many": (300, 300)}


def build_identity(cls, rng):
    """both launches: min(ceil(M N / 256), 2048) workgroups (launch_id_fwd / launch_id_adj; the library has no shape call for them)"""
    M, N = IDENTITY_SHAPES[cls]
    c = hip.HipContext(0)
    c.set_identity(M, N)
    n = M * N
    assert c.shape() == (n, n)
    grid = min(-(-n // 256), 2048)
    assert {"one": grid == 1, "few": 2 <= grid <= 256, "many": grid > 256}[cls]
    c.set_loss_lsq(rng.randn(n))
    return c, n, n, "identity", {}


FORMS = [("sparse", build_sparse, SPARSE_SHAPES), ("spmulti", build_spmulti, SPARSE_SHAPES), ("multi", build_multi, MULTI_SHAPES),
         ("quad", build_quad, QUAD_SHAPES), ("bilinear", build_bilinear, BILINEAR_SHAPES), ("tv3d", build_tv3d, TV3_SHAPES),
         ("dct", build_dct, DCT_SHAPES), ("conv", build_conv, CONV_SHAPES), ("identity", build_identity, IDENTITY_SHAPES)]
CASES = [(name, build, cls) for name, build, shapes in FORMS for cls in shapes]


# ---- f of a form from the host copies -----------------------------------------------------------------------------------------------------------
def extrap(v, vprev, coef):
    return v + coef * (v - vprev)                            # :242-243, two roundings after the difference


def bilinear_f(S, m, K, x):
    """(terms of sum (S - X Y^T)^2, the allowance for the dot products' order) -- f is half their sum"""
    Z = x.reshape(-1, K)
    X, Y = Z[:m], Z[m:]
    E = S - X @ Y.T
    d = (K + 2) * U * (np.abs(S) + np.abs(X) @ np.abs(Y).T)
    return (E * E).ravel(), float(np.sum(2.0 * np.abs(E) * (2.0 * d) + (2.0 * d) ** 2))


def f_terms(kind, ex, b, z, x, halve=False):
    """terms of FH_S_FSQ (or _ADJ) at the m-side point z / the n-side point x, and the scale and allowance that go with them"""
    if kind == "lsq":
        return (z - b) ** 2, 1.0, 0.0
    if kind == "identity":
        return (x - b) ** 2, 1.0, 0.0
    if kind == "quad":
        return x * ((0.5 * z) + ex["c"]), 1.0, 0.0             # qd_term: three roundings
    t, allow = bilinear_f(ex["S"], ex["m"], ex["K"], x)
    return t, 0.5, allow


@pytest.mark.parametrize("name,build,cls", CASES, ids=[f"{n}-{k}" for n, _, k in CASES])
def test_every_scalar_of_one_fwd_and_adj(name, build, cls):
    rng = np.random.RandomState(1000 + sum(map(ord, name + cls)))
    c, nlen, mlen, kind, ex = build(cls, rng)
    V = lambda which, ln: c.get_vector(which, ln)
    try:
        c.set_prox(hip.PROX_SHRINK, MU)
        # one accelerated iteration first: its commit makes this iteration's xprox and z the acceleration history (x_accel0, z_accel0),
        # a pair of vectors the host has read (a plain iteration leaves x_accel0 where fh_init armed it)
        c.set_vector(hip.VEC_X0, rng.randn(nlen))
        c.init()
        c.fwd(TAU0)
        c.adj(TAU0, accel=True, coef=COEF)
        xacc, zacc = V(hip.VEC_XPROX, nlen), (V(hip.VEC_Z, mlen) if mlen else None)
        c.commit()
        x0, g0 = rng.randn(nlen), rng.randn(nlen)
        c.set_vector(hip.VEC_X0, x0)
        c.set_vector(hip.VEC_G0, g0)
        b = V(hip.VEC_B, mlen) if kind in ("lsq", "identity") else None

        # ---- K-fwd
        s = c.fwd(TAU)
        xhat, xp, z = V(hip.VEC_XHAT, nlen), V(hip.VEC_XPROX, nlen), (V(hip.VEC_Z, mlen) if mlen else None)
        assert same_bits(xhat, x0 - TAU * g0)                                              # :181
        print(f"{name}-{cls}: fwd")
        dx = xp - x0
        t, scale, allow = f_terms(kind, ex, b, z, xp)
        held("FSQ", s[hip.S_FSQ] / scale, t, allow)
        held("DXG0", s[hip.S_DXG0], dx * g0)
        held("DX2", s[hip.S_DX2], dx * dx)
        held("XH2", s[hip.S_XH2], (xp - xhat) ** 2)
        held("G02", s[hip.S_G02], g0 * g0)
        held("GSUM", s[hip.S_GSUM], np.abs(xp))
        held("RDOT", s[hip.S_RDOT], (x0 - xp) * (xp - xacc))                                # :231
        assert s[hip.S_GMAX] == np.abs(xp).max() and s[hip.S_ALPHA] == 0.0 and s[15] == 0.0
        assert same_bits(c.fwd(TAU)[:8], s[:8])

        # ---- K-adj, without and with acceleration
        for accel in (False, True):
            s = c.adj(TAU, accel=accel, coef=COEF)
            g1, x1 = V(hip.VEC_G1, nlen), V(hip.VEC_X1, nlen)
            assert same_bits(x1, extrap(xp, xacc, COEF) if accel else xp)                  # :242
            print(f"{name}-{cls}: adj accel={accel}")
            dg = g1 + (xhat - x0) / TAU                                                     # :254
            zx = None if z is None else (extrap(z, zacc, COEF) if accel else z)
            t, scale, allow = f_terms(kind, ex, b, zx, x1)
            held("FSQ_ADJ", s[hip.S_FSQ_ADJ] / scale, t, allow)
            held("DXDG", s[hip.S_DXDG], dx * dg)
            held("DG2", s[hip.S_DG2], dg * dg)
            held("XH2_ADJ", s[hip.S_XH2_ADJ], (x1 - xhat) ** 2)
            held("GSUM_ADJ", s[hip.S_GSUM_ADJ], np.abs(x1))
            assert s[hip.S_GMAX_ADJ] == np.abs(x1).max() and s[15] == 0.0
            assert same_bits(c.adj(TAU, accel=accel, coef=COEF)[8:14], s[8:14])
    finally:
        c.close()
