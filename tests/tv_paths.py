"""Cases, geometry and the exact model for the tests of EVERY instantiation of the 2-D stencil kernels (csrc/fh_tv.h): the one-pass sweep
k_tv_onepass<IDENT, ACCEL, U, NT, NB> (fh_step / fh_step_accel) and the two-launch family k_fwd_tv_step<IDENT, U, NT> / k_adj_tv_step<U, NT> /
k_fwd_tv<4, NT> / k_adj_tv<4, NT> (fh_fwd, fh_adj, fh_init, fh_apply).  A plain helper module, the sibling of tests/mc_paths.py and
tests/sparse_lanes.py: the CPU tier (tests/test_tv_paths_cpu.py) checks every condition claimed here, the GPU tier
(tests/test_gpu_tv_paths.py) runs the kernels.

The model (`fbs_step`) is one iteration of the reference's loop (oracle/fasta_np.py: the forward-backward step, the FISTA extrapolation with its
restart rule, the Barzilai-Borwein sums; oracle/problems.py: div, grad; fo.tv_dual_ball), written from that loop and not from the kernels,
generic over the number type: float64, np.longdouble and scaled integers (`Fx`: an integer mantissa and a binary exponent, exact).

Exactness.  The operands are dyadic: x0 holds integers of [-2, 2], b integers of [-3, 3], tau, c_prev and coef are powers of two.  With no prox
the step is linear, so every product, extrapolation and sum of the two steps of a chain is a dyadic rational below 2^53 units of its grid
(the widest, sum dG^2 of the second step, at or below 2^52; the CPU tier asserts it): float64 cannot round whatever the order of summation and
with or without fused multiply-adds, so a kernel's result must EQUAL the model's.  A third step would push that sum past 2^53: the chains stay
two steps deep.  The lagged state (P1, P0, c_prev) is made the only way the C ABI allows: one committed accelerated step from fh_init
(UPHILL, tau = -1/8, coef = 1/2).  From there tau = 1/64 gives a positive restart dot and tau = 1/16 a negative one on every image, so both
branches of the restart rule and all three arms of the finaliser's `plain` predicate (restart and dot > 1e-30; coef == 0; neither) are reached.

With the TV-ball prox (a square root and two divisions per pixel) nothing is exact.  Vectors are compared with the model evaluated in float64
in NumPy's own order of roundings (which the project already pins bit for bit: tests/test_gpu_prox_tv.py), sums against the same float64
terms added up in np.longdouble, within (terms + 4) * 2^-53 * sum|term|: the worst case of a float64 sum of that many terms in any order, with
or without fused products.  At the at most 150 000 terms of these images that is below 2e-11 of sum|term|, and a single dropped pixel moves a
sum by about 1 / terms = 7e-6 of it.  The operands are scaled by 1/4 (x0) and 3/2 (b), and the second step of a chain that is to KEEP its
coefficient goes uphill once more (tau = -1/64; the downhill tau = 1/16 of the no-prox chain would pull 97 % of the pixels back inside), so
that between 20 % and 80 % of the pixels of every launch lie outside the unit ball: both arms of max(||y||, 1) run.  Images of fewer than
64 pixels draw their operands from a seed searched for that (SMALL_SEEDS); the image of ONE pixel has no such fraction and is exempt.  At
these scales the restart dot of the TV-ball `restarts` / `no-restart` launches (tau = 1/64) is POSITIVE on every image of 64 pixels or more
and that of the `keeps` / `coef-zero` launches is not, so both branches of the restart rule run with the TV-ball prox too (the CPU tier
asserts it)."""
import collections
import functools
import itertools

import numpy as np

from fasta_python_amd import hip

# restated once; tests/test_tv_paths_cpu.py reads csrc/fh_tv.h and csrc/fh_device.h as text and asserts the #defines still carry these values
TVZ_OWN = 60                 # owned columns per wave of k_tv_onepass (two halo lanes per side)
TVS_FWD_OWN = 62             # ... of k_fwd_tv_step
TVS_ADJ_OWN = 63             # ... of k_adj_tv_step
TV_SW = 64                   # ... of the plain pair k_fwd_tv / k_adj_tv
FH_WG = 256
WAVES = FH_WG // 64          # wave strips per workgroup (a strip group)
RESTART_EPS = 1e-30          # fasta/__init__.py:231

IDENTITY, TVBALL = "identity", "tvball"
PROX_KIND = {IDENTITY: hip.PROX_IDENTITY, TVBALL: hip.PROX_TVBALL}
ALL_U, ALL_PIPE, ALL_NT = (2, 4, 8), (1, 3), (0, 3)                # FH_TUNE_TV_U, _PIPE, _NT of the one-pass sweep (0 = auto: also run)
TWO_U, TWO_NT = (2, 4, 8), (0, 1)                                   # FH_TUNE_TV_U, _NT of the two-launch family
FWD_SCALARS = ("S_FSQ", "S_DXG0", "S_DX2", "S_XH2", "S_G02", "S_GSUM", "S_GMAX", "S_RDOT")
ADJ_SCALARS = ("S_DXDG", "S_DG2", "S_FSQ_ADJ", "S_XH2_ADJ", "S_GSUM_ADJ", "S_GMAX_ADJ")
SCALARS = FWD_SCALARS + ADJ_SCALARS
MAXIMA = ("S_GMAX", "S_GMAX_ADJ")


# ---- which kernel a tuning reaches: the host's rule (csrc/fh_host_launch.h: launch_tv_onepass, launch_fwd_tv, launch_adj_tv) restated ----------
def onepass_instantiation(prox, accel, U=0, pipe=0, nt=0):
    """(IDENT, ACCEL, U, NT, NB) of k_tv_onepass.  No prox: the burst form with plain accesses whatever PIPE and NT say."""
    u = U or (4 if accel else 2)
    if prox == IDENTITY:
        return (1, int(accel), u, 0, 1)
    return (0, int(accel), u, 0 if nt == 3 else 2, 3 if (pipe or (3 if accel else 1)) >= 2 else 1)


ONEPASS_ALL = frozenset(onepass_instantiation(p, a, U, pipe, nt) for p in (TVBALL, IDENTITY) for a in (0, 1)
                        for U in ALL_U for pipe in ALL_PIPE for nt in ALL_NT)


def two_launch_instantiations(prox, U=0, nt=0):
    """The step kernels fh_fwd + fh_adj launch under a tuning: U = 8 unless the key says 2 or 4, NT = 1 only for the key's value 1."""
    u, n = (U if U in (2, 4) else 8), int(nt == 1)
    return {("k_fwd_tv_step", int(prox == IDENTITY), u, n), ("k_adj_tv_step", u, n)}


def plain_pair_instantiations(nt=0):
    return {("k_fwd_tv", 4, int(nt == 1)), ("k_adj_tv", 4, int(nt == 1))}


TWO_LAUNCH_ALL = frozenset(itertools.chain.from_iterable(
    list(two_launch_instantiations(p, U, nt)) + list(plain_pair_instantiations(nt)) for p in (TVBALL, IDENTITY) for U in TWO_U for nt in TWO_NT))


def tunings(prox):
    """Every (U, PIPE, NT) the one-pass sweep distinguishes for this prox: 12 with the TV-ball prox, the 3 trip lengths without."""
    if prox == IDENTITY:
        return [(U, 1, 0) for U in ALL_U]
    return list(itertools.product(ALL_U, ALL_PIPE, ALL_NT))


# ---- geometry ----------------------------------------------------------------------------------------------------------------------------------
Shape = collections.namedtuple("Shape", "strips strip_groups chunks last_rows grid")


def ceil_div(a, b):
    return -(-a // b)


def sweep_shape(H, W, rows, own=TVZ_OWN):
    """Strips, strip groups, row chunks, rows of the last chunk and workgroups of a sweep whose waves own `own` columns, `rows` rows per chunk."""
    strips = ceil_div(W, own)
    sg = ceil_div(strips, WAVES)
    chunks = ceil_div(H, rows)
    return Shape(strips, sg, chunks, H - (chunks - 1) * rows, sg * chunks)


def trips(chunk_rows, U):
    """(total rows a chunk of k_tv_onepass walks, trips of U rows, passes of the NB = 3 loop of three trips each)."""
    total = chunk_rows + 4
    return total, ceil_div(total, U), ceil_div(total, 3 * U)


def auto_rows(H, W, accel, ncu=256):
    """The automatic chunk height of launch_tv_onepass, restated (the two default-rule cases leave FH_TUNE_TV_ROWS alone)."""
    pixels = H * W
    min_rows = 8 if pixels <= 1 << 18 else (8 if pixels <= 1 << 20 and not accel else 32)
    chunks = max(1, ncu * 5 // sweep_shape(H, W, 1).strip_groups)
    return min(H, max(min_rows, ceil_div(H, chunks)))


def xcd_order(b, grid, on):
    """tv_xcd_order of csrc/fh_tv.h: the logical id of workgroup b."""
    per = grid // 8
    if not on or b >= per * 8:
        return b
    return (b % 8) * per + b // 8


# A geometry: the image, FH_TUNE_TV_ROWS (0 = the automatic rule), the trip length its claim is about (0: every U alike), the values of
# FH_TUNE_TV_XCD it runs under, and what it claims as a dict that the CPU tier recomputes from (H, W, rows, U).
Geometry = collections.namedtuple("Geometry", "name H W rows U xcd claim")


def _g(name, H, W, rows, U=0, xcd=(0,), **claim):
    return Geometry(name, H, W, rows, U, xcd, claim)


GEOMETRIES = (
    # degenerate wraps: tv_wrap_row wrapping twice (H = 1, 2), % W with W < 4
    _g("wrap 1x1", 1, 1, 1, grid=1, total=5),
    _g("wrap 1x5", 1, 5, 1, grid=1, total=5),
    _g("wrap 2x3", 2, 3, 2, grid=1, total=6),
    _g("wrap 3x1", 3, 1, 2, grid=2, last_rows=1),
    # strip seams of the 60-column wave strips: one strip exactly, then one column into the next wave; one column short of it
    _g("strip 59", 6, 59, 4, strips=1, grid=2),
    _g("strip 60", 6, 60, 4, strips=1, grid=2),
    _g("strip 61", 6, 61, 4, strips=2, grid=2),
    # strip-group seams: four waves exactly, then a second strip group
    _g("group 240", 6, 240, 4, strips=4, strip_groups=1, grid=2),
    _g("group 241", 6, 241, 4, strips=5, strip_groups=2, grid=4),
    # the two-launch kernels' own strip widths (62, 63, 64 columns; four of them, then one more column)
    _g("two-launch 62", 5, 62, 3, strips=2),
    _g("two-launch 63", 5, 63, 3, strips=2),
    _g("two-launch 64", 5, 64, 3, strips=2),
    _g("two-launch 65", 5, 65, 3, strips=2),
    _g("two-launch 248", 5, 248, 3, strip_groups=2),
    _g("two-launch 249", 5, 249, 3, strip_groups=2),
    _g("two-launch 252", 5, 252, 3, strip_groups=2),
    _g("two-launch 253", 5, 253, 3, strip_groups=2),
    _g("two-launch 256", 5, 256, 3, strip_groups=2),
    _g("two-launch 257", 5, 257, 3, strip_groups=2),
    # a chunk shorter than a trip: a one-row last chunk, total = 5 < U = 8
    _g("short chunk", 9, 33, 8, U=8, chunks=2, last_rows=1, last_total=5, last_trips=1),
    # chunk rows that are no multiple of U: total = 7 at U = 4
    _g("ragged trips", 9, 33, 3, U=4, chunks=3, last_rows=3, total=7, trips=2),
    # the NB = 3 rotation, per U: total < 3 U (one loop pass), total = 3 U exactly, 3 U < total < 6 U with total % U != 0
    _g("rotation U2 one pass", 2, 33, 1, U=2, total=5, passes=1),
    _g("rotation U2 exact", 4, 33, 2, U=2, total=6, passes=1),
    _g("rotation U2 two passes", 10, 33, 5, U=2, total=9, passes=2),
    _g("rotation U4 one pass", 10, 33, 5, U=4, total=9, passes=1),
    _g("rotation U4 exact", 16, 33, 8, U=4, total=12, passes=1),
    _g("rotation U4 two passes", 26, 33, 13, U=4, total=17, passes=2),
    _g("rotation U8 one pass", 26, 33, 13, U=8, total=17, passes=1),
    _g("rotation U8 exact", 40, 33, 20, U=8, total=24, passes=1),
    _g("rotation U8 two passes", 54, 33, 27, U=8, total=31, passes=2),
    # FH_TUNE_TV_ROWS taller than the image: one chunk
    _g("rows above H", 5, 64, 64, chunks=1, last_rows=5, grid=1),
    # one chunk per row: 300 workgroups, so the finaliser's `i += FH_WG` loop makes a second pass
    _g("finaliser second pass", 300, 61, 1, grid=300, finaliser_passes=2),
    # XCD dealing on / off on a ragged grid: 600 workgroups across two strip groups (600 % 8 == 0, per = 75)
    _g("xcd 600", 300, 250, 1, xcd=(0, 2), grid=600, strip_groups=2, per=75),
    # ... and on grids of 5 (per = 0: no workgroup is dealt), 8 (all dealt) and 13 (the last 5 keep their ids)
    _g("xcd 5", 5, 33, 1, xcd=(0, 2), grid=5, per=0, kept=5),
    _g("xcd 8", 8, 33, 1, xcd=(0, 2), grid=8, per=1, kept=0),
    _g("xcd 13", 13, 33, 1, xcd=(0, 2), grid=13, per=1, kept=5),
    # the automatic chunk rule, tuning untouched
    _g("auto 40x257", 40, 257, 0, auto_rows=8),
    _g("auto 130x121", 130, 121, 0, auto_rows=8),
    # several chunks (8, the last of 2 rows) and two strip groups: the geometry of the same-bits test
    _g("bits 37x250", 37, 250, 5, xcd=(0, 2), chunks=8, last_rows=2, strip_groups=2, grid=16),
)
GEOMETRY = {g.name: g for g in GEOMETRIES}
BITS_GEOMETRY = "bits 37x250"
BACK_TO_BACK = "finaliser second pass"


def geometry_id(g):
    return g.name.replace(" ", "_")


def claims_of(g, ncu=256):
    """Everything a geometry may claim, recomputed from (H, W, rows, U)."""
    rows = g.rows or auto_rows(g.H, g.W, False, ncu)
    sh = sweep_shape(g.H, g.W, rows)
    U = g.U or 2
    full = min(rows, g.H)
    total, ntrips, passes = trips(full, U)
    last_total, last_trips, _ = trips(sh.last_rows, U)
    per = sh.grid // 8
    return dict(strips=sh.strips, strip_groups=sh.strip_groups, chunks=sh.chunks, last_rows=sh.last_rows, grid=sh.grid, total=total, trips=ntrips,
                passes=passes, last_total=last_total, last_trips=last_trips, finaliser_passes=ceil_div(sh.grid, FH_WG), per=per,
                kept=sh.grid - 8 * per, auto_rows=rows)


# ---- the states a launch starts from -------------------------------------------------------------------------------------------------------------
# name -> (accelerated, lagged: one committed accelerated step first, tau, coef, restart)
FIRST_TAU, FIRST_COEF = -0.125, 0.5                      # the committed first step of a lagged chain: uphill
State = collections.namedtuple("State", "name accel lagged tau tv_tau coef restart")       # tv_tau: the step size with the TV-ball prox
STATES = (
    State("plain", 0, 0, 0.125, 0.125, 0.0, 0),                  # fh_step from fh_init
    State("first", 1, 0, FIRST_TAU, FIRST_TAU, FIRST_COEF, 1),   # fh_step_accel from fh_init: c_prev = 0 (the sweep skips P0), dot = -||dx||^2 <= 0
    State("restarts", 1, 1, 1.0 / 64, 1.0 / 64, 0.5, 1),         # a small downhill step against the uphill momentum: dot > 0, restart taken
    State("keeps", 1, 1, 1.0 / 16, -1.0 / 64, 0.5, 1),           # a larger one (TV-ball: uphill again): dot <= 0, coef applied
    State("no-restart", 1, 1, 1.0 / 64, 1.0 / 64, 0.5, 0),       # dot > 0 but restart = 0: coef applied
    State("coef-zero", 1, 1, 1.0 / 16, -1.0 / 64, 0.0, 1),       # dot <= 0 and coef = 0: the plain set through the third arm of the predicate
)


def tau_of(state, prox):
    return state.tv_tau if prox == TVBALL else state.tau
STATE = {s.name: s for s in STATES}


def state_id(s):
    return s.name


# ---- exact scaled integers ---------------------------------------------------------------------------------------------------------------------
class Fx:
    """m * 2^-e with an int64 array (or a Python int) m: the arithmetic of the model, exact."""
    __slots__ = ("m", "e")

    def __init__(self, m, e=0):
        self.m, self.e = m, int(e)

    @staticmethod
    def of(v):
        """A dyadic float (array or scalar), exactly."""
        a = np.asarray(v, dtype=np.float64)
        e = 0
        while not np.array_equal(np.ldexp(a, e), np.rint(np.ldexp(a, e))):
            e += 1
            assert e < 60
        m = np.ldexp(a, e).astype(np.int64)
        return Fx(m if m.ndim else int(m), e)

    def _at(self, e):
        return self.m * (1 << (e - self.e)) if e > self.e else self.m

    def _pair(self, o):
        e = max(self.e, o.e)
        return self._at(e), o._at(e), e

    def __add__(self, o):
        a, b, e = self._pair(o)
        return Fx(a + b, e)

    def __sub__(self, o):
        a, b, e = self._pair(o)
        return Fx(a - b, e)

    def __mul__(self, o):
        return Fx(self.m * o.m, self.e + o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        assert isinstance(o.m, int) and abs(o.m) == 1                  # by a power of two only
        return Fx(self.m * o.m, self.e - o.e) if self.e >= o.e else Fx(self.m * o.m * (1 << (o.e - self.e)), 0)

    def __abs__(self):
        return Fx(np.abs(self.m), self.e)

    def roll(self, shift, axis):
        return Fx(np.roll(self.m, shift, axis), self.e)

    def sum(self):
        return Fx(int(self.m.sum()), self.e)

    def max(self):
        return Fx(int(self.m.max()), self.e)

    @property
    def size(self):
        return self.m.size

    def to_float(self):
        m = np.asarray(self.m)
        assert np.all(np.abs(m) < 1 << 53)
        out = np.ldexp(m.astype(np.float64), -self.e)
        return out if out.ndim else float(out)


class Number:
    """A number system of the model: how operands enter, in which type sums are accumulated, how results leave."""

    def __init__(self, name, enter, wide, leave):
        self.name, self.enter, self.wide, self.leave = name, enter, wide, leave


F64 = Number("float64", lambda v: np.asarray(v, dtype=np.float64), lambda v: v, lambda v: v)
LONGDOUBLE = Number("longdouble", lambda v: np.asarray(v, dtype=np.longdouble), lambda v: v, lambda v: v)
INTEGER = Number("integer", Fx.of, lambda v: v, lambda v: v)
# float64 elements in NumPy's own order of roundings, sums (and the products under them) in np.longdouble: the reference of a TV-ball launch
F64_WIDE_SUMS = Number("float64, longdouble sums", F64.enter, lambda v: np.asarray(v, dtype=np.longdouble), lambda v: v)

Sum = collections.namedtuple("Sum", "value terms mag")                 # a scalar of the block: its value, how many terms, sum of |term|


def _roll(a, shift, axis):
    return a.roll(shift, axis) if isinstance(a, Fx) else np.roll(a, shift, axis)


def _sqrt(a):
    return np.sqrt(a)


def grad(X):
    """examples/tv_denoising.py:26-40: the two components roll(X, +1, axis d) - X."""
    return (_roll(X, 1, 0) - X, _roll(X, 1, 1) - X)


def div(Y):
    """examples/tv_denoising.py:43-63: sum_d roll(Y_d, -1, axis d) - Y_d."""
    return (_roll(Y[0], -1, 0) - Y[0]) + (_roll(Y[1], -1, 1) - Y[1])


def tv_dual_ball(Y):
    """examples/tv_denoising.py:89-96: Y / max(||Y||_2, 1) per pixel."""
    mags = _sqrt(Y[0] * Y[0] + Y[1] * Y[1])
    mags = np.maximum(mags, 1)
    return (Y[0] / mags, Y[1] / mags)


def _field(ns, Y):
    """(H, W, 2) -> the pair of its components in the number system."""
    Y = np.asarray(Y)
    return (ns.enter(Y[..., 0]), ns.enter(Y[..., 1]))


def _dot(ns, A, B):
    """sum over both components of a * b, with the number of terms and the sum of their magnitudes."""
    prods = [ns.wide(a) * ns.wide(b) for a, b in zip(A, B)]
    value = prods[0].sum() + prods[1].sum() if len(prods) == 2 else prods[0].sum()
    mag = abs(prods[0]).sum() + abs(prods[1]).sum() if len(prods) == 2 else abs(prods[0]).sum()
    return Sum(value, sum(p.size for p in prods), mag)


def _l1(ns, A):
    mags = [abs(ns.wide(a)) for a in A]
    s = mags[0].sum() + mags[1].sum()
    return Sum(s, mags[0].size * 2, s)


def _linf(A):
    m0, m1 = abs(A[0]).max(), abs(A[1]).max()
    if isinstance(m0, Fx):
        a, b, e = m0._pair(m1)
        return Sum(Fx(max(a, b), e), 0, None)
    return Sum(max(m0, m1), 0, None)


def _sub(A, B):
    return tuple(a - b for a, b in zip(A, B))


def _extrapolate(V, Vprev, c):
    """fasta/__init__.py:242-243: v + c * (v - v_prev), in that order."""
    if isinstance(V, tuple):
        return tuple(_extrapolate(v, w, c) for v, w in zip(V, Vprev))
    return V + c * (V - Vprev)


def fbs_step(ns, P1, P0, cprev, b, tau, coef, restart, prox, accel=True):
    """One iteration of the reference's loop on the periodic stencil (A = div, A^H = grad, f = ||z - b||^2 / 2) from the state the previous
    iteration left: its prox output P1 = x_accel_new, the one before P0 = x_accel_old and the coefficient c_prev it applied, i.e.
    x_old = P1 + c_prev (P1 - P0) and z_old = div P1 + c_prev (div P1 - div P0) (:242-243 of the previous iteration).  A plain step, or the
    first one after the set-up, is P0 = P1 = x0 with c_prev = 0.  Returns the vectors and every scalar of the block, each as a Sum."""
    p1, p0, bb = _field(ns, P1), _field(ns, P0), ns.enter(b)
    t, c, cp = ns.enter(tau), ns.enter(coef), ns.enter(cprev)
    za_old = div(p1)                                              # z_accel of the previous iteration (:224)
    if cprev != 0.0:
        x_old, z_old = _extrapolate(p1, p0, cp), _extrapolate(za_old, div(p0), cp)
    else:
        x_old, z_old = p1, za_old
    grad_old = grad(z_old - bb)                                   # :248 of the previous iteration: A^H gradf(z), gradf(z) = z - b
    # forward-backward step (:181-188)
    x_hat = tuple(x - t * g for x, g in zip(x_old, grad_old))
    x_new = x_hat if prox == IDENTITY else tv_dual_ball(x_hat)
    step = _sub(x_new, x_old)
    z_new = div(x_new)
    out = {}
    out["S_FSQ"] = _dot(ns, (z_new - bb,), (z_new - bb,))         # 2 f(z_new)
    out["S_DXG0"] = _dot(ns, step, grad_old)                      # the backtracking test's inner product (:196)
    out["S_DX2"] = _dot(ns, step, step)
    back = _sub(x_new, x_hat)
    out["S_XH2"] = _dot(ns, back, back)                           # ||x_new - x_hat||^2 before the extrapolation
    out["S_G02"] = _dot(ns, grad_old, grad_old)
    out["S_GSUM"], out["S_GMAX"] = _l1(ns, x_new), _linf(x_new)
    # FISTA (:220-245): x_accel_old = P1
    rdot = _dot(ns, _sub(x_old, x_new), _sub(x_new, p1))
    out["S_RDOT"] = rdot
    value = rdot.value.to_float() if isinstance(rdot.value, Fx) else float(rdot.value)
    restarted = bool(accel and restart and value > RESTART_EPS)   # :231
    applied = coef if accel and not restarted else 0.0
    if applied != 0.0:
        x1, z1 = _extrapolate(x_new, p1, c), _extrapolate(z_new, za_old, c)
    else:
        x1, z1 = x_new, z_new
    grad_new = grad(z1 - bb)                                      # :248
    # Barzilai-Borwein (:253-258)
    dgrad = tuple(g + (xh - x) / t for g, xh, x in zip(grad_new, x_hat, x_old))
    out["S_DXDG"] = _dot(ns, step, dgrad)
    out["S_DG2"] = _dot(ns, dgrad, dgrad)
    out["S_FSQ_ADJ"] = _dot(ns, (z1 - bb,), (z1 - bb,))           # 2 f(z1')
    ahead = _sub(x1, x_hat)
    out["S_XH2_ADJ"] = _dot(ns, ahead, ahead)                     # ||x1 - x_hat||^2 (:280)
    out["S_GSUM_ADJ"], out["S_GMAX_ADJ"] = _l1(ns, x1), _linf(x1)
    out.update(xprox=x_new, z=z_new, x1=x1, x_hat=x_hat, restarted=restarted, applied=applied)
    return out


def as_image(v):
    """A field of the model as the float64 array the C ABI returns: (H, W, 2) for a pair, (H, W) otherwise."""
    if isinstance(v, tuple):
        return np.stack([as_image(k) for k in v], axis=-1)
    return v.to_float() if isinstance(v, Fx) else np.asarray(v, dtype=np.float64)


def scalar(s):
    """The float64 value of a Sum."""
    return s.value.to_float() if isinstance(s.value, Fx) else float(s.value)


# ---- operands ------------------------------------------------------------------------------------------------------------------------------------
X_SCALE = {IDENTITY: 1.0, TVBALL: 0.25}
B_SCALE = {IDENTITY: 1.0, TVBALL: 1.5}
SMALL_SEEDS = {(1, 5): 1, (2, 3): 2, (3, 1): 1}        # TV-ball operands of the images of fewer than 64 pixels: see the module's docstring


@functools.lru_cache(maxsize=None)
def operands(H, W, prox, seed=None):
    """(x0, b): integers of [-2, 2] and [-3, 3]; with the TV-ball prox times 1/4 and 3/2 (see the module's docstring)."""
    if seed is None:
        seed = SMALL_SEEDS.get((H, W), 0) if prox == TVBALL else 0
    rng = np.random.RandomState(7000 + 131 * H + W + 100003 * seed)
    x0 = rng.randint(-2, 3, size=(H, W, 2)).astype(np.float64) * X_SCALE[prox]
    b = rng.randint(-3, 4, size=(H, W)).astype(np.float64) * B_SCALE[prox]
    for v in (x0, b):
        v.setflags(write=False)
    return x0, b


def chain(ns, H, W, prox, state, seed=None):
    """The model of a state's launch: [the committed first step of a lagged chain,] the launch itself.  Returns (first or None, launch)."""
    x0, b = operands(H, W, prox, seed)
    if not state.lagged:
        return None, fbs_step(ns, x0, x0, 0.0, b, tau_of(state, prox), state.coef, state.restart, prox, accel=bool(state.accel))
    first = fbs_step(ns, x0, x0, 0.0, b, FIRST_TAU, FIRST_COEF, 1, prox)
    assert first["applied"] == FIRST_COEF                          # its dot is -||dx||^2: never a restart
    P1 = as_image(first["xprox"]) if ns is not LONGDOUBLE else np.stack(first["xprox"], axis=-1)
    return first, fbs_step(ns, P1, x0, FIRST_COEF, b, tau_of(state, prox), state.coef, state.restart, prox)


def plain_twice(ns, H, W, prox, tau=0.125):
    """Two plain steps back to back (step, commit, step): the second starts from the first one's prox output."""
    x0, b = operands(H, W, prox)
    one = fbs_step(ns, x0, x0, 0.0, b, tau, 0.0, 0, prox, accel=False)
    P1 = as_image(one["xprox"])
    return one, fbs_step(ns, P1, P1, 0.0, b, tau, 0.0, 0, prox, accel=False)


def reference_number(prox):
    return F64 if prox == IDENTITY else F64_WIDE_SUMS


@functools.lru_cache(maxsize=None)
def model(H, W, prox, state_name):
    """The reference of a launch, computed once and shared read-only: float64 (exact) with no prox, float64 elements and longdouble sums with
    the TV-ball prox.  Vectors as the arrays the C ABI returns."""
    first, m = chain(reference_number(prox), H, W, prox, STATE[state_name])
    out = dict(m)
    for k in ("xprox", "z", "x1", "x_hat"):
        out[k] = as_image(m[k])
        out[k].setflags(write=False)
    out["first"] = first
    return out


def sum_bound(s):
    """(terms + 4) * 2^-53 * sum|term|: see the module's docstring."""
    return (s.terms + 4) * 2.0 ** -53 * float(s.mag)


def outside_ball(x_hat):
    """Fraction of pixels whose forward point lies outside the unit ball."""
    y = as_image(x_hat)
    return float(np.mean(np.sqrt(y[..., 0] ** 2 + y[..., 1] ** 2) > 1.0))


# ---- the case lists ------------------------------------------------------------------------------------------------------------------------------
OnePass = collections.namedtuple("OnePass", "geometry prox state")


@functools.lru_cache(maxsize=None)
def onepass_cases():
    """geometry x prox x state; every case runs every tuning of its prox (tunings) under every FH_TUNE_TV_XCD of its geometry.  The two
    default-rule geometries leave the tuning alone."""
    return tuple(OnePass(g, prox, s) for g in GEOMETRIES for prox in (IDENTITY, TVBALL) for s in STATES)


def onepass_id(c):
    return f"{geometry_id(c.geometry)}-{c.prox}-{c.state.name}"


def onepass_launches(c):
    """(U, PIPE, NT, XCD) of every launch of a case; zeros (automatic) for the default-rule geometries."""
    if c.geometry.rows == 0:
        return [(0, 0, 0, 0)]
    return [(U, pipe, nt, xcd) for U, pipe, nt in tunings(c.prox) for xcd in c.geometry.xcd]


TwoLaunch = collections.namedtuple("TwoLaunch", "geometry prox state U nt")
TWO_LAUNCH_STATES = tuple(s for s in STATES if s.name in ("plain", "first", "restarts", "keeps"))


@functools.lru_cache(maxsize=None)
def two_launch_cases():
    """fh_fwd + fh_adj in both `accel` modes: U x NT x prox on the kernels' own strip seams and the chunk shapes; the state rotates so that every
    (U, NT, prox) meets the plain step and an accelerated one with either restart decision."""
    names = [g.name for g in GEOMETRIES if g.name.startswith("two-launch")] + ["wrap 1x1", "wrap 2x3", "wrap 3x1", "short chunk", "ragged trips",
                                                                             "rows above H", "finaliser second pass", BITS_GEOMETRY]
    out = []
    for i, name in enumerate(names):
        for j, (U, nt, prox) in enumerate(itertools.product(TWO_U, TWO_NT, (IDENTITY, TVBALL))):
            for k in range(2):
                out.append(TwoLaunch(GEOMETRY[name], prox, TWO_LAUNCH_STATES[(i + j + 2 * k) % 4], U, nt))
    return tuple(out)


def two_launch_id(c):
    return f"{geometry_id(c.geometry)}-{c.prox}-{c.state.name}-U{c.U}-nt{c.nt}"


def plain_pair_cases():
    """(geometry, NT) of fh_apply in both directions and of fh_init: k_fwd_tv<4, NT> / k_adj_tv<4, NT> on their 64-column strips."""
    names = ["wrap 1x1", "wrap 1x5", "wrap 2x3", "wrap 3x1", "two-launch 63", "two-launch 64", "two-launch 65", "two-launch 256", "two-launch 257",
             "short chunk", "ragged trips", "finaliser second pass", BITS_GEOMETRY]
    return [(GEOMETRY[n], nt) for n in names for nt in TWO_NT]


def reached_onepass(cases=None):
    """The k_tv_onepass instantiations a list of one-pass cases dispatches."""
    out = set()
    for c in cases if cases is not None else onepass_cases():
        for U, pipe, nt, _ in onepass_launches(c):
            out.add(onepass_instantiation(c.prox, c.state.accel, U, pipe, nt))
            if c.state.lagged:
                out.add(onepass_instantiation(c.prox, 1, U, pipe, nt))
    return out


def reached_two_launch():
    out = set()
    for c in two_launch_cases():
        out |= two_launch_instantiations(c.prox, c.U, c.nt)
    for _, nt in plain_pair_cases():
        out |= plain_pair_instantiations(nt)
    return out
