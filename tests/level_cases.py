"""Shared by tests/test_level_cpu.py and tests/test_gpu_level.py: the case table of the sort-free clipping-level search of FH_PROX_LINF / FH_PROX_L1BALL
(csrc/fh_prox.h), a restatement of its decisions (LvlCtl) -- a MODEL of the rule, held to the exact sort-based level without a GPU, never the thing
under test -- the exact reference, the dispatch rule restated, and deterministic inputs on a dyadic grid.

Exactness.  x0 and g0 are multiples of 2^-4 of magnitude at most 64 and tau is 1 or 1/4, so xhat = x0 - tau * g0 is exact and |xhat| a multiple of
GRID = 2^-6, at most 80; radii are multiples of GRID.  With n <= 2^19 every sum of |xhat| stays below 2^40 grid units: every partial sum is exact in
any order, and so is `s - radius`.  The one division is correctly rounded on both sides, and no active-set decision can flip by an ulp: an entry is
either exactly on the level (the comparison is strict: inactive) or at least GRID / count away from it.  The device's level must therefore EQUAL
fl((S_A - t) / |A|) of the true active set.  (`one_per_pass` leaves the magnitude bound -- integers near 2^40 -- but not the argument: 15 non-zeros.)"""
import collections
import fractions
import functools
import math

import numpy as np

GRID = 2.0 ** -6
LVL_WG, LVL_MEPT, LVL_MAXG = 1024, 8, 32            # csrc/fh_prox.h
LENGTHS = (1, 2, 3, 1023, 1024, 1025, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 24576, 24577, 262143, 262144, 262145, 300000)
EVERY_KIND_AT = (1025, 16385, 262145)
KINDS = ("distinct", "ties", "all_equal", "mostly_zero", "dominant", "radius_zero", "radius_is_l1", "radius_above_l1", "one_per_pass")
PROX_KINDS = ("linf", "l1ball")

LevelShape = collections.namedtuple("LevelShape", "multi threads ept workgroups")
Input = collections.namedtuple("Input", "x0 g0 tau radius")
Case = collections.namedtuple("Case", "kind n")


def shape_of(n):
    """What fh_level_shape_for must report for n entries: the dispatch rule of launch_level_search restated."""
    if n <= 4 * 256:
        return LevelShape(0, 256, 4, 1)
    if n <= 16 * 256:
        return LevelShape(0, 256, 16, 1)
    if n <= 32 * 256:
        return LevelShape(0, 256, 32, 1)
    if n <= 16 * LVL_WG:
        return LevelShape(0, LVL_WG, 16, 1)
    if n <= LVL_MAXG * LVL_MEPT * LVL_WG:
        return LevelShape(1, LVL_WG, LVL_MEPT, -(-n // (LVL_MEPT * LVL_WG)))
    return LevelShape(0, LVL_WG, 0, 1)


CLASS_EDGES = (1, 1024, 1025, 4096, 4097, 8192, 8193, 16384, 16385, 24576, 24577, 262144, 262145, 300000)


def class_name(n):
    sh = shape_of(n)
    if sh.multi:
        return f"multi-G{sh.workgroups}"
    return f"one-{sh.ept}x{sh.threads}"


def cases():
    out = [Case(kind, n) for kind in ("distinct", "ties") for n in LENGTHS]
    out += [Case(kind, n) for kind in KINDS[2:] for n in EVERY_KIND_AT]
    return tuple(out)


def case_id(c):
    return f"{c.kind}-{c.n}-{class_name(c.n)}"


# ---- the rule and the reference -------------------------------------------------------------------------------------------------------------
def _units(ax):
    """|xhat| in grid units as exact integers (the inputs are on the grid: asserted)"""
    u = np.asarray(ax, dtype=np.float64) / GRID
    k = u.astype(np.int64)
    assert np.array_equal(k.astype(np.float64), u) and (k >= 0).all(), "an entry is off the grid"
    return k


def model(ax, radius, guess=None):
    """LvlCtl (csrc/fh_prox.h) restated: (level, passes, final_count).  The guess counts only if it is positive and finite; the pass from a guess
    only sets a lower bound and restarts cold when nothing lies above the guess; otherwise strict `>`, stop when the count is 0 or unchanged.  The
    sums are exact integers of grid units rounded once, the subtraction and the division are float64's."""
    ax = np.asarray(ax, dtype=np.float64)
    units = _units(ax)
    radius = np.float64(radius)
    alpha = np.float64(guess) if (guess is not None and guess > 0.0 and guess < np.inf) else np.float64(-np.inf)
    warm = bool(alpha > 0.0)
    prev, passes, cnt = -1.0, 0, 0.0
    while True:
        active = ax > alpha
        s = np.float64(float(fractions.Fraction(int(units[active].sum()), 64)))
        cnt = float(np.count_nonzero(active))
        passes += 1
        assert passes <= 100000
        if warm:
            warm = False
            alpha = np.float64(-np.inf) if cnt == 0.0 else (s - radius) / np.float64(cnt)
            continue
        if cnt == 0.0 or cnt == prev:
            break
        prev = cnt
        alpha = (s - radius) / np.float64(cnt)
    return float(alpha), passes, int(cnt)


def exact_level(ax, radius):
    """The reference: max_k (c_k - t) / k over the descending cumulative sums (fasta/proximal.py:22-26), in rationals, rounded once to float64."""
    units = np.sort(_units(ax))[::-1]
    t = fractions.Fraction(float(radius)) * 64
    csum = np.cumsum(units)
    k = np.arange(1, units.size + 1, dtype=np.int64)
    assert t.denominator == 1 and float(np.max(units.astype(np.float64) * k)) < 2.0 ** 62, "the radius is off the grid, or the integers overflow"
    # the quotients rise while a_k > (c_k - t) / k, i.e. a_k * k > c_k - t (integers), and fall afterwards: the maximum sits at the last such k --
    # or at k = 1 when there is none (t = 0), or at k = n when every quotient is negative; all of them are compared, in rationals
    rising = np.flatnonzero(units * k > csum - int(t))
    candidates = {1, units.size, int(np.argmax((csum - float(t)) / k)) + 1} | ({int(rising[-1]) + 1} if rising.size else set())
    best = max(fractions.Fraction(int(csum[c - 1]) - int(t), c) for c in candidates)
    return float(best / 64)


def same_level(a, b):
    """equal as float64 bits where positive; at or below zero only the sign class counts (the prox distinguishes nothing else)"""
    if a > 0.0 or b > 0.0:
        return a == b
    return True


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def _seed(kind, n):
    return 1000 * KINDS.index(kind) + n


def _from_xhat(xhat, rng, tau):
    """(x0, g0) with x0 - tau * g0 == xhat exactly; g0 multiples of 1/4 in [-2, 2], non-zero for about three entries in four"""
    g0 = rng.randint(-8, 9, size=xhat.size) / 4.0
    g0[xhat == 0.0] = 0.0                               # (a zero of xhat keeps the sign of its x0)
    return xhat + tau * g0, g0


def _signs(rng, n):
    return np.where(rng.randint(0, 2, size=n) == 0, 1.0, -1.0)


def _grid_radius(v):
    return math.floor(v / GRID) * GRID


def one_per_pass_values(V=2 ** 40, t=2 ** 20):
    """non-zeros, top-down: given the set's sum S and size m, a = (S - t) / m, add the largest integer below a - (m + 1)(a - min) (and below a):
    the pass that holds the new entry drops it and nothing else"""
    vals = [V]
    while len(vals) < 64:
        S, m = sum(vals), len(vals)
        a = fractions.Fraction(S - t, m)
        v = math.ceil(min(a - (m + 1) * (a - min(vals)), a)) - 1
        if v < 1:
            break
        vals.append(v)
    return vals


@functools.lru_cache(maxsize=8)
def build(case):
    """The Input of a case; arrays are read-only."""
    kind, n = case
    rng = np.random.RandomState(_seed(kind, n))
    tau = 1.0
    if kind in ("distinct", "radius_zero", "radius_is_l1", "radius_above_l1"):
        tau = 0.25
        x0 = rng.randint(-1024, 1025, size=n) / 16.0
        g0 = rng.randint(-1024, 1025, size=n) / 16.0
        if not np.any(x0 - tau * g0):
            x0[0] = 3.0
        l1 = float(np.abs(x0 - tau * g0).sum())
        radius = {"distinct": _grid_radius(0.3 * l1), "radius_zero": 0.0, "radius_is_l1": l1, "radius_above_l1": 2.0 * l1}[kind]
    elif kind == "ties":
        hi = max(1, n // 8)
        mid = (n - hi + 1) // 2
        mags = np.concatenate([np.full(hi, 4.0), np.full(mid, 2.0), np.full(n - hi - mid, 1.0)])
        xhat = rng.permutation(mags) * _signs(rng, n)
        x0, g0 = _from_xhat(xhat, rng, tau)
        radius = 2.0 * hi                               # sum over the 4s of (4 - 2): the level falls exactly on the middle value
    elif kind == "all_equal":
        xhat = 3.0 * _signs(rng, n)
        x0, g0 = _from_xhat(xhat, rng, tau)
        radius = n / 4.0                                # level 3 - 1/4
    elif kind == "mostly_zero":
        tau = 0.25
        xhat = np.zeros(n)
        nz = rng.choice(n, size=max(2, n // 100), replace=False)
        xhat[nz] = rng.randint(1, 1009, size=nz.size) / 16.0 * _signs(rng, nz.size)
        x0, g0 = _from_xhat(xhat, rng, tau)
        zeros = np.flatnonzero(xhat == 0.0)
        x0[zeros[::2]] = -0.0                           # both zeros, at even and odd positions of the pairs the kernels load
        x0[zeros[:2]] = [0.0, -0.0]
        radius = _grid_radius(0.3 * float(np.abs(xhat).sum()))
    elif kind == "dominant":
        tau = 0.25
        xhat = rng.randint(-16, 17, size=n) / 16.0
        xhat[n // 3] = -60.0
        x0, g0 = _from_xhat(xhat, rng, tau)
        radius = 1.0
    elif kind == "one_per_pass":
        vals = one_per_pass_values()
        xhat = np.zeros(n)
        xhat[n - len(vals):] = np.array(vals[::-1], dtype=np.float64) * _signs(rng, len(vals))      # at the END: the last workgroup holds them
        x0, g0 = _from_xhat(xhat, rng, tau)
        radius = float(2 ** 20)
    else:
        raise KeyError(kind)
    out = Input(x0, g0, tau, float(radius))
    assert np.array_equal(x0 - tau * g0 + tau * g0, x0)
    for v in (x0, g0):
        v.setflags(write=False)
    return out


def xhat_of(inp):
    return inp.x0 - inp.tau * inp.g0


def mu_of(inp, prox):
    """the mu that gives the search the case's radius: FH_PROX_LINF searches with tau * mu, FH_PROX_L1BALL with mu"""
    return inp.radius / inp.tau if prox == "linf" else inp.radius


def sgn(x):
    """csrc/fh_device.h: (x > 0) - (x < 0), +0.0 at either zero"""
    return (x > 0).astype(np.float64) - (x < 0).astype(np.float64)


def prox_of(prox, xhat, level):
    """csrc/fh_device.h, prox_scalar: LINF  level > 0 ? fmin(|x|, level) * sgn(x) : +0.0;  L1BALL  x minus that"""
    clip = np.minimum(np.abs(xhat), level) * sgn(xhat) if level > 0.0 else np.zeros(xhat.size)
    return clip if prox == "linf" else xhat - clip


def guesses(ax, level):
    """left-over levels a search may start from: far below the root, between the root and the largest entry, above every entry, at or below zero"""
    top = float(np.max(ax))
    out = [GRID / 4.0, top + 1.0, 0.0, -3.5, float("inf"), float("nan")]
    if level > 0.0:
        out += [level / 1024.0, level, (level + top) / 2.0]
    return out


# ---- a small dense problem for the one-pass step: integer A, the level exactly on the middle value ----------------------------------------------
StepProblem = collections.namedtuple("StepProblem", "A b x0 g0 tau radius")
STEP_SHAPES = ((16, 4097), (16, 16385))


@functools.lru_cache(maxsize=2)
def step_problem(m, n):
    """A of -1, 0, 1 (one entry in four non-zero), b = A x0 + noise of multiples of 1/2, so g0 = A^T (A x0 - b) = -A^T noise is exact; x0 is chosen
    so that xhat = x0 - g0 / 4 is the `ties` vector of 4s, 2s and 1s, whose level under radius 2 * #4s is exactly 2: xprox, z = A xprox,
    g1 = A^T (z - b) and every sum of the step are then exact in any order (sums_are_exact below checks the magnitudes)."""
    rng = np.random.RandomState(77 + m + n)
    A = ((rng.randint(0, 2, size=(m, n)) * 2 - 1) * (rng.randint(0, 4, size=(m, n)) == 0)).astype(np.float64)
    noise = rng.randint(-2, 3, size=m) / 2.0
    noise[0] = 1.0
    g0 = 0.0 - A.T @ noise                              # (0.0 - x: a zero sum stays +0.0, as the device's sum is)
    tau = 0.25
    hi = n // 8
    mid = (n - hi + 1) // 2
    xhat = rng.permutation(np.concatenate([np.full(hi, 4.0), np.full(mid, 2.0), np.full(n - hi - mid, 1.0)])) * _signs(rng, n)
    x0 = xhat + tau * g0
    b = A @ x0 + noise
    out = StepProblem(A, b, x0, g0, tau, 2.0 * hi)
    for v in out[:4]:
        v.setflags(write=False)
    return out


def step_model(p, prox):
    """float64 restatement of one FBS step (K-fwd, K-adj) on a StepProblem: level, vectors, and per scalar the terms it sums"""
    xhat = p.x0 - p.tau * p.g0
    level = model(np.abs(xhat), p.radius)[0]
    xp = prox_of(prox, xhat, level)
    z = p.A @ xp
    g1 = p.A.T @ (z - p.b)
    dx, dg = xp - p.x0, g1 + (xhat - p.x0) / p.tau
    terms = dict(fsq=(z - p.b) ** 2, dxg0=dx * p.g0, dx2=dx * dx, xh2=(xp - xhat) ** 2, g02=p.g0 * p.g0, gsum=np.abs(xp), dxdg=dx * dg, dg2=dg * dg)
    return dict(level=level, xhat=xhat, xprox=xp, z=z, g1=g1, terms=terms)


def sums_are_exact(terms, lsb):
    """every term a multiple of lsb and the sum of magnitudes below 2^52 of them: any order of summation, fused or not, gives the same float64"""
    return all(np.array_equal(np.rint(t / lsb), t / lsb) and float(np.abs(t).sum()) < 2.0 ** 52 * lsb for t in terms.values())
