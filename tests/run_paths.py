"""Cases, claimed geometry, exact operands and the model for the tests of EVERY path of the device-side loop kernel (csrc/fh_run.h:
k_run_dense<PPT>, what fh_run launches).  A plain helper module, the sibling of tests/mc_paths.py: the CPU tier (tests/test_run_paths_cpu.py)
proves every condition claimed here, the GPU tier (tests/test_gpu_run_paths.py) runs the kernel.

Geometry.  Which instantiation, how many workgroups, how many rows each and how phase B splits the columns depend on the device's CU count and
on the rows-per-team floor; every case pins both (FH_TUNE_FUSED_CUS <= 64, the high half of FH_TUNE_FUSED_VARIANT), states the geometry it
expects (expected_shape) and both tiers compare that with the library's own rule (fh_run_shape_for / fh_run_shape), so a change of the host's
rule fails a test instead of emptying it.

Exactness.  Geometry "A": A holds -1, 0, 1 with a quarter of the entries non-zero, x0 a few multiples of 1/2.  Geometry "B": 8 or 16 entries of
+-1 per row, x0 dense multiples of 1/2.  b multiples of 1/2, mu = 1, tau0 and stepsize_shrink powers of two: every product of an attempt is exact
and every sum stays below 2^53 of its terms' common lsb over the compared iterations, whatever the order of summation and whichever
multiply-adds are fused -- tests/test_run_paths_cpu.py proves that in integer arithmetic (prove) -- so the kernel's history records, the state it
writes back and the vectors it leaves must EQUAL the model's.  What is not dyadic (the square root in f and in the residual, the
Barzilai-Borwein quotient) is one correctly rounded operation on exact sums in the controller's own order."""
import collections
import functools
import math

import numpy as np

from fasta_python_amd import hip

FH_WG = 256                                          # csrc/fh_device.h
RUN_TABLE = (1, 2, 4, 5, 6, 7, 8, 10, 12, 14)        # csrc/fasta_hip.hip: kRunTable
WINDOW_MAX = hip.RUN_WINDOW_MAX
KINDS = ("identity", "shrink", "nonneg", "box")
PROX = {"identity": (hip.PROX_IDENTITY, 1.0, 0.0, 0.0), "shrink": (hip.PROX_SHRINK, 1.0, 0.0, 0.0), "nonneg": (hip.PROX_NONNEG, 1.0, 0.0, 0.0),
        "box": (hip.PROX_BOX, 1.0, 2.0 ** -6, 2.0)}
# (kind, mu, lo, hi): mu = 1.  The box EXCLUDES zero: every other kind maps the zero padding behind an odd row's last entry to zero, so a last
# column pair that is masked wrongly would change nothing; here it puts 1/64 into the sums and into the padding.  (1/64: about the size of
# geometry A's first forward step, so that some entries are clipped and others pass.)
SUMS = ("FSQ", "DXG0", "DX2", "XH2", "G02", "GSUM", "GMAX", "RDOT", "DXDG", "DG2", "FSQ_ADJ", "XH2_ADJ", "GSUM_ADJ", "GMAX_ADJ")      # FC_* of csrc/fh_controller.h
VECTORS = {"X0": hip.VEC_X0, "G0": hip.VEC_G0, "XHAT": hip.VEC_XHAT, "XPROX": hip.VEC_XPROX, "X1": hip.VEC_X1, "G1": hip.VEC_G1,
           "BEST": hip.VEC_BEST, "Z": hip.VEC_Z}
STATE_FIELDS = ("tau_next", "alpha1", "max_residual", "best_quality", "iteration", "backtracks", "stopped")

# mode: plain / adaptive / accel; ctl: "" | "maxbt" (max_backtracks = 2) | "stop" (the stop rule fires) | "stale" (the entering best_quality
# cannot be beaten: no iteration is `better`); steps: compared iterations (what the proof covers)
Case = collections.namedtuple("Case", "name m n cus floor geom per_row mode restart kind nt evalobj window steps log2_tau0 ctl")


def round_up(v, k):
    return (v + k - 1) // k * k


# ---- the case list ---------------------------------------------------------------------------------------------------------------------------
# row-block geometries (m, cus, floor): what each is for is asserted through paths_of, not trusted
ROWS = {
    "short_last": (20, 6, 0),        # mp = 32 on 6 workgroups: blocks of 6 rows, a last one of 2; 12 padding rows inside live blocks
    "one_row_last": (50, 10, 0),     # mp = 64 on 10: blocks of 7, the last of 1
    "empty_wgs": (70, 64, 0),        # mp = 80 on 64: 40 blocks of 2 rows, 24 workgroups without rows
    "one_wg": (20, 1, 0),            # G = 1: one block of 32 rows
    "floor16": (300, 64, 16),        # the default floor: 24 workgroups of 13 rows, the last of 5
}
ROW_ORDER = ("short_last", "one_row_last", "empty_wgs", "one_wg", "floor16")


def _widths():
    """(tag, n) per table entry: a row of exactly PPT * 512 columns, a clamped one (n odd, n % 16 != 0, lanes past the row's end), rows that need
    3 / 9 / 11 / 13 pieces per lane and take the next entry up, and further clamped rows so that every NB meets every row-block geometry."""
    out = []
    for ppt in RUN_TABLE:
        out.append((f"full{ppt}", ppt * 512))
    for ppt in RUN_TABLE:
        out.append((f"clamped{ppt}", (ppt - 1) * 512 + 37))
    for need in (3, 9, 11, 13):
        out.append((f"idle{need}", (need - 1) * 512 + 37))
    out += [("extra5", 4 * 512 + 203), ("extra6", 5 * 512 + 75), ("extra7", 6 * 512 + 301), ("extra8", 7 * 512 + 11)]
    return out


MODES = (("plain", 0), ("adaptive", 0), ("accel", 0), ("accel", 1))


@functools.lru_cache(maxsize=None)
def cases():
    out, per_nb, per_geom = [], collections.Counter(), collections.Counter()
    for i, (tag, n) in enumerate(_widths()):
        ppt = ppt_of(n)
        nb = nb_of(ppt)
        rows = ROW_ORDER[per_nb[nb] % len(ROW_ORDER)]
        per_nb[nb] += 1
        m, cus, floor = ROWS[rows]
        full = tag.startswith("full")
        geom = "B" if full or tag.startswith("idle") else "A"
        mode, restart = ("plain", 0) if full else MODES[i % 4]
        steps = {"plain": 4 if geom == "B" else 1, "adaptive": 1, "accel": 2}[mode]
        per_row = 16 if (geom == "B" and m <= 70) else 8      # (few rows: 8 entries per row leave the first step without a retry)
        # the prox kinds rotate per geometry; NonNeg only where x0 is dense (B): on A's few non-zeros it returns x0 itself in half the entries
        per_geom[geom] += 1
        kind = KINDS[per_geom[geom] % 4] if geom == "B" else ("identity", "shrink", "box")[per_geom[geom] % 3]
        out.append(Case(f"{tag}-{rows}", m, n, cus, floor, geom, per_row, mode, restart, kind, i % 2, (i // 2) % 2,
                        1 if i % 3 == 0 else 10, steps, None, ""))
    # the controller's corners and phase B's, at small widths
    out.append(Case("maxbt", 50, 1573, 2, 0, "A", 8, "plain", 0, "shrink", 0, 1, 10, 1, None, "maxbt"))     # share = 396: one slice, a ragged second trip
    out.append(Case("stop", 50, 1030, 10, 0, "B", 8, "plain", 0, "identity", 1, 0, 10, 1, None, "stop"))
    out.append(Case("stale_best", 20, 600, 6, 0, "B", 16, "plain", 0, "box", 0, 1, 10, 3, None, "stale"))
    out.append(Case("stale_best_accel", 50, 3500, 10, 0, "B", 16, "accel", 1, "nonneg", 1, 0, 1, 2, None, "stale"))
    out.append(Case("one_trip", 70, 1030, 3, 0, "B", 8, "plain", 0, "shrink", 1, 1, 10, 3, None, ""))       # share = 173: one slice, one trip
    return tuple(out)


def case_id(c):
    return f"{c.name}-{c.m}x{c.n}-{c.geom}-{c.mode}{'-restart' if c.restart else ''}-{c.kind}-nt{c.nt}"


def need_of(n):
    return -(-(round_up(n, 16) // 2) // FH_WG)


def ppt_of(n):
    return next(p for p in RUN_TABLE if p >= need_of(n))


def nb_of(ppt):
    """row buffers of k_run_dense<PPT> (csrc/fh_run.h: NB)"""
    return 3 if ppt > 8 else (4 if ppt >= 7 else (5 if ppt >= 5 else 6))


def tuning_of(case):
    t = {hip.TUNE_FUSED_CUS: case.cus, hip.TUNE_FUSED_VARIANT: ((case.floor or 0xFFFF) << 16) | 34, hip.TUNE_NT_LOADS: case.nt}
    if case.n > 4096:
        t[hip.TUNE_RUN_MAX_N] = 7168
    return t


def shape_query(case):
    """the library's own rule in its pure form, with the numbers tuning_of() sets"""
    return hip.run_shape_for(case.m, case.n, cus=case.cus, min_rows=case.floor, run_max_n=7168 if case.n > 4096 else 0, nt_loads=case.nt)


# ---- what a case claims ----------------------------------------------------------------------------------------------------------------------
def expected_shape(case):
    """The hip.RunShape a case must be launched with, from the case's own numbers."""
    mp, ld2 = round_up(case.m, 16), round_up(case.n, 16) // 2
    ppt = ppt_of(case.n)
    G = case.cus if not case.floor else min(case.cus, max(8, round_up(-(-mp // case.floor), 8)))
    rpt = -(-mp // G)
    live = -(-mp // rpt)
    share = -(-ld2 // G)
    slices = min(FH_WG // share, G) if share < FH_WG else 1
    return hip.RunShape(PPT=ppt, need=need_of(case.n), XLDS=int(ppt >= 7), BIG=int(ppt > 8), NB=nb_of(ppt), G=G, rows_per_team=rpt, empty_wgs=G - live,
                        last_rows=mp - (live - 1) * rpt, share=share, slices=slices, tps=-(-G // slices), trips=-(-share // FH_WG), NT=case.nt, ld2=ld2)


ROW_PATHS = ("padding rows in a live block", "workgroups with no rows", "short last block", "r_end % NB != 0", "r_end < NB - 1", "r_end == 1",
             "block of >= 2 NB rows")
PHASE_B_PATHS = ("slices > 1, slices * tps > G", "slices > 1, last share cut", "slices == 1, one trip", "slices == 1, ragged trips", "G == 1")
LANE_PATHS = ("all lanes live", "clamped lanes", "idle piece")


def paths_of(sh, m, n):
    """The paths a launch geometry `sh` (hip.RunShape) of an (m, n) matrix runs, as a dict of booleans: the rows of the coverage table
    (scripts/run_path_coverage.py) and what the CPU tier asserts of every case."""
    mp = round_up(m, 16)
    blocks = {sh.rows_per_team, sh.last_rows}           # r_end of the workgroups that have rows
    live = sh.G - sh.empty_wgs
    return {
        "all lanes live": sh.PPT * FH_WG == sh.ld2 and n == 2 * sh.ld2,
        "clamped lanes": sh.PPT * FH_WG > sh.ld2 and n % 2 == 1 and n % 16 != 0,
        "idle piece": sh.need < sh.PPT,
        "padding rows in a live block": m % 16 != 0 and m < mp,
        "workgroups with no rows": sh.empty_wgs > 0,
        "short last block": live > 1 and sh.last_rows < sh.rows_per_team,
        "r_end % NB != 0": any(r % sh.NB for r in blocks),
        "r_end < NB - 1": any(r < sh.NB - 1 for r in blocks),
        "r_end == 1": 1 in blocks,
        "block of >= 2 NB rows": any(r >= 2 * sh.NB for r in blocks),
        "slices > 1, slices * tps > G": sh.slices > 1 and sh.slices * sh.tps > sh.G,
        "slices > 1, last share cut": sh.slices > 1 and sh.G * sh.share > sh.ld2,
        "slices == 1, one trip": sh.slices == 1 and sh.trips == 1 and sh.G > 1,
        "slices == 1, ragged trips": sh.slices == 1 and sh.trips > 1 and sh.share % FH_WG != 0,
        "G == 1": sh.G == 1,
    }


# ---- operands --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def matrix(m, n, geom, per_row):
    """float64 (m, n) of -1, 0, 1.  "A": a quarter of the entries non-zero, no empty row or column.  "B": per_row entries per row in random
    columns, the first and the last column among them."""
    rng = np.random.RandomState(7000 + 31 * m + n + (0 if geom == "A" else per_row))
    if geom == "A":
        A = rng.choice([-1, 1], size=(m, n)) * (rng.randint(0, 4, size=(m, n)) == 0)
        for j in np.flatnonzero(~A.any(axis=0)):
            A[j % m, j] = 1
        for i in np.flatnonzero(~A.any(axis=1)):
            A[i, i % n] = -1
    else:
        A = np.zeros((m, n), dtype=np.int64)
        for i in range(m):
            A[i, rng.choice(n, size=min(per_row, n), replace=False)] = rng.choice([-1, 1], size=min(per_row, n))
        A[0, 0], A[m - 1, n - 1] = 1, -1
    A = A.astype(np.float64)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def operands(case):
    """(A, x0, b, log2 tau0)"""
    A = matrix(case.m, case.n, case.geom, case.per_row)
    rng = np.random.RandomState(9000 + case.m + 3 * case.n)
    if case.geom == "A":
        x0 = np.zeros(case.n)
        idx = np.unique(np.concatenate([[0, case.n - 1], rng.choice(case.n, size=max(4, case.n // 64), replace=False)]))
        x0[idx] = rng.choice([-2.0, -1.5, -1.0, -0.5, 0.5, 1.0, 1.5, 2.0], size=idx.size)
        b = rng.randint(-4, 5, size=case.m) / 2.0
        # a step about 16 times the reciprocal of ||A||^2 ~ (sqrt m + sqrt n)^2 / 4, as a power of two: the first iteration has to backtrack
        log2_tau0 = 4 - int(math.floor(math.log2((math.sqrt(case.m) + math.sqrt(case.n)) ** 2 / 4)))
    else:
        x0 = rng.randint(-4, 5, size=case.n) / 2.0
        b = rng.randint(-8, 9, size=case.m) / 2.0
        log2_tau0 = -1
    if case.log2_tau0 is not None:
        log2_tau0 = case.log2_tau0
    for v in (x0, b):
        v.setflags(write=False)
    return A, x0, b, log2_tau0


def run_opts(case, cls=hip.RunOpts):
    o = cls()
    o.adaptive, o.accelerate, o.backtrack, o.restart = int(case.mode == "adaptive"), int(case.mode == "accel"), 1, int(case.restart)
    o.evaluate_objective, o.stop_rule, o.window = int(case.evalobj), 0, int(case.window)
    o.max_backtracks = 2 if case.ctl == "maxbt" else 20
    o.stepsize_shrink, o.tolerance = 0.5, (1e300 if case.ctl == "stop" else 0.0)
    return o


def entering_state(case, f0, log2_tau0, cls=hip.RunState):
    """The caller's state before the first iteration.  Accelerated cases enter with alpha1 = 0: fc_alpha then gives coef = -1 in the first
    iteration and 0 in the second -- two exact iterations with an extrapolation that is not the identity."""
    st = cls()
    st.tau_next, st.alpha1 = 2.0 ** log2_tau0, (0.0 if case.mode == "accel" else 1.0)
    st.max_residual, st.best_quality = -np.inf, (-1.0 if case.ctl == "stale" else np.inf)
    st.iteration, st.backtracks, st.stopped = 0, 0, 0
    st.f_window[0] = f0
    return st


# ---- the controller, restated (csrc/fh_controller.h with FcSqMul; tests/test_run_paths_cpu.py proves it equal to the shipped header) ---------
_f = np.float64


def _sq(x):
    return x * x


def fc_f(lsq, s):
    return _f(0.5) * _sq(np.sqrt(_f(s))) if lsq else _f(s)


def fc_backtrack(o, fwin, iteration, f1, dxg0, dx2, tau, bt):
    if not o.backtrack:
        return False
    i = int(iteration)
    lo = i + 1 - o.window if i + 1 > o.window else 0
    M = _f(fwin[lo % WINDOW_MAX])
    for j in range(lo + 1, i + 1):
        v = _f(fwin[j % WINDOW_MAX])
        if M != M:
            break
        if v != v or v > M:
            M = v
    with np.errstate(all="ignore"):
        return bool(_f(f1) - (M + _f(dxg0) + _sq(np.sqrt(_f(dx2))) / (_f(2.0) * _f(tau))) > 1E-12 and bt < o.max_backtracks)


def fc_alpha(o, alpha1, rdot):
    """(alpha0, alpha1, coef, restarted)"""
    if not o.accelerate:
        return _f(0.0), _f(alpha1), _f(0.0), False
    alpha0, restarted = _f(alpha1), False
    if o.restart and rdot > 1E-30:
        alpha0, restarted = _f(1.0), True
    a1 = (_f(1.0) + np.sqrt(_f(1.0) + _f(4.0) * _sq(alpha0))) / _f(2.0)
    return alpha0, a1, (alpha0 - _f(1.0)) / a1, restarted


def fc_decide(o, lsq, g_kind, mu, s, tau, bt, alpha1, max_residual, best_quality):
    """dict of fc_decide's FcDecision fields plus `record`, the FR_HIST history doubles"""
    s = [_f(v) for v in s]
    tau = _f(tau)
    FSQ, DX2, G02, DXDG, DG2, FSQ_ADJ = s[0], s[2], s[4], s[8], s[9], s[10]
    alpha0, a1, coef, restarted = fc_alpha(o, alpha1, s[7])
    with np.errstate(all="ignore"):
        f1 = fc_f(lsq, FSQ_ADJ if o.accelerate else FSQ)
        xh2, gsum, gmax = (s[11], s[12], s[13]) if o.accelerate else (s[3], s[5], s[6])
        tau_next = tau
        dx_norm = np.sqrt(DX2)
        if o.adaptive:
            tau_s = _sq(dx_norm) / DXDG
            q = DXDG / _sq(np.sqrt(DG2))
            tau_m = _f(0.0) if 0.0 > q else q
            tau_next = tau_m if _f(2.0) * tau_m > tau_s else tau_s - _f(.5) * tau_m
            if tau_next <= 0.0 or np.isinf(tau_next) or np.isnan(tau_next):
                tau_next = tau * _f(1.5)
        resid = dx_norm / tau
        na, nb = np.sqrt(G02), np.sqrt(xh2) / tau
        normalizer = (nb if nb > na else na) + _f(1E-12)
        norm_resid = resid / normalizer
        new_max = resid if resid > max_residual else _f(max_residual)
        objective, quality = _f(0.0), resid
        if o.evaluate_objective:
            g = _f(mu) * gsum if g_kind == 1 else (_f(mu) * gmax if g_kind == 2 else _f(0.0))
            objective = f1 + g
            quality = objective
        better = bool(quality < best_quality)
        ratio, normed = bool(resid / new_max < o.tolerance), bool(norm_resid < o.tolerance)
        stop = [bool(resid < o.tolerance), normed, ratio, ratio or normed][o.stop_rule]
    record = [resid, norm_resid, tau, f1, objective, _f(bt), alpha0, _f((1.0 if better else 0.0) + (2.0 if restarted else 0.0))]
    return dict(better=better, stop=stop, restarted=restarted, tau_next=tau_next, alpha0=alpha0, alpha1=a1, coef=coef, f1=f1,
                max_residual=new_max, best_quality=quality if better else _f(best_quality), record=[float(v) for v in record])


def fc_rotate(accelerate, better, roles, perm):
    """fh_commit's rotation of the buffer roles: roles = [xi, ti, bi, pc, gc, zc, last_accel], perm[5]; returns the new pair"""
    xi, ti, bi, pc, gc, zc, last_accel = roles
    perm = list(perm)
    if accelerate:
        pc ^= 1
        last_accel = 1
    else:
        perm[ti], perm[3 + (pc ^ 1)] = perm[3 + (pc ^ 1)], perm[ti]
        last_accel = 0
    xi = ti
    if better:
        bi = xi
    ti = next(k for k in range(3) if k != xi and k != bi)
    return [xi, ti, bi, pc, gc ^ 1, zc ^ 1, last_accel], perm


# ---- one attempt: the reference's order of operations, all 14 sums ---------------------------------------------------------------------------
def prox_of(kind, x, thr, lo, hi):
    if kind == "shrink":
        return np.sign(x) * np.maximum(np.abs(x) - thr, 0)
    if kind == "nonneg":
        return np.maximum(x, 0)
    if kind == "box":
        return np.minimum(np.maximum(x, lo), hi)
    return x.copy()


def loss_grad(z, b, loss, dtype=np.float64):
    return z - b if loss == "lsq" else -b / (1 + np.exp(b * z))


def loss_sum(z, b, loss):
    """what the device adds up for f: squares of the residual (least squares), the loss itself (logistic)"""
    if loss == "lsq":
        return np.sum((z - b) * (z - b))
    return np.sum(np.log(1 + np.exp(z)) - np.where(b == 1, z, 0))


def attempt(A, b, x0, g0, xacc0, zacc0, tau, coef, accelerate, kind, loss="lsq", dtype=np.float64, magnitudes=None):
    """One attempt with step tau at (x0, g0): fasta/__init__.py:181-188 and :242-254 as the device runs them.  Returns (sums in FC_* order, vectors).
    coef: the extrapolation coefficient, or a function of this attempt's restart dot that gives it (fc_alpha: the kernel forms the dot first).
    magnitudes: a dict that receives the sums of the signed sums' |terms| (the tolerance of the inexact cases)."""
    _, mu, lo, hi = PROX[kind]
    tau = dtype(tau)
    xhat = x0 - tau * g0
    xp = prox_of(kind, xhat, tau * dtype(mu), dtype(lo), dtype(hi))
    dx, dh = xp - x0, xp - xhat
    xa = xacc0 if accelerate else np.zeros_like(x0)
    if callable(coef):
        coef = coef(float(np.sum((x0 - xp) * (xp - xa))))
    coef = dtype(coef)
    z = A @ xp
    zx = z + coef * (z - zacc0) if accelerate else z
    rv = loss_grad(zx, b, loss)
    g1 = A.T @ rv
    x1 = xp + coef * (xp - xacc0) if accelerate else xp
    dg = g1 + (xhat - x0) / tau
    dh1 = x1 - xhat
    fsq = loss_sum(z, b, loss)
    fsq_adj = loss_sum(zx, b, loss) if accelerate else dtype(0)
    sums = [fsq, np.sum(dx * g0), np.sum(dx * dx), np.sum(dh * dh), np.sum(g0 * g0), np.sum(np.abs(xp)), np.max(np.abs(xp)),
            np.sum((x0 - xp) * (xp - xa)), np.sum(dx * dg), np.sum(dg * dg), fsq_adj, np.sum(dh1 * dh1), np.sum(np.abs(x1)), np.max(np.abs(x1))]
    if magnitudes is not None:
        magnitudes.update(DXG0=np.sum(np.abs(dx * g0)), DXDG=np.sum(np.abs(dx * dg)), G1=np.abs(A).T @ np.abs(rv), Z=np.abs(A) @ np.abs(xp))
    return sums, dict(xhat=xhat, xprox=xp, z=z, g1=g1, x1=x1, coef=float(coef))


# ---- the loop: controller on top of the attempts, buffer roles as the context keeps them ------------------------------------------------------
class Model:
    """State of a solve as fh_init leaves it; run(k) is fh_run(max_steps = k)."""

    def __init__(self, case, x0=None, loss="lsq", dtype=np.float64, on_attempt=None):
        A, x0_, b, log2_tau0 = operands(case)
        self.case, self.loss, self.dtype, self.on_attempt = case, loss, dtype, on_attempt
        self.A, self.b = A.astype(dtype), (np.where(b > 0, 1.0, -1.0) if loss == "logistic" else b).astype(dtype)
        x0 = (x0_ if x0 is None else x0).astype(dtype)
        z0 = self.A @ x0
        g0 = self.A.T @ loss_grad(z0, self.b, loss)
        self.f0 = fc_f(loss == "lsq", float(loss_sum(z0, self.b, loss)))
        self.nb = [x0, None, None, x0.copy(), None]          # the physical n-side buffers X[0..2], P[0..1]
        self.G, self.Z, self.xhat = [g0, None], [z0, None], None
        self.roles, self.perm = [0, 1, 0, 0, 0, 0, 0], [0, 1, 2, 3, 4]
        self.o = run_opts(case)
        self.st = dict(tau_next=2.0 ** log2_tau0, alpha1=0.0 if case.mode == "accel" else 1.0, max_residual=-np.inf,
                       best_quality=-1.0 if case.ctl == "stale" else np.inf, iteration=0, backtracks=0, stopped=0)
        self.fwin = [0.0] * WINDOW_MAX
        self.fwin[0] = float(self.f0)
        self.history, self.retries, self.all_sums = [], [], []
        self.magnitudes = {} if loss != "lsq" else None       # of the last attempt (the inexact cases' tolerance)

    def run(self, max_steps):
        o, st, case = self.o, self.st, self.case
        g_kind = 1 if case.kind == "shrink" else 0
        st["stopped"] = 0
        tau, steps, bt = _f(st["tau_next"]), 0, 0
        while steps < max_steps and not st["stopped"]:
            xi, ti, bi, pc, gc, zc, _ = self.roles
            X = lambda q: self.perm[q]
            P = lambda q: self.perm[3 + q]
            x0, g0, xacc0, zacc0 = self.nb[X(xi)], self.G[gc], self.nb[P(pc)], self.Z[zc]
            sums, v = attempt(self.A, self.b, x0, g0, xacc0, zacc0, tau, lambda rdot: fc_alpha(o, st["alpha1"], rdot)[2], bool(o.accelerate),
                              case.kind, self.loss, self.dtype, self.magnitudes)
            if self.on_attempt:
                self.on_attempt(self, x0, g0, xacc0, zacc0, tau, v["coef"], sums, v)
            sums = [float(s) for s in sums]
            self.last = v
            self.all_sums.append((sums, float(tau), bt, dict(st), list(self.fwin)))
            self.xhat, self.nb[P(pc ^ 1)], self.Z[zc ^ 1], self.G[gc ^ 1] = v["xhat"], v["xprox"], v["z"], v["g1"]
            if o.accelerate:
                self.nb[X(ti)] = v["x1"]
            lsq = self.loss == "lsq"
            if fc_backtrack(o, self.fwin, st["iteration"], fc_f(lsq, sums[0]), sums[1], sums[2], tau, bt):
                tau = tau * _f(o.stepsize_shrink)
                bt += 1
                continue
            d = fc_decide(o, lsq, g_kind, PROX[case.kind][1], sums, tau, bt, st["alpha1"], st["max_residual"], st["best_quality"])
            self.history.append(d["record"])
            self.retries.append(bt)
            self.fwin[(st["iteration"] + 1) % WINDOW_MAX] = float(d["f1"])
            st.update(tau_next=float(d["tau_next"]), alpha1=float(d["alpha1"]), max_residual=float(d["max_residual"]),
                      best_quality=float(d["best_quality"]), iteration=st["iteration"] + 1, backtracks=st["backtracks"] + bt)
            self.roles, self.perm = fc_rotate(bool(o.accelerate), d["better"], self.roles, self.perm)
            tau, bt = _f(d["tau_next"]), 0
            steps += 1
            if d["stop"]:
                st["stopped"] = 1
        return steps

    def vectors(self):
        """What fh_get_vector returns after the launch (csrc/fh_host_ctx.h: vec_ptr); None = a buffer nothing has written yet."""
        xi, ti, bi, pc, gc, zc, last_accel = self.roles
        X = lambda q: self.nb[self.perm[q]]
        P = lambda q: self.nb[self.perm[3 + q]]
        return {"X0": X(xi), "G0": self.G[gc], "XHAT": self.xhat, "XPROX": P(pc ^ 1), "X1": X(ti) if last_accel else P(pc ^ 1),
                "G1": self.G[gc ^ 1], "BEST": X(bi), "Z": self.Z[zc ^ 1]}


def launches_of(case):
    """max_steps a test asks for: the compared iterations -- two more where the stop rule has to end the launch before them"""
    return case.steps + (2 if case.ctl == "stop" else 0)


@functools.lru_cache(maxsize=None)
def model(case):
    """The float64 model of a case's launch, computed once and shared (read-only)."""
    mdl = Model(case)
    mdl.steps_done = mdl.run(launches_of(case))
    for v in mdl.vectors().values():
        if v is not None:
            v.setflags(write=False)
    return mdl


CONTROLLER_PATHS = ("two retries or more in one iteration", "accepted at bt == max_backtracks", "ended by max_steps", "ended by the stop rule",
                    "accepted but not better", "window == 1", "window > 1", "second iteration in the launch")


def controller_paths(case, mdl):
    """The controller's paths inside a launch that the model of `case` takes (the launch of launches_of(case) steps)."""
    records = mdl.history
    return {
        "two retries or more in one iteration": any(r >= 2 for r in mdl.retries),
        "accepted at bt == max_backtracks": any(r == mdl.o.max_backtracks for r in mdl.retries),
        "ended by max_steps": mdl.steps_done == launches_of(case) and not mdl.st["stopped"],
        "ended by the stop rule": mdl.st["stopped"] == 1 and mdl.steps_done < launches_of(case),
        "accepted but not better": any(int(r[7]) & 1 == 0 for r in records),
        "window == 1": case.window == 1,
        "window > 1": case.window > 1 and len(records) > 1,
        "second iteration in the launch": len(records) > 1,
    }


def compared_outputs(mdl):
    """Everything the GPU tier compares, flattened: history, state on exit, f_window, vectors."""
    out = [np.ravel(mdl.history), np.array([mdl.st[k] for k in STATE_FIELDS], dtype=np.float64), np.array(mdl.fwin)]
    out += [v for v in mdl.vectors().values() if v is not None]
    return out


# ---- the proof: the same attempt in integer arithmetic -------------------------------------------------------------------------------------------
LIMIT = 1 << 62


class NotExact(AssertionError):
    pass


def _need(ok, what):
    if not ok:
        raise NotExact(what)


def _imax(N):
    return int(np.abs(N).max()) if N.size else 0


def _shl(N, k):
    _need(k >= 0 and (_imax(N) << k) < LIMIT, "shift leaves 62 bits")
    return N * np.int64(1 << k)


def _dot(a, b, bits, where):
    """exact sum of the products a * b after the condition (each factor first freed of its vector's common trailing zeros)"""
    ta, tb = _tz(a), _tz(b)
    a, b = a >> ta, b >> tb
    _need(_imax(a) * _imax(b) < LIMIT, f"{where}: a product leaves 62 bits")
    return _sum(a * b, bits, where) << (ta + tb)


def _tz(N):
    v = int(np.bitwise_or.reduce(np.abs(np.ravel(N)))) if N.size else 0
    return (v & -v).bit_length() - 1 if v else 0


class Bits:
    """the most bits any sum (or element) of the proof needed: sum|terms| / (common lsb of the terms)"""

    def __init__(self):
        self.worst, self.where = 0, ""

    def note(self, bits, where):
        if bits > self.worst:
            self.worst, self.where = bits, where
        _need(bits <= 53, f"{where} needs {bits} bits")


def _sum(T, bits, where):
    """exact sum of the int64 terms T, after the condition sum|terms| / lsb < 2^53"""
    _need(_imax(T) * max(T.size, 1) < LIMIT, f"{where}: the magnitudes leave 62 bits")
    bits.note((int(np.abs(T).sum()) >> _tz(T)).bit_length(), where)
    return int(T.sum())


def _elements(N, bits, where):
    """every element representable: |element| / (its own lowest set bit) < 2^53, bounded here by the vector's common lsb"""
    bits.note((_imax(N) >> _tz(N)).bit_length(), where)
    return N


def _matvec(Ai, N, bits, where):
    """Ai @ N with every row's sum|terms| / lsb < 2^53"""
    mag = np.abs(Ai) @ np.abs(N)
    _need(_imax(mag) < LIMIT and _imax(N) * Ai.shape[1] < LIMIT, f"{where}: the magnitudes leave 62 bits")
    bits.note((_imax(mag) >> _tz(N)).bit_length(), where)
    return Ai @ N


def _ints(v, s):
    """float64 multiples of 2^-s as int64 numerators"""
    N = np.rint(np.asarray(v, dtype=np.float64) * 2.0 ** s)
    _need(np.array_equal(N * 2.0 ** -s, v) and _imax(N) < 2 ** 53, f"not a multiple of 2^-{s}")
    return N.astype(np.int64)


def _scale_of(*vs):
    """the least s with every entry of the float64 vectors a multiple of 2^-s"""
    s = 0
    for v in vs:
        v = np.asarray(v, dtype=np.float64)
        while not np.array_equal(np.rint(v * 2.0 ** s) * 2.0 ** -s, v):
            s += 1
            _need(s < 200, "not dyadic")
    return s


def prove_attempt(Ai, b, x0, g0, xacc0, zacc0, tau, coef, accelerate, kind, bits):
    """The attempt of `attempt()` over the integers: every operand as int64 numerators over a common power of two.  Raises NotExact unless
    every product is exact and every sum satisfies sum|terms| / lsb < 2^53; returns (sums as float64, vectors as float64) -- what ANY order of
    summation and any fusing of multiply-adds gives in float64 arithmetic."""
    k = -int(round(math.log2(tau)))
    _need(2.0 ** -k == tau, "tau is a power of two")
    # the coefficient as cn / 2^cq (any dyadic number; 0 and -1, what the loop's accelerated cases enter with, have cq = 0): what it multiplies moves
    # to a scale cq bits finer
    cq = _scale_of(np.array([coef])) if accelerate else 0
    cn = int(round(coef * 2.0 ** cq)) if accelerate else 0
    _need(abs(cn) < (1 << 20), "the coefficient is a short dyadic number")
    _, mu, lo, hi = PROX[kind]
    xa_f = xacc0 if accelerate else np.zeros_like(x0)
    s0 = _scale_of(x0, g0, xa_f, np.array([lo, hi]))
    S = s0 + max(k, 0)                                            # n side: multiples of 2^-S
    X0, G0, XA = (_shl(_ints(v, s0), S - s0) for v in (x0, g0, xa_f))
    TG = _shl(_ints(g0, s0), S - s0 - k) if k >= 0 else _shl(G0, -k)      # tau * g0: exact, a shift
    XH = _elements(X0 - TG, bits, "xhat")
    one = 1 << S
    THR, LO, HI = (one >> k) if k >= 0 else (one << -k), int(lo * one), int(hi * one)
    XP = {"shrink": lambda: np.sign(XH) * np.maximum(np.abs(XH) - int(mu) * THR, 0), "nonneg": lambda: np.maximum(XH, 0),
          "box": lambda: np.minimum(np.maximum(XH, LO), HI), "identity": lambda: XH.copy()}[kind]()
    DX, DH = _elements(XP - X0, bits, "xprox - x0"), _elements(XP - XH, bits, "xprox - xhat")
    sm = {}
    sm["DXG0"] = _dot(DX, G0, bits, "<dx, g0>")
    sm["DX2"] = _dot(DX, DX, bits, "|dx|^2")
    sm["XH2"] = _dot(DH, DH, bits, "|xprox - xhat|^2")
    sm["G02"] = _dot(G0, G0, bits, "|g0|^2")
    sm["GSUM"], sm["GMAX"] = _sum(np.abs(XP), bits, "sum |xprox|"), _imax(XP)
    sm["RDOT"] = _dot(X0 - XP, _elements(XP - XA, bits, "xprox - x_accel0"), bits, "restart dot")
    # m side: multiples of 2^-Sz
    sb = _scale_of(b, zacc0)
    Sz = max(S, sb)
    Z = _shl(_matvec(Ai, XP, bits, "z = A xprox"), Sz - S)
    B, ZA = _shl(_ints(b, sb), Sz - sb), _shl(_ints(zacc0, sb), Sz - sb)
    Sr, ZX = Sz + cq, Z                                      # the extrapolated z, the residual and g1: multiples of 2^-Sr
    if accelerate:
        D = _elements(Z - ZA, bits, "z - z_accel0")
        ZX = _elements(_shl(Z, cq) + cn * D, bits, "extrapolated z")
    R, RX = _elements(Z - B, bits, "z - b"), _elements(ZX - _shl(B, cq), bits, "residual")
    sm["FSQ"] = _dot(R, R, bits, "|z - b|^2")
    sm["FSQ_ADJ"] = _dot(RX, RX, bits, "|zx - b|^2") if accelerate else 0
    G1 = _matvec(Ai.T, RX, bits, "g1 = A^T r")              # multiples of 2^-Sr
    # phase B at scale Sb = max(Sz, S - k ... ) : dg = g1 + (xhat - x0) / tau
    Sq = S - k                                               # (xhat - x0) / tau = -g0: multiples of 2^-(S - k) -- exact, a shift
    Sb = max(Sr, Sq, S)
    DGq = _shl(XH - X0, Sb - Sq)
    DG = _elements(_shl(G1, Sb - Sr) + DGq, bits, "dg")
    S1, X1 = S + cq, XP                                      # x1: multiples of 2^-S1
    if accelerate:
        D = _elements(XP - XA, bits, "xprox - x_accel0")
        X1 = _elements(_shl(XP, cq) + cn * D, bits, "x1")
    DH1 = _elements(X1 - _shl(XH, cq), bits, "x1 - xhat")
    DXb = _shl(DX, Sb - S)
    sm["DXDG"] = _dot(DXb, DG, bits, "<dx, dg>")
    sm["DG2"] = _dot(DG, DG, bits, "|dg|^2")
    sm["XH2_ADJ"] = _dot(DH1, DH1, bits, "|x1 - xhat|^2")
    sm["GSUM_ADJ"], sm["GMAX_ADJ"] = _sum(np.abs(X1), bits, "sum |x1|"), _imax(X1)
    scale = {"FSQ": 2 * Sz, "FSQ_ADJ": 2 * Sr, "DXG0": 2 * S, "DX2": 2 * S, "XH2": 2 * S, "G02": 2 * S, "GSUM": S, "GMAX": S, "RDOT": 2 * S,
             "DXDG": 2 * Sb, "DG2": 2 * Sb, "XH2_ADJ": 2 * S1, "GSUM_ADJ": S1, "GMAX_ADJ": S1}
    sums = [math.ldexp(sm[name], -scale[name]) for name in SUMS]      # (representable: |sum| <= sum|terms|, a multiple of the same lsb)
    vec = lambda N, s: np.ldexp(N.astype(np.float64), -s)
    return sums, dict(xhat=vec(XH, S), xprox=vec(XP, S), z=vec(Z, Sz), g1=vec(G1, Sr), x1=vec(X1, S1))


def prove(case, steps=None):
    """Run the case's launch with every attempt redone in integer arithmetic and compared with the float64 attempt.  Returns
    (iterations proven exact, worst bits, where); raises nothing: an attempt that fails the condition ends the count."""
    A = operands(case)[0]
    Ai, bits, state = A.astype(np.int64), Bits(), dict(failed=None)

    def check(mdl, x0, g0, xacc0, zacc0, tau, coef, sums, v):
        if state["failed"] is not None:
            return
        try:
            isums, iv = prove_attempt(Ai, mdl.b, x0, g0, xacc0, zacc0, float(tau), float(coef), bool(mdl.o.accelerate), case.kind, bits)
            _need([float(s) for s in sums] == isums, f"float64 sums differ from the integers': {[n for n, a, c in zip(SUMS, sums, isums) if float(a) != c]}")
            for name in iv:
                _need(np.array_equal(iv[name], v[name]), f"float64 {name} differs from the integers'")
        except NotExact as exc:
            state["failed"] = (len(mdl.history), str(exc))

    mdl = Model(case, on_attempt=check)
    mdl.run(case.steps if steps is None else steps)
    proven = len(mdl.history) if state["failed"] is None else state["failed"][0]
    return proven, bits.worst, bits.where, state["failed"]
