"""Cases, claimed geometry, exact operands and the models for the tests of EVERY instantiation and path of the one-pass dense kernels
(csrc/fh_fused.h + fh_fused_body.inc: k_fused_dense, what fh_step / fh_step_accel launch; csrc/fh_setup.h: k_setup_dense, fh_setup's one-read
launch).  A plain helper module, the sibling of tests/run_paths.py, whose machinery it reuses (attempt, prove_attempt, Bits, NotExact, PROX): the
CPU tier (tests/test_fused_paths_cpu.py) proves every condition claimed here, the GPU tier (tests/test_gpu_fused_paths.py) runs the kernels.

Geometry.  Which instantiation, how many teams, how many rows each and how the finaliser splits the columns depend on the CUs the launch takes,
on the rows-per-team floor and on the scheduling word; every case pins all three (FH_TUNE_FUSED_CUS -- at most 64 but for a few pins the GPU tier
checks the device against -- and both halves of FH_TUNE_FUSED_VARIANT), states the geometry it expects (expected_shape, the host's rule restated from the case's own numbers) and both tiers compare
that with the library's own rule (fh_fused_launch_shape_for / fh_setup_shape_for, what the launchers call; the GPU tier asks the context).  The
"whole device" cases (cus = 0) are the exception: teams of 8 and more members reach one row per team, or a grid above 256, only on more than 64
CUs; the GPU tier computes their expectation from the CU count the device reports, the CPU tier takes DEVICE_CUS.

Exactness.  A holds -1, 0, 1 (a quarter of the entries non-zero, fewer in the wide rows), x0 multiples of 1/2 in [-2, 2], b = A x0 + noise of
multiples of 1/2, tau = 1/2, mu = 1, the box [2^-6, 2], the FISTA coefficient 1/2: every product of a launch is exact and every sum stays below 2^53
of its terms' common lsb, whatever the order of summation and whichever multiply-adds are fused -- the CPU tier proves that in integer arithmetic
(run_paths.prove_attempt, prove_setup here) -- so scalars and vectors must EQUAL the model's.  Only the logistic loss is not exact."""
import collections
import functools
import os
import re

import numpy as np

from fasta_python_amd import hip
from tests import run_paths as RP

FH_WG = 256                                          # csrc/fh_device.h
DEVICE_CUS = 256                                     # MI355X: what the CPU tier assumes of the whole-device cases
TAU, COEF = 0.5, 0.5
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fasta_python_amd", "csrc")
KINDS = ("shrink", "box", "nonneg", "identity")
MODES = ("plain", "accel", "restart_hi", "restart_lo")     # accel: restart off; restart_hi: restart on, the dot above 1e-30 (coefficient dropped); _lo: below
WORDS = (34, 2, 0, 38)                               # scheduling words: bit 2 members one XCD apart, 4 no sleep between polls, 32 rows dealt cyclically

# what: "step" | "setup"; cus: CUs the launch is pinned to (0 = the whole device); floor: rows-per-team floor (0 = none); variant: the low half of
# FH_TUNE_FUSED_VARIANT (None = not set: the host resolves the cyclic bit, the floor stays 16); dens: one entry in `dens` of A is non-zero
Case = collections.namedtuple("Case", "name what m n storage cus floor variant mode kind loss dens")


def round_up(v, k):
    return (v + k - 1) // k * k


def cdiv(a, b):
    return -(-a // b)


# ---- the instance tables, parsed (never restated) --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fused_table():
    """rows of csrc/fh_fused_instances.inc as (PPT, PIPE, TEAM, XLDS, NBO, F32)"""
    text = re.sub(r"//.*", "", open(os.path.join(CSRC, "fh_fused_instances.inc")).read())
    return tuple(tuple(int(v) for v in args.split(",")) for args in re.findall(r"FUSED_INST_\d\(([^)]*)\)", text))


@functools.lru_cache(maxsize=None)
def setup_table():
    """rows of csrc/fh_setup_instances.inc as (MPP, PIPE, TEAM, threads, NR, F32): group 2 is the float32-storage group"""
    text = re.sub(r"//.*", "", open(os.path.join(CSRC, "fh_setup_instances.inc")).read())
    return tuple(tuple(int(v) for v in args.split(",")) + (1 if group == "2" else 0,) for group, args in re.findall(r"SETUP_INST_(\d)\(([^)]*)\)", text))


# ---- the host's rule, restated from a case's own numbers -------------------------------------------------------------------------------------
def step_key(n, f32, word, ncu):
    """csrc/fh_host_launch.h:fused_shape_for -> (PPT, PIPE, TEAM, XLDS, NBO) or None"""
    pieces = round_up(n, 32) // 4 if f32 else round_up(n, 16) // 2
    key = None
    if f32:
        for team in (1, 2, 4, 8, 16):
            if pieces > team * FH_WG * 8:
                continue
            ppt = cdiv(pieces, team * FH_WG)
            ppt = 4 if ppt == 3 else ppt
            key = (ppt, 1, team, 1, 4 if ppt <= 6 else 3) if ppt >= 5 else (ppt, 1, team, 0, 0)
            if ppt == 8 and team in (4, 8) and not word & 8 and ncu % (2 * team) == 0:
                key = (4, 1, 2 * team, 0, 4)
            break
    elif pieces <= FH_WG * 8 and not word & 8:
        ppt = cdiv(pieces, FH_WG)
        key = (4 if ppt == 3 else ppt, 1, 1, 0, 0)
    elif pieces <= 2 * FH_WG * 8 and not word & 8:
        key = (cdiv(pieces, 2 * FH_WG), 1, 2, 0, 0)
    elif pieces <= 4 * FH_WG * 8 and not word & 8:
        key = (cdiv(pieces, 4 * FH_WG), 1, 4, 0, 0)
    elif pieces <= 8 * FH_WG * 8:
        ppt = cdiv(pieces, 8 * FH_WG)
        key = (4 if ppt == 3 else ppt, 1, 8, 0, 0)
    elif pieces == 8 * FH_WG * 16 and word & 8:
        key = (16, 0, 8, 0, 0)
    elif pieces <= 16 * FH_WG * 8:
        key = (cdiv(pieces, 16 * FH_WG), 2, 16, 0, 0)
    elif pieces <= 16 * FH_WG * 16:
        ppt = cdiv(pieces, 16 * FH_WG)
        key = (16, 0, 16, 0, 0) if word & 16 else (ppt, 1, 16, 1, 4 if ppt <= 10 else 3)
    elif pieces <= 32 * FH_WG * 16:
        ppt = cdiv(pieces, 32 * FH_WG)
        key = (ppt, 1, 32, 1, 4 if ppt <= 10 else 3)
    if key is None or ncu < key[2] or ncu % key[2]:
        return None
    return key


def setup_key(m, n, f32, word, ncu):
    """csrc/fasta_hip.hip:setup_entry_for -> (MPP, PIPE, TEAM, threads, NR, F32) or None"""
    if not (n >= 16384 or m * n >= 1 << 23):
        return None
    if f32:
        pieces = round_up(n, 32) // 4
        for team in (1, 2, 4, 8, 16):
            if pieces > team * FH_WG * 4:
                continue
            if ncu % team:
                return None
            mpp = cdiv(pieces, team * FH_WG)
            mpp = 4 if (mpp == 3 or team > 1) else mpp
            return (mpp, 1, team, 256, 2, 1)
        return None
    key = step_key(n, 0, word, ncu)
    if key is None or key[3]:
        return None
    ppt, pipe, team = key[:3]
    threads = 512 if (ppt == 8 and team in (8, 16) and not word & 16) else 256
    want = (ppt, 1 if team == 1 else pipe, team, threads, 2, 0)
    if want in setup_table():
        return want
    return (ppt, want[1], team, 256, 2, 0) if threads == 512 else None


def word_of(case):
    return 34 if case.variant is None else case.variant


def floor_of(case):
    return 16 if case.variant is None else case.floor


def cus_of(case, device_cus=DEVICE_CUS):
    return case.cus or device_cus


def expected_shape(case, device_cus=DEVICE_CUS):
    """The hip.FusedLaunchShape / hip.SetupShape a case must be launched with, from the case's own numbers."""
    f32, word, ncu, floor = int(case.storage == "f32"), word_of(case), cus_of(case, device_cus), floor_of(case)
    mp = round_up(case.m, 16)
    ld2 = round_up(case.n, 32) // 4 if f32 else round_up(case.n, 16) // 2
    if case.what == "step":
        ppt, pipe, team, xlds, nbo = step_key(case.n, f32, word, ncu)
        wpc = 2 if (f32 and team >= 8 and ppt == 4 and not xlds) else 1
    else:
        ppt, pipe, team, threads, nr, _ = setup_key(case.m, case.n, f32, word, ncu)
        wpc = 1
    nteams = ncu * wpc // team
    if floor:
        nteams = min(nteams, max(8, round_up(cdiv(mp, floor), 8)))
    rpt = cdiv(mp, nteams)
    auto = case.variant is None
    variant = word & ~32 if ((auto and rpt < 128) or (auto and f32 and case.what == "setup")) else word
    tail = (wpc, nteams, rpt, nteams * team, variant, ld2, ld2 * (2 if f32 else 1))
    if case.what == "step":
        return hip.FusedLaunchShape(ppt, pipe, team, xlds, nbo, f32, *tail)
    return hip.SetupShape(ppt, pipe, team, threads, nr, f32, *tail)


def shape_query(case, device_cus=DEVICE_CUS):
    """the library's own rule in its pure form, with the numbers tuning_of() sets"""
    fn = hip.fused_launch_shape_for if case.what == "step" else hip.setup_shape_for
    return fn(case.m, case.n, case.storage, word_of(case), case.variant is None, cus_of(case, device_cus), floor_of(case))


def tuning_of(case):
    t = {}
    if case.cus:
        t[hip.TUNE_FUSED_CUS] = case.cus
    if case.variant is not None:
        t[hip.TUNE_FUSED_VARIANT] = ((case.floor or 0xFFFF) << 16) | case.variant
    return t


def row_of(sh):
    """the row of the instance table a shape launches"""
    return tuple(sh[:6])


# ---- what the kernels derive from the shape, each with the line it mirrors ---------------------------------------------------------------------
def is_setup(sh):
    return isinstance(sh, hip.SetupShape)


def nb_of(sh):
    """row buffers: fh_fused_body.inc `constexpr int NB = NBO ? NBO : ...`; fh_setup.h `constexpr int NB = F32 ? ... `"""
    if is_setup(sh):
        ppt = cdiv(sh.MPP * FH_WG, sh.threads)              # pieces per lane
        if sh.F32:
            return 4 if ppt >= 4 else 6
        return 4 if sh.threads == 512 else ((5 if (sh.NR == 2 and sh.PIPE >= 2) else 4) if ppt >= 7 else (5 if ppt >= 5 else 6))
    if sh.NBO:
        return sh.NBO
    if sh.TEAM == 1:
        return 5 if sh.PPT >= 8 else 6
    return 3 if not sh.PIPE else (3 if sh.PPT >= 16 else (5 if sh.PPT >= 8 else 6))


def preload_of(sh):
    """fh_fused_body.inc `constexpr bool PRELOAD = TEAM <= 8 && !XLDS && PPT <= 8` (the set-up kernel never preloads)"""
    return (not is_setup(sh)) and sh.TEAM <= 8 and not sh.XLDS and sh.PPT <= 8


def distance_of(sh):
    """rows between a post and its poll (`constexpr int D = PIPE`); a team of one exchanges nothing"""
    return sh.PIPE if sh.TEAM > 1 else 0


def team_rows(sh, mp, t):
    """rows of A team t works on (`row_base`, `row_step`, `r_end`, `grow`): blocked unless variant bit 32"""
    if sh.variant & 32:
        return list(range(t, mp, sh.nteams))
    base = min(t * sh.rows_per_team, mp)
    return list(range(base, min(base + sh.rows_per_team, mp)))


def r_ends(sh, mp):
    if sh.variant & 32:
        return [cdiv(mp - t, sh.nteams) if t < mp else 0 for t in range(sh.nteams)]
    return [min(min(t * sh.rows_per_team, mp) + sh.rows_per_team, mp) - min(t * sh.rows_per_team, mp) for t in range(sh.nteams)]


def finaliser_of(sh):
    """(share, slices, tps, trips): `share = (nv2 + gridDim.x - 1) / gridDim.x`, `slices = share < FH_WG ? min(FH_WG / max(share, 1), nteams) : 1`,
    `tps = (nteams + slices - 1) / slices`, the `t0` loop"""
    share = cdiv(sh.nv2, sh.grid)
    slices = min(FH_WG // max(share, 1), sh.nteams) if share < FH_WG else 1
    return share, slices, cdiv(sh.nteams, slices), cdiv(share, FH_WG)


def pieces_per_member(sh):
    return FH_WG * sh[0]


def member_columns(sh, n, mem):
    """columns [lo, hi) of member `mem` (`c0 = mem * (FH_WG * PPT) + tid`); empty for a member that is clamped entirely"""
    e = 4 if sh.F32 else 2
    lo = mem * pieces_per_member(sh) * e
    return min(lo, n), min(lo + pieces_per_member(sh) * e, n)


ROW_PATHS = ("team with no rows", "r_end == 1", "r_end <= PIPE", "r_end < NB - 1", "r_end % NB != 0", "several trips", "uneven last team",
             "padding rows in a live team", "team of padding rows only")
COLUMN_PATHS = ("all lanes live", "clamped lanes", "odd n", "f32: n % 4 != 0 and n % 32 != 0", "idle piece", "idle members")
FIN_PATHS = ("slices > 1, last slice cut", "slices == 1, one trip", "slices == 1, several trips", "share beyond nv2", "grid > 256")


def paths_of(sh, m, n):
    """The paths a launch geometry `sh` (hip.FusedLaunchShape or hip.SetupShape) of an (m, n) matrix runs, as a dict of booleans."""
    mp = round_up(m, 16)
    ends = r_ends(sh, mp)
    live = [r for r in ends if r]
    nb, dist = nb_of(sh), distance_of(sh)
    teams = [team_rows(sh, mp, t) for t in range(sh.nteams)] if sh.nteams <= 4096 else []
    share, slices, tps, trips = finaliser_of(sh)
    e = 4 if sh.F32 else 2
    need = cdiv(sh.ld2, FH_WG * sh.TEAM)
    return {
        "team with no rows": 0 in ends,
        "r_end == 1": 1 in ends,
        "r_end <= PIPE": dist > 0 and any(r <= dist for r in live),
        "r_end < NB - 1": any(r < nb - 1 for r in live),
        "r_end % NB != 0": any(r % nb for r in live),
        "several trips": any(r > nb for r in live),
        "uneven last team": len(live) > 1 and live[-1] < live[0],
        "padding rows in a live team": any(rows and rows[0] < m <= rows[-1] for rows in teams),
        "team of padding rows only": any(rows and min(rows) >= m for rows in teams),
        "all lanes live": n == e * pieces_per_member(sh) * sh.TEAM,
        "clamped lanes": sh.ld2 < pieces_per_member(sh) * sh.TEAM,
        "odd n": n % 2 == 1,
        "f32: n % 4 != 0 and n % 32 != 0": bool(sh.F32) and n % 4 != 0 and n % 32 != 0,
        "idle piece": need < sh[0],
        "idle members": (sh.TEAM - 1) * pieces_per_member(sh) >= sh.ld2,
        "slices > 1, last slice cut": slices > 1 and slices * tps > sh.nteams,
        "slices == 1, one trip": slices == 1 and trips == 1,
        "slices == 1, several trips": slices == 1 and trips > 1,
        "share beyond nv2": (sh.grid - 1) * share >= sh.nv2,
        "grid > 256": sh.grid > 256,
    }


FORMS = ("TEAM 1", "in line", "one ahead", "two ahead", "x in LDS", "float32", "two per CU")


def form_of(sh):
    """the loop form of the body a step shape runs"""
    if sh.wpc == 2:
        return "two per CU"
    if sh.F32:
        return "float32"
    if sh.TEAM == 1:
        return "TEAM 1"
    if not sh.PIPE:
        return "in line"
    if sh.XLDS:
        return "x in LDS"
    return "two ahead" if sh.PIPE == 2 else "one ahead"


# (form, path) -> why no launch on at most 256 CUs reaches it; tests/test_fused_paths_cpu.py searches the geometries for each and finds none
UNREACHABLE = {
    ("TEAM 1", "r_end <= PIPE"): "a team of one posts nothing ahead",
    ("TEAM 1", "grid > 256"): "one workgroup per CU",
    ("in line", "r_end <= PIPE"): "PIPE = 0: nothing is posted ahead",
    ("in line", "slices > 1, last slice cut"): "nv2 >= 32768: a share below 129 pairs needs 256 workgroups, i.e. 32 or 16 teams, which 2 slices divide",
    ("in line", "grid > 256"): "one workgroup per CU",
    ("one ahead", "grid > 256"): "one workgroup per CU",
    ("two ahead", "grid > 256"): "one workgroup per CU",
    ("x in LDS", "slices > 1, last slice cut"): "nv2 > 32768 on at most 256 workgroups: a share above 128 pairs, one slice",
    ("x in LDS", "grid > 256"): "one workgroup per CU",
    ("float32", "grid > 256"): "one workgroup per CU",
}


# ---- the case list -----------------------------------------------------------------------------------------------------------------------------
# row geometries (m, teams): what each is for is asserted through paths_of (ROW_CLAIMS of the CPU tier), not trusted.  mp = round_up(m, 16).
ROWS = collections.OrderedDict([
    ("one_row_last", (16, 6)),       # mp = 16 on 6 teams, blocked: 3, 3, 3, 3, 3 and 1 row
    ("one_each", (13, 16)),          # one row per team under both dealings, three teams of padding rows only
    ("some_empty", (16, 20)),        # 16 teams of one row, 4 without rows under both dealings
    ("empty_last", (16, 5)),         # blocked: 4, 4, 4, 4, 0
    ("pairs", (11, 8)),              # two rows each; blocked: a live and a padding row in team 5, teams 6 and 7 own padding only
    ("uneven", (20, 5)),             # mp = 32: 7, 7, 7, 7, 4 blocked (row 20, padding, inside team 2's live range); 7, 7, 6, 6, 6 cyclic
    ("long", (50, 3)),               # mp = 64: 22, 22, 20
    ("single", (20, 1)),             # one team of 32 rows
    ("tall", (40, 1)),               # mp = 48: one team of 48 rows
    ("halves", (40, 2)),             # mp = 48: 24 and 24, the padding rows behind team 1's live ones (blocked) or in both (cyclic)
    ("three", (20, 3)),              # mp = 32: 11, 11, 10; team 1 ends in padding rows, team 2 (blocked) owns padding only
])


def widths_of(row):
    """(tag, n) per table row: the full width, a ragged one (odd; float32 storage: n % 4 and n % 32 non-zero) near the shape's lower end -- lanes
    clamped, the 3-piece rows that take the 4-piece shape, members without columns where the shape has such widths"""
    ppt, pipe, team, xlds, nbo, f32 = row
    e = 4 if f32 else 2
    full = e * FH_WG * ppt * team
    if f32 and ppt == 4 and team >= 8 and not xlds:           # two per CU: the 8-piece widths of half the members
        return [("full", full), ("ragged", full - 8 * e * 100 + 3)]
    if not pipe or (ppt == 16 and not xlds and not f32):      # the in-line A/B shapes
        return [("full", full)] if team == 8 else [("full", full), ("ragged", 65536 + 1029)]
    lo_pieces = {1: 0, 2: FH_WG, 4: 2 * FH_WG}.get(ppt, (ppt - 1) * FH_WG) * team       # the widest row the next shape down takes
    if ppt == 5 and team > 1 and not (f32 and team == 1):
        lo_pieces = 8 * FH_WG * (team // 2)                   # below 5 pieces a team is half the size
    if ppt == 9:
        lo_pieces = 8 * FH_WG * 16 if team == 16 else 16 * FH_WG * 16
    ragged = lo_pieces * e + (37 if ppt > 1 or team > 1 else 101)
    return [("full", full), ("ragged", ragged)]


def density(n, kind):
    """one entry in this many of A is non-zero: the widest rows sparser, and the box (whose bound 2^-6 makes every square 12 bits longer) sparser
    again, so that the longest sum -- |dg|^2, which grows as n^2 m / dens^2 -- keeps headroom below 53 bits (the proof decides)"""
    base = 4 if n <= 32768 else (8 if n <= 65536 else (16 if n <= 131072 else 32))
    return base * (4 if (kind == "box" and n > 16384) else 1)


def _pinned_teams(row, wpc):
    """team counts a case can pin on at most 64 CUs"""
    return 64 * wpc // row[2]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    names = [k for k in ROWS if k not in ("three", "tall", "halves")]
    i = 0
    for row in fused_table():
        ppt, pipe, team, xlds, nbo, f32 = row
        wpc = 2 if (f32 and team >= 8 and ppt == 4 and not xlds) else 1
        # the A/B bits that select a row: 8 -- teams of 8 below n = 16384 and in line at n = 65536; float32 storage: the one-per-CU 8-piece shapes
        # of 4 and 8 members, which otherwise run as two workgroups per CU wherever the CU count allows -- and 16 -- 16 members in line
        word_bits = 8 if ((team == 8 and not f32 and (ppt <= 4 or not pipe)) or (f32 and ppt == 8 and team in (4, 8))) else (16 if (not pipe and team == 16) else 0)
        for tag, n in widths_of(row):
            # the next row geometry this team size can pin, the prox kinds, modes and scheduling words in rotation
            for _ in range(len(names)):
                rows = names[i % len(names)]
                m, teams = ROWS[rows]
                i += 1
                if teams <= _pinned_teams(row, wpc) and (wpc == 1 or teams % 2 == 0) and (rows != "long" or n <= 65536):
                    break
            if n > 65536:                                     # the widest rows: 40 rows of them (see operands)
                rows = ("tall", "halves")[len(out) % 2]
                m, teams = ROWS[rows]
            j = len(out)
            word = WORDS[j % 4] | word_bits
            # a ragged width meets the box, the one kind that does not map the padding behind the row's last entry to zero
            kind = "box" if tag == "ragged" else ("shrink", "nonneg", "identity")[(j // 2) % 3]
            out.append(Case(f"{tag}-{rows}", "step", m, n, "f32" if f32 else "f64", teams * team // wpc, 0, word, MODES[(j // 2 + j % 2) % 4], kind, "lsq",
                            density(n, kind)))
    out += _extra_step_cases()
    out += _setup_cases()
    return tuple(out)


def _step(name, m, n, cus, word, mode="plain", kind="box", storage="f64", floor=0, loss="lsq", dens=None):
    dens = dens or density(n, kind)
    return Case(name, "step", m, n, storage, cus, floor, word, mode, kind, loss, dens)


def _extra_step_cases():
    """what the rotation leaves open in the matrix of loop forms x paths, the whole-device cases, the host's own word, the logistic loss"""
    out = [
        # TEAM 1: finaliser corners (share 683: three trips; nv2 = 8 on 6 workgroups: shares beyond it; 11 teams: 2 slices of 6)
        _step("trips-long", 50, 4096, 3, 34, "accel"), _step("beyond-one_row_last", 16, 16, 6, 2, "restart_hi"),
        _step("cut-t11", 11, 2801, 11, 0, "restart_lo"), _step("onetrip-uneven", 20, 2048, 5, 34, "plain", "shrink"),
        # one ahead
        _step("beyond-empty_last", 16, 16, 40, 2 | 8, "accel"), _step("cut-t11", 16, 4207, 22, 34, "plain", "shrink"),
        _step("onetrip-t10", 20, 16001, 40, 0, "restart_hi", "nonneg"), _step("trips-single", 20, 8192, 2, 38, "plain", "identity"),
        _step("plain-one_each", 13, 5001, 32, 34, "restart_lo"), _step("plain-empty_last", 16, 9001, 20, 2, "plain", "shrink"),
        # in line: 8 members at n = 65536 (bit 8), 16 members (bit 16)
        _step("full-one_row_last", 16, 65536, 48, 2 | 8, "accel"), _step("full-empty_last", 16, 65536, 40, 34 | 8, "plain", "shrink"),
        _step("full-uneven", 20, 65536, 40, 0 | 8, "restart_hi", "nonneg"), _step("full-pairs", 11, 65536, 64, 34 | 8, "restart_lo"),
        _step("ragged-three", 20, 70001, 48, 2 | 16, "plain", "identity"), _step("full-single", 20, 131072, 16, 34 | 16, "accel", "shrink"),
        # two ahead (16 members): at most 4 teams on 64 CUs
        _step("ragged-single", 20, 40001, 16, 34), _step("ragged-three", 20, 50001, 48, 2, "accel", "shrink"),
        _step("idlemem-long", 50, 32784 + 1, 48, 34, "restart_hi"),
        # x slice in LDS
        _step("ragged-three", 20, 90001, 48, 34, "accel"), _step("ragged-single", 20, 150001, 32, 2, "restart_lo", "shrink"),
        # float32 storage and two per CU
        _step("cut-t11", 11, 2803, 11, 34, "accel", storage="f32"), _step("beyond-some_empty", 16, 32, 20, 2, "plain", storage="f32"),
        _step("trips-long", 50, 8192, 3, 0, "restart_hi", storage="f32"), _step("ragged-some_empty", 16, 9003, 40, 34, "restart_lo", "shrink", storage="f32"),
        _step("ragged-one_each", 13, 17003, 64, 2, "accel", "nonneg", storage="f32"), _step("ragged-empty_last", 16, 33003, 40, 34, "plain", storage="f32"),
        _step("full-three", 20, 131072, 48, 38, "accel", "shrink", storage="f32"),
        _step("full-pairs", 11, 32768, 32, 34, "restart_hi", storage="f32"), _step("ragged-one_row_last", 16, 65003, 48, 2, "restart_lo", storage="f32"),
        _step("ragged-uneven", 20, 32003, 20, 0, "restart_hi", "shrink", storage="f32"), _step("full-long4", 50, 65536, 32, 34, "plain", "nonneg", storage="f32"),
        # the host's own scheduling word (FH_TUNE_FUSED_VARIANT not set, floor 16): bit 32 cleared below 128 rows per team, kept from there on
        # pins above 64 CUs (the GPU tier requires that many): teams of 16 without rows, one finaliser trip of one slice, a last share beyond nv2,
        # three slices of nine for 26 teams of two workgroups per CU
        _step("plain-empty12", 16, 40001, 192, 2, "accel"), _step("onetrip-pairs", 11, 40001, 128, 34, "plain", "shrink"),
        _step("plain-empty12", 16, 90001, 192, 2, "restart_hi"), _step("beyond-one_each", 13, 65553, 256, 34, "restart_lo"),
        _step("cut-wide26", 20, 32768, 104, 34, "accel", storage="f32"),
        Case("auto-blocked", "step", 300, 5001, "f64", 16, 16, None, "plain", "box", "lsq", 4),
        Case("auto-cyclic", "step", 1100, 2001, "f64", 8, 16, None, "accel", "shrink", "lsq", 4),
    ]
    # the whole device, one per loop form: one row per team (or two, 32 members) with teams without rows, under the cyclic dealing
    out += [_step("whole-TEAM1", 16, 1001, 0, 34, "accel"), _step("whole-inline8", 16, 65536, 0, 34 | 8, "restart_hi"),
            _step("whole-inline16", 13, 65552, 0, 34 | 16, "plain"), _step("whole-one_ahead", 13, 20001, 0, 34, "restart_lo", "shrink"),
            _step("whole-two_ahead", 13, 40001, 0, 34, "accel"), _step("whole-lds16", 13, 131072, 0, 34, "plain", "shrink"),
            _step("whole-lds32", 16, 140001, 0, 34, "accel", "shrink"), _step("whole-f32", 16, 20003, 0, 34, "plain", storage="f32"),
            _step("whole-two_per_cu", 16, 65536, 0, 34, "accel", storage="f32"), _step("whole-two_per_cu_blocked", 13, 60003, 0, 2, "restart_lo", storage="f32")]
    # the logistic loss (not exact): one per loop form, both dealings, padding rows
    out += [_step("logistic-uneven", 20, 3001, 5, 34, "plain", "shrink", loss="logistic"), _step("logistic-uneven", 20, 65536, 40, 2 | 8, "accel", "shrink", loss="logistic"),
            _step("logistic-uneven", 20, 12001, 20, 34, "restart_hi", "shrink", loss="logistic"), _step("logistic-t4", 11, 50001, 64, 2, "plain", "shrink", loss="logistic"),
            _step("logistic-t4", 11, 100001, 64, 34, "accel", "shrink", loss="logistic"),
            _step("logistic-uneven", 20, 12003, 10, 2, "restart_lo", "shrink", storage="f32", loss="logistic"),
            _step("logistic-pairs", 11, 32768, 32, 34, "plain", "shrink", storage="f32", loss="logistic")]
    return out


def _setup_cases():
    """every row of the set-up table, full and ragged: fh_setup takes the one-read kernel from n = 16384 or 2^23 elements on"""
    out = []
    names = [k for k in ROWS if k not in ("single", "three", "tall", "halves")]
    i = 0
    for row in setup_table():
        mpp, pipe, team, threads, nr, f32 = row
        e = 4 if f32 else 2
        full = e * FH_WG * mpp * team
        lo = {1: 0, 2: FH_WG, 4: 2 * FH_WG}.get(mpp, (mpp - 1) * FH_WG) * team
        if f32 and team > 1:
            lo = 4 * FH_WG * (team // 2)
        elif mpp == 5 and team > 1:
            lo = 8 * FH_WG * (team // 2)
        for tag, n in (("full", full), ("ragged", lo * e + (37 if lo else 101))):
            word = WORDS[len(out) % 4] | (16 if (threads == 256 and mpp == 8 and team in (8, 16) and not f32) else 0)
            if n >= 16384:
                for _ in range(len(names)):
                    rows = names[i % len(names)]
                    i += 1
                    if ROWS[rows][1] <= 64 // team:
                        break
                m, teams = ROWS[rows]
            else:
                m = cdiv(1 << 23, n) + 3
                m += 5 if m % 16 == 0 else 0                   # (padding rows behind the last one)
                teams = (5, 6, 3, 16)[len(out) % 4]
                teams = min(teams, 64 // team)
                rows = f"many{teams}"
            out.append(Case(f"{tag}-{rows}", "setup", m, n, "f32" if f32 else "f64", teams * team, 0, word, "plain", "shrink", "lsq", 4))
    return out


def case_id(c):
    sh = expected_shape(c)
    key = "x".join(str(v) for v in row_of(sh))
    return f"{c.what}-{key}-{c.name}-{c.m}x{c.n}-cus{c.cus or 'all'}-w{'auto' if c.variant is None else c.variant}-{c.mode}-{c.kind}" + ("-logistic" if c.loss != "lsq" else "")


def step_cases():
    return tuple(c for c in cases() if c.what == "step")


def exact_step_cases():
    return tuple(c for c in cases() if c.what == "step" and c.loss == "lsq")


def logistic_cases():
    return tuple(c for c in cases() if c.loss == "logistic")


def setup_cases():
    return tuple(c for c in cases() if c.what == "setup")


# ---- operands ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def matrix(m, n, dens, seed=0):
    """float64 (m, n) of -1, 0, 1 with one entry in `dens` non-zero, no empty row or column"""
    rng = np.random.RandomState(7100 + 31 * m + n + 1009 * seed)
    A = (rng.randint(0, 2, size=(m, n), dtype=np.int8) * 2 - 1) * (rng.randint(0, dens, size=(m, n), dtype=np.int8) == 0)
    empty = np.flatnonzero(~A.any(axis=0))                    # (random signs: a sparse matrix has many, and equal signs would add up coherently)
    A[(empty * 7 + seed) % m, empty] = rng.randint(0, 2, size=empty.size) * 2 - 1
    for i in np.flatnonzero(~A.any(axis=1)):
        A[i, i % n] = -1
    A = A.astype(np.float64)
    A.setflags(write=False)
    return A


def _halves(rng, lo, hi, size):
    return rng.randint(lo, hi + 1, size=size) * 0.5


def required_rows(case, sh):
    """live rows whose gradient factor must be non-zero: row m - 1, the first and the last live row of every team's range"""
    mp = round_up(case.m, 16)
    need = {case.m - 1}
    for t in range(sh.nteams):
        live = [r for r in team_rows(sh, mp, t) if r < case.m]
        if live:
            need |= {live[0], live[-1]}
    return sorted(need)


def required_pieces(case, sh):
    """column ranges in which xprox must hold a non-zero: the row's last live piece, each member's first and last live piece"""
    e = 4 if sh.F32 else 2
    out = [((case.n - 1) // e * e, case.n)]
    for mem in range(sh.TEAM):
        lo, hi = member_columns(sh, case.n, mem)
        if lo < hi:
            out += [(lo, min(lo + e, hi)), ((hi - 1) // e * e, hi)]
    return out


State = collections.namedtuple("State", "A b x0 g0 xacc0 zacc0 labels")


@functools.lru_cache(maxsize=4)
def operands(case):
    """The entering state of a step case (State), by the recipe of tests/sparse_lanes.py:step_operands: x0 multiples of 1/2 in [-2, 2],
    b = A x0 + noise of multiples of 1/2 (two thirds zero), g0 = A^T (A x0 - b); accelerated cases enter with x_accel0 = x0 + multiples of 1/2 and
    z_accel0 = A x_accel0.  Entries that would leave a compared output insensitive are drawn again (x0 where xprox must not vanish; the whole
    draw where a row's gradient factor must not)."""
    assert case.what == "step"
    sh = expected_shape(case)
    accel = case.mode != "plain"
    for seed in range(40):
        A = matrix(case.m, case.n, case.dens, seed // 8)
        rng = np.random.RandomState(9100 + case.m + 3 * case.n + 7919 * seed)
        x0 = _halves(rng, -4, 4, case.n)
        # (a step of 1/2 on a row of c entries of +-1 multiplies the residual by about c / 2: beyond 65536 columns the noise is +-1/2 only, and the
        # cases have 40 rows, so that |dg|^2 -- which grows with the square of that -- keeps its headroom)
        noise = _halves(rng, -1, 1, case.m) if case.n > 65536 else _halves(rng, -2, 2, case.m)
        noise = noise * (rng.randint(0, 3, size=case.m) == 0)
        if np.count_nonzero(noise) < case.m / 4:
            continue
        g0 = -(A.T @ noise)                                   # = A^T (A x0 - b): does not depend on x0
        sparse = 1
        if case.loss == "logistic":
            # exp(z) must stay finite in float64 (the device evaluates log(1 + exp(z)) as the reference does): one entry in 32 of x0, and of a
            # dyadic g0 that is no gradient of anything -- to the launch it is an input like any other -- keep |z| of order 10
            sparse = 32
            x0 = x0 * (rng.randint(0, sparse, size=case.n) == 0)
            g0 = _halves(rng, -4, 4, case.n) * (rng.randint(0, sparse, size=case.n) == 0)
        prox = lambda v: RP.prox_of(case.kind, v, TAU * RP.PROX[case.kind][1], RP.PROX[case.kind][2], RP.PROX[case.kind][3])
        ok = True
        for lo, hi in required_pieces(case, sh):
            if prox(x0[lo:hi] - TAU * g0[lo:hi]).any():
                continue
            for v in (2.0, -2.0, 1.5, -1.5, 1.0, -1.0, 0.5, -0.5, 0.0):
                if prox(np.array([v - TAU * g0[lo]]))[0] != 0:
                    x0[lo] = v
                    break
            else:
                ok = False
        if not ok:
            continue
        b = A @ x0 + noise
        xp = prox(x0 - TAU * g0)
        xacc0, zacc0 = x0.copy(), A @ x0
        if accel:
            dx = xp - x0
            if case.mode == "restart_hi":                     # <x0 - xp, xp - x_accel0> = -|dx|^2 + <dx, d> > 0
                d = np.sign(dx) * np.ceil(np.abs(dx) * 4) / 2
            else:
                d = _halves(rng, -2, 2, case.n) * (rng.randint(0, 4 * sparse, size=case.n) == 0)
                if case.mode == "restart_lo" and float(np.sum((x0 - xp) * (xp - x0 - d))) > 0:
                    d = -d
            xacc0 = x0 + d
            zacc0 = A @ xacc0
        labels = np.where(np.arange(case.m) % 2 == 0, 1.0, -1.0) * np.where(rng.randint(0, 2, size=case.m) == 0, 1.0, -1.0)
        st = State(A, b, x0, g0, xacc0, zacc0, labels)
        if case.loss == "lsq" and not _sensitive(case, sh, st):
            continue
        for v in st[1:]:
            v.setflags(write=False)
        return st
    raise AssertionError(f"no sensitive operands for {case}")


def coef_rule(case):
    """the coefficient a launch applies, as a function of its own restart dot (fh_fused_body.inc: `coef = (p.restart && rdot > 1E-30) ? 0.0 : p.coef`)"""
    restart = case.mode in ("restart_hi", "restart_lo")
    return lambda rdot: 0.0 if (restart and rdot > 1E-30) else COEF


def _attempt(case, st, dtype=np.float64, magnitudes=None, **over):
    accel = case.mode != "plain"
    f = lambda v: np.asarray(v).astype(dtype)
    A, b, x0, g0, xacc0, zacc0 = (over.get(k, getattr(st, k)) for k in ("A", "b", "x0", "g0", "xacc0", "zacc0"))
    b = st.labels if (case.loss == "logistic" and "b" not in over) else b
    sums, v = RP.attempt(f(A), f(b), f(x0), f(g0), f(xacc0), f(zacc0), TAU, coef_rule(case), accel, case.kind, case.loss, dtype, magnitudes)
    if not accel:                                             # the launch leaves the restart dot zero and reports f itself as f at the extrapolated point
        sums[7], sums[10] = dtype(0), sums[0]
        v["coef"] = 0.0
    return sums, v


def gradient_factors(case, st):
    sums, v = _attempt(case, st)
    zx = v["z"] + v["coef"] * (v["z"] - st.zacc0) if case.mode != "plain" else v["z"]
    return zx - st.b


def _sensitive(case, sh, st):
    rv = gradient_factors(case, st)
    nz = rv != 0
    return bool(np.count_nonzero(nz) >= 0.9 * case.m and nz[required_rows(case, sh)].all() and st.A[nz].any(axis=0).all())


Result = collections.namedtuple("Result", "sums vectors")


@functools.lru_cache(maxsize=None)
def model(case):
    """The float64 model of a step case's launch: run_paths.attempt at the entering state.  sums in FH_S_* order; vectors xhat, xprox, z, g1, x1."""
    sums, v = _attempt(case, operands(case))
    return Result([float(s) for s in sums], {k: v[k] for k in ("xhat", "xprox", "z", "g1", "x1")} | {"coef": v["coef"]})


def prove(case):
    """The launch redone over the integers (run_paths.prove_attempt); returns (bits, where) or raises NotExact"""
    st = operands(case)
    mdl = model(case)
    bits = RP.Bits()
    accel = case.mode != "plain"
    isums, iv = RP.prove_attempt(st.A.astype(np.int64), st.b, st.x0, st.g0, st.xacc0, st.zacc0, TAU, mdl.vectors["coef"], accel, case.kind, bits)
    if not accel:
        isums[7], isums[10] = 0.0, isums[0]
    RP._need(isums == mdl.sums, f"float64 sums differ from the integers': {[n for n, a, c in zip(RP.SUMS, mdl.sums, isums) if a != c]}")
    for name in iv:
        RP._need(np.array_equal(iv[name], mdl.vectors[name]), f"float64 {name} differs from the integers'")
    # the state the launch enters with is formed on the device too: z0 = A x0 (fh_init) and g0 = A^T (z0 - b)
    Z0 = RP._matvec(st.A.astype(np.int64), RP._ints(st.x0, 1), bits, "z0 = A x0")
    RP._matvec(st.A.astype(np.int64).T, Z0 - RP._ints(st.b, 1), bits, "g0 = A^T (z0 - b)")
    return bits.worst, bits.where


# ---- the set-up's model ------------------------------------------------------------------------------------------------------------------------
Setup = collections.namedtuple("Setup", "A b x0 t0 t1")


@functools.lru_cache(maxsize=2)
def setup_operands(case):
    """x0 and the probes T0 / T1 multiples of 1/2 in [-2, 2]; b = A x0 + noise of non-zero multiples of 1/2 (the noise IS the gradient factor of
    the x0 column: it must not vanish)."""
    assert case.what == "setup"
    A = matrix(case.m, case.n, case.dens)
    rng = np.random.RandomState(9300 + case.m + 3 * case.n)
    x0, t0, t1 = (_halves(rng, -4, 4, case.n) for _ in range(3))
    noise = _halves(rng, 1, 2, case.m) * np.where(rng.randint(0, 2, size=case.m) == 0, 1.0, -1.0)
    e = 4 if case.storage == "f32" else 2
    for j in (0, case.n - 1, (case.n - 1) // e * e):          # the first and the last column, the last piece: both columns carry something
        x0[j] = x0[j] or 1.5
        if t0[j] == t1[j]:
            t0[j] = t1[j] + 0.5
    out = Setup(A, A @ x0 + noise, x0, t0, t1)
    for v in out[1:]:
        v.setflags(write=False)
    return out


def setup_model(case, ops=None):
    """what fh_setup's one-read launch leaves: z = A x0, f's sum |z - b|^2, g0 = A^T (z - b), T2 = A^T A (T0 - T1) and the two norms of L"""
    o = ops or setup_operands(case)
    d = o.t0 - o.t1
    z = o.A @ o.x0
    r = z - o.b
    zd = o.A @ d
    t2 = o.A.T @ zd
    return dict(FSQ=float(np.sum(r * r)), DX2=float(np.sum(d * d)), DG2=float(np.sum(t2 * t2)), GSUM=float(np.sum(np.abs(o.x0))), z=z, g0=o.A.T @ r, t2=t2,
                factors=(zd, r))


def prove_setup(case):
    """the set-up over the integers: every sum below 2^53 of its terms' lsb, the float64 model equal to the integers' result; (bits, where)"""
    o = setup_operands(case)
    mdl = setup_model(case)
    bits = RP.Bits()
    Ai = o.A.astype(np.int64)
    X0, D, B = RP._ints(o.x0, 1), RP._ints(o.t0, 1) - RP._ints(o.t1, 1), RP._ints(o.b, 1)
    Z, ZD = RP._matvec(Ai, X0, bits, "z = A x0"), RP._matvec(Ai, D, bits, "A d")
    R = RP._elements(Z - B, bits, "z - b")
    G0, T2 = RP._matvec(Ai.T, R, bits, "g0 = A^T r"), RP._matvec(Ai.T, ZD, bits, "A^T A d")
    got = dict(FSQ=RP._dot(R, R, bits, "|z - b|^2") / 4.0, DX2=RP._dot(D, D, bits, "|d|^2") / 4.0, DG2=RP._dot(T2, T2, bits, "|A^T A d|^2") / 4.0,
               GSUM=RP._sum(np.abs(X0), bits, "sum |x0|") / 2.0)
    for k, v in got.items():
        RP._need(v == mdl[k], f"float64 {k} differs from the integers'")
    for name, N in (("z", Z), ("g0", G0), ("t2", T2)):
        RP._need(np.array_equal(N / 2.0, mdl[name]), f"float64 {name} differs from the integers'")
    return bits.worst, bits.where


# ---- mutants of the model: defects a kernel could have, each with the path whose cases must show it ---------------------------------------------
MUTANTS = {"last pair unmasked": "odd n", "padding row in f": "padding rows in a live team", "last row skipped": "r_end % NB != 0",
           "member slice dropped from z": "clamped lanes", "team partial dropped from g1": "uneven last team", "x0 for x_accel0": None}


def compared(result):
    return [np.array(result.sums)] + [np.asarray(result.vectors[k]) for k in ("xhat", "xprox", "z", "g1", "x1")]


def differs(a, b):
    return any(x.shape != y.shape or not np.array_equal(x, y) for x, y in zip(a, b))


def mutant(case, which):
    """compared outputs of the model with defect `which`, or None where the defect does not apply to the case"""
    st, sh, mp = operands(case), expected_shape(case), round_up(case.m, 16)
    true = model(case)
    if which == "last pair unmasked":                        # the padding column behind an odd row's last entry goes through the prox and into the sums
        if case.n % 2 == 0:
            return None
        pad = lambda v: np.concatenate([v, [0.0]])
        sums, v = _attempt(case, st, A=np.hstack([st.A, np.zeros((case.m, 1))]), x0=pad(st.x0), g0=pad(st.g0), xacc0=pad(st.xacc0))
        return compared(Result([float(s) for s in sums], v))
    if which == "last row skipped":                          # the last live row of the last team that has one: no z, no term of f, no update
        rows = [r for t in range(sh.nteams) for r in [q for q in team_rows(sh, mp, t) if q < case.m][-1:]]
        A, b, za = st.A.copy(), st.b.copy(), st.zacc0.copy()
        A[rows[-1]], b[rows[-1]], za[rows[-1]] = 0, 0, 0
        sums, v = _attempt(case, st, A=A, b=b, zacc0=za)
        return compared(Result([float(s) for s in sums], v))
    if which == "member slice dropped from z":               # the last member that owns columns
        mem = max(k for k in range(sh.TEAM) if member_columns(sh, case.n, k)[0] < member_columns(sh, case.n, k)[1])
        if sh.TEAM == 1:
            return None
        lo, hi = member_columns(sh, case.n, mem)
        out = dict(true.vectors)
        out["z"] = true.vectors["z"] - st.A[:, lo:hi] @ true.vectors["xprox"][lo:hi]
        return compared(Result(true.sums, out))
    if which == "team partial dropped from g1":              # the last team that has live rows
        rows = [r for r in [team_rows(sh, mp, t) for t in range(sh.nteams) if any(r < case.m for r in team_rows(sh, mp, t))][-1] if r < case.m]
        if sh.nteams == 1:
            return None
        rv = gradient_factors(case, st)
        out = dict(true.vectors)
        out["g1"] = true.vectors["g1"] - st.A[rows].T @ rv[rows]
        return compared(Result(true.sums, out))
    if which == "x0 for x_accel0":
        if case.mode == "plain":
            return None
        sums, v = _attempt(case, st, xacc0=st.x0, zacc0=st.A @ st.x0)
        return compared(Result([float(s) for s in sums], v))
    raise KeyError(which)


def padding_rows_in_f(case):
    """the defect 'a padding row counted in f'.  For least squares a padding row's term is (0 - 0)^2: the defect cannot show, whatever the data.  The
    logistic loss adds log 2 per padding row: returns (the model's f, the mutant's f) of a logistic case."""
    assert case.loss == "logistic"
    sums, _ = _attempt(case, operands(case), dtype=np.longdouble)
    return float(sums[0]), float(sums[0] + (round_up(case.m, 16) - case.m) * np.log(np.longdouble(2)))
