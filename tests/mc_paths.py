"""Inputs and geometry for the tests of EVERY loop of the multi-column dense kernels (csrc/fh_multi.h: k_mc_fwd / k_mc_adj<LB, .., NT>) and of
the tuning grid of the vector kernels (csrc/fh_dense.h: k_fwd_dense<R, NT, PROX> / k_adj_dense<CPT, NT>).  A plain helper module, the
sibling of tests/sparse_lanes.py, whose exact model (exact_step, the operands, tau = 1/2, coef = 1/4, the GroupShrink tolerances) it reuses:
the CPU tier (tests/test_mc_paths_cpu.py) checks every condition claimed here, the GPU tier (tests/test_gpu_mc_paths.py) runs the kernels.

The loops in question need m > 4096 .. 32768 under the automatic launch rules; FH_TUNE_ADJ_SLAB_ROWS and FH_TUNE_FWD_GRID_CAP reach every
one of them at about 2000 x 1000.  A case states the tuning it sets AND the geometry it expects of it (expected_shape); both tiers compare
that with the library's own rule (fh_multi_shape_for / fh_multi_shape), so a change of the host's rule fails a test instead of emptying it.

Exactness: matrices hold -1, 0, 1 with three quarters of the entries zero, the operands are those of tests/sparse_lanes.py (multiples of
1/2), so every product, sum and extrapolation of a step is a multiple of 1/16 (its squares of 1/256) below 2^53 of them whatever the order
of summation: a kernel's result must EQUAL the model's."""
import collections
import functools

import numpy as np

from fasta_python_amd import hip
from tests import sparse_lanes as SL

FH_WG = 256                                   # csrc/fh_device.h
MC_LDS_DOUBLES = 2048                         # csrc/fh_multi.h: doubles of the residual a stage of k_mc_adj holds
MC_ADJ_CPT = 2                                # csrc/fh_multi.h: 16-byte column pairs per lane of k_mc_adj
ADJ_MAX_SLAB = 2048                           # csrc/fh_dense.h
MC_FOR_EACH = {2: (2, 16), 4: (4, 16), 8: (8, 8), 16: (8, 8)}          # csrc/fh_multi.h: LB -> (CH, R)
ALL_LB = SL.ALL_LB
TAU, COEF = SL.TAU, SL.COEF
N_WIDE, N_NARROW = 1030, 24                   # ld2 = 520: two column chunks, 8 live lanes in the second; ld2 = 16: one chunk, one trip

Case = collections.namedtuple("Case", "name LB m n L slab cap kind")


def stage_rows(LB):
    """SB: rows of the residual k_mc_adj stages at a time."""
    return MC_LDS_DOUBLES // LB


def round_up(v, k):
    return (v + k - 1) // k * k


def uneven_cap(nrg):
    """FH_TUNE_FWD_GRID_CAP: 3, or the next value that does not divide the row groups (LB = 4: 66 row groups -> 4; LB = 16: 36 -> 5), so that
    the workgroups of k_mc_fwd make unequal numbers of passes."""
    cap = 3
    while nrg % cap == 0:
        cap += 1
    return cap


def _geometries():
    """(name, LB, m, n, slab tuning, grid cap, column counts)."""
    out = []
    for LB in ALL_LB:
        R = MC_FOR_EACH[LB][1]
        slab = stage_rows(LB) + 8                     # two stages, the second of 8 rows
        mp = 2 * slab + 16                            # two full slabs and a last slab of 16 rows
        m = mp - 10                                   # ... of which 10 rows are padding (m is no multiple of 16)
        cap = uneven_cap(mp // R)
        both = [LB, LB - 1]
        smallest = LB // 2 + 1                        # the fewest columns this LB serves: 3, 5, 9 (LB = 2: 1 = LB - 1 already)
        out.append(("staged", LB, m, N_WIDE, slab, cap, both + [smallest] * (smallest not in both)))
        out.append(("narrow", LB, m, N_NARROW, slab, cap, both))
        out.append(("default", LB, 200, 1000, 0, 0, both))
    out.append(("many stages", 16, 2100, N_WIDE, ADJ_MAX_SLAB, uneven_cap(round_up(2100, 16) // 8), [16, 15]))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """Every (geometry, column count); the elementwise prox kind rotates so that each kind meets each LB."""
    out, seen = [], collections.Counter()
    for name, LB, m, n, slab, cap, Ls in _geometries():
        for L in Ls:
            kind = SL.PROX_KINDS[(seen[LB] + LB // 2) % 4]
            seen[LB] += 1
            out.append(Case(name, LB, m, n, L, slab, cap, kind))
    return tuple(out)


def group_cases():
    """One column count per geometry for the GroupShrink step, alternating between LB - 1 and LB; (case, nt) with the load policy alternating."""
    out = []
    for i, (name, LB, m, n, slab, cap, Ls) in enumerate(_geometries()):
        L = max(1, LB - 1) if i % 2 == 0 else LB
        out.append((Case(name, LB, m, n, L, slab, cap, "group"), i % 2))
    return out


def case_id(c):
    return f"{c.name.replace(' ', '_')}-LB{c.LB}-L{c.L}-{c.m}x{c.n}-{c.kind}"


def tuning_of(case, nt):
    t = {hip.TUNE_NT_LOADS: nt}
    if case.slab:
        t[hip.TUNE_ADJ_SLAB_ROWS] = case.slab
    if case.cap:
        t[hip.TUNE_FWD_GRID_CAP] = case.cap
    return t


# ---- what a case's name claims ----------------------------------------------------------------------------------------------------------------
def expected_shape(case, nt):
    """The hip.MultiShape a case must be launched with, from the case's own numbers (forced slab and cap) -- or, for `default`, from the
    automatic rules restated here once: a K-fwd grid of min(nrg, 512), slabs of max(32, round_up(ceil(mp / 128), 8)) rows at one column chunk."""
    CH, R = MC_FOR_EACH[case.LB]
    mp, ld2 = round_up(case.m, 16), round_up(case.n, 16) // 2
    nrg = mp // R
    ncc = -(-ld2 // (FH_WG * MC_ADJ_CPT))
    if case.slab:
        slab = case.slab
    else:
        assert ncc == 1
        slab = min(max(round_up(-(-mp // 128), 8), 32), ADJ_MAX_SLAB)
    nslab = -(-mp // slab)
    SB = stage_rows(case.LB)
    return hip.MultiShape(LB=case.LB, CH=CH, R=R, NT=nt, fwd_grid=min(nrg, case.cap or 512), nrg=nrg, ntrip=-(-ld2 // (FH_WG * CH // case.LB)),
                          npro=-(-2 * ld2 // FH_WG), slab_rows=slab, nslab=nslab, last_slab_rows=mp - (nslab - 1) * slab, SB=SB,
                          stages=-(-slab // SB), ncc=ncc)


def paths_of(sh, m, n):
    """The loops a launch geometry `sh` (hip.MultiShape) of an (m, n) matrix runs, as a dict of booleans -- the rows of the coverage table
    (scripts/mc_path_coverage.py) and what the CPU tier asserts of every case's name."""
    ld2 = round_up(n, 16) // 2
    last_stage = sh.slab_rows - (sh.stages - 1) * sh.SB
    lanes = FH_WG * sh.CH // sh.LB                    # lanes of a column group of k_mc_fwd
    return {
        "several stages": sh.stages > 1,
        "short last stage": sh.stages > 1 and last_stage < sh.SB,
        "ragged last slab": sh.last_slab_rows < sh.slab_rows,
        "ncc > 1": sh.ncc > 1,
        "clamped chunk": sh.ncc * FH_WG * MC_ADJ_CPT > ld2,
        "K-fwd second pass": sh.nrg > sh.fwd_grid,
        "uneven passes": sh.nrg > sh.fwd_grid and sh.nrg % sh.fwd_grid != 0,
        "masked last trip": sh.ntrip * lanes > ld2,
    }


PATHS = ("several stages", "short last stage", "ragged last slab", "ncc > 1", "clamped chunk", "K-fwd second pass", "uneven passes", "accelerated adjoint")


# ---- matrices and operands --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def matrix(m, n):
    """(m, n) of -1, 0, 1, three quarters of the entries zero (with none zero the widest sum of a step has a headroom of only 5 x)."""
    rng = np.random.RandomState(4000 + 31 * m + n)
    A = rng.choice([-1, 1], size=(m, n)) * (rng.randint(0, 4, size=(m, n)) == 0)
    A = A.astype(np.float64)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def step_inputs(m, n, L):
    """(A, X0, B) of the exact step: the operands of tests/sparse_lanes.py:step_operands on matrix(m, n).  L = None: the vector form."""
    A = matrix(m, n)
    X0, B = SL.step_operands(A, L)
    for V in (X0, B):
        V.setflags(write=False)
    return A, X0, B


@functools.lru_cache(maxsize=None)
def step_model(m, n, L, kind):
    """The float64 model of one exact step, computed once and shared (read-only) by the tests that compare against it."""
    A, X0, B = step_inputs(m, n, L)
    want = SL.exact_step(A, X0, B, SL.prox_tag(kind))
    for name in SL.MATRICES:
        want[name].setflags(write=False)
    return want


# ---- the vector kernels through the same harness ---------------------------------------------------------------------------------------------
VECTOR_M, VECTOR_N = 2070, N_WIDE
VECTOR_SLAB, VECTOR_CAP = 1032, 3            # mp = 2080: two slabs of 1032 rows and a last one of 16; 520 / R row groups on 3 workgroups


N_RAGGED_F32 = 1029                          # float32 storage: n % 4 = 1 and n % 32 = 5 -- a last four-column piece with one live column


def vector_cases(storage="f64"):
    """(tuning, prox kind) of the exact step in the vector form: FH_TUNE_FWD_ROWS x FH_TUNE_NT_LOADS, then FH_TUNE_ADJ_CPT x NT x
    FH_TUNE_ADJ_CYCLIC, all under the forced slab (a ragged last slab) and grid cap; the four exact prox kinds rotate.

    storage="f32": (tuning, prox kind, n) of k_fwd_dense<4|8, 1, KIND, 1> / k_adj_dense<1|2|4, 1, 1>.  Float32 storage loads non-temporally
    whatever FH_TUNE_NT_LOADS says, so the axis is left out: every exact prox kind at every FH_TUNE_FWD_ROWS (16 launches the 8-row form: only
    then is every row of Z written), FH_TUNE_ADJ_CPT x FH_TUNE_ADJ_CYCLIC, a width with n % 4 != 0 and n % 32 != 0 under the automatic
    CPT (keyed on ld / 4) and one case with FH_TUNE_LD_PAD = 32."""
    base = {hip.TUNE_ADJ_SLAB_ROWS: VECTOR_SLAB, hip.TUNE_FWD_GRID_CAP: VECTOR_CAP}
    out = []
    if storage == "f32":
        for R in (4, 8, 16):
            for kind in SL.PROX_KINDS:
                out.append(({**base, hip.TUNE_FWD_ROWS: R}, kind, N_WIDE))
        for cpt in (1, 2, 4):
            for cyclic in (0, 1):
                out.append(({**base, hip.TUNE_ADJ_CPT: cpt, hip.TUNE_ADJ_CYCLIC: cyclic}, SL.PROX_KINDS[len(out) % 4], N_WIDE))
        out.append(({**base, hip.TUNE_FWD_ROWS: 4}, "box", N_RAGGED_F32))
        out.append(({**base, hip.TUNE_FWD_ROWS: 8, hip.TUNE_ADJ_CPT: 2, hip.TUNE_ADJ_CYCLIC: 1}, "shrink", N_RAGGED_F32))
        out.append(({**base, hip.TUNE_LD_PAD: 32, hip.TUNE_FWD_ROWS: 4, hip.TUNE_ADJ_CPT: 1}, "nonneg", N_WIDE))
        return out
    assert storage == "f64", storage
    for R in (4, 8, 16):
        for nt in (0, 1):
            out.append(({**base, hip.TUNE_FWD_ROWS: R, hip.TUNE_NT_LOADS: nt}, SL.PROX_KINDS[len(out) % 4]))
    for cpt in (1, 2, 4):
        for nt in (0, 1):
            for cyclic in (0, 1):
                out.append(({**base, hip.TUNE_ADJ_CPT: cpt, hip.TUNE_NT_LOADS: nt, hip.TUNE_ADJ_CYCLIC: cyclic}, SL.PROX_KINDS[len(out) % 4]))
    return out


def vector_level_cases(storage="f32"):
    """(tuning, level prox) of k_fwd_dense<4|8, ., PX_LINF | PX_L1BALL, F32>: each once per rows-per-pass form, on tests/level_cases.py's
    step problem at VECTOR_M x N_WIDE (the level falls exactly on 2, so the step stays exact)."""
    base = {hip.TUNE_ADJ_SLAB_ROWS: VECTOR_SLAB, hip.TUNE_FWD_GRID_CAP: VECTOR_CAP}
    return [({**base, hip.TUNE_FWD_ROWS: R}, prox) for R in (4, 8) for prox in ("linf", "l1ball")]


TUNE_NAMES = {hip.TUNE_FWD_ROWS: "R", hip.TUNE_NT_LOADS: "nt", hip.TUNE_ADJ_CPT: "cpt", hip.TUNE_ADJ_CYCLIC: "cyclic", hip.TUNE_LD_PAD: "pad"}


def vector_id(v):
    if isinstance(v, dict):
        return "-".join(f"{TUNE_NAMES[k]}{v[k]}" for k in sorted(v) if k in TUNE_NAMES)
    return str(v)
