"""The list of stations (tests/carry_cases.py) is complete: checked without a device.  The proof that the exact stations' operands ARE exact stays
in the home modules' CPU tests (test_fused_paths_cpu, test_run_paths_cpu, test_mc_paths_cpu, test_sparse_lanes_cpu, test_tv_paths_cpu,
test_tv3d_cpu, test_quad_cpu, test_factor_cpu, test_conv_cpu); here: the stations take their cases FROM those modules."""
import ast
import os
import re

import numpy as np

from fasta_python_amd import hip
from tests import carry_cases as K
from tests import refusal_cases as RC

HERE = os.path.dirname(os.path.abspath(__file__))
ALL = K.STATIONS + K.F32_STATIONS


def test_every_setter_and_every_operator_form_has_a_station():
    setters = {s.setter for s in ALL}
    assert setters == set(RC.SETTERS), (set(RC.SETTERS) - setters, setters - set(RC.SETTERS))
    assert {s.op for s in ALL} == set(RC.OP_OF.values())
    for s in ALL:
        assert s.op == RC.OP_OF.get(s.setter, "OP_DENSE")                          # (the two other ways into the dense form)
    # float32 storage: what the fixture records as accepted there, read from it
    assert sorted({s.setter for s in K.F32_STATIONS}) == K.f32_setters() and all(s.storage == "f32" for s in K.F32_STATIONS)
    assert "dense_f32_host" in K.f32_setters() and "csr" not in K.f32_setters()


def test_the_stations_the_issue_names_are_there():
    names = {s.name for s in K.STATIONS}
    assert len(K.STATIONS) == len(names) == 24
    for want in ("dense one-pass", "dense pair", "dense rhs4 group", "dense softmax", "dense fh_run", "dense fh_setup", "csr", "csr rhs", "stencil plain",
                 "stencil lazy", "stencil 3-D", "quadratic L1", "quadratic L2 rowball", "factorisation split", "dct two-level", "dct 2-D", "convolution",
                 "identity nuclear", "identity weights nucball", "l1 ball dense", "l1 ball dct", "l1 ball conv", "duality gap"):
        assert want in names, want
    assert [s.name for s in K.STATIONS if s.leaves_lazy] == ["stencil lazy"]
    assert {s.name for s in K.STATIONS if not s.bitwise} == {"l1 ball dense", "l1 ball dct", "l1 ball conv"}     # the level search alone: home tolerance


def test_every_tuning_key_is_stated():
    keys = {v for k, v in vars(hip).items() if k.startswith("TUNE_") and k != "TUNE_TEST_HOOKS"}
    assert set(K.TUNING_AUTO) == keys and hip.TUNE_TEST_HOOKS not in K.TUNING_AUTO
    for s in ALL:
        assert set(s.tuning) <= keys - K.NEVER_WRITTEN and hip.TUNE_TEST_HOOKS not in s.tuning, s.name
    # the automatic values are the ones the context starts with (csrc/fh_host_ctx.h), but for the two keys a write cannot bring back to automatic
    text = open(os.path.join(HERE, "..", "fasta_python_amd", "csrc", "fh_host_ctx.h")).read()
    for field, key in (("fwd_rows", hip.TUNE_FWD_ROWS), ("adj_slab", hip.TUNE_ADJ_SLAB_ROWS), ("adj_cpt", hip.TUNE_ADJ_CPT), ("adj_cyclic", hip.TUNE_ADJ_CYCLIC),
                       ("tv_u", hip.TUNE_TV_U), ("tv_rows", hip.TUNE_TV_ROWS), ("tv_nt", hip.TUNE_TV_NT), ("tv_xcd", hip.TUNE_TV_XCD), ("tv_pipe", hip.TUNE_TV_PIPE),
                       ("tv3_planes", hip.TUNE_TV3_PLANES), ("nuc_block_rows", hip.TUNE_NUC_BLOCK_ROWS), ("dct_row_cap", hip.TUNE_DCT_ROW_CAP),
                       ("seq_poll", hip.TUNE_SEQ_POLL), ("run_max_n", hip.TUNE_RUN_MAX_N), ("fused_cus", hip.TUNE_FUSED_CUS), ("run_chain_on", hip.TUNE_RUN_CHAIN)):
        m = re.search(rf"\bint {field} = (-?\d+);", text)
        assert m and int(m.group(1)) == K.TUNING_AUTO[key], field
    assert re.search(r"int nt_loads = -1;", text) and K.TUNING_AUTO[hip.TUNE_NT_LOADS] == 0
    assert re.search(r"int fused_variant = 2 \| 32;", text) and re.search(r"int fused_min_rows = 16;", text)
    assert K.TUNING_AUTO[hip.TUNE_FUSED_VARIANT] == (16 << 16) | 2 | 32


def test_the_plan_covers_every_ordered_pair():
    for stations in (K.STATIONS, K.F32_STATIONS):
        want = {(a.name, b.name) for a in stations for b in stations if a is not b}
        assert K.pairs_of(stations) == want and len(want) == len(stations) * (len(stations) - 1)
        for p in stations:
            seq = K.plan(stations, p)
            assert seq[0] is p and seq[-1] is p and len(seq) == 2 * len(stations) - 1 and all(a is not b for a, b in zip(seq, seq[1:]))
    chain = K.long_chain(K.STATIONS)
    assert len(chain) == 3 * len(K.STATIONS) and {s.name for s in chain} == {s.name for s in K.STATIONS} and chain == K.long_chain(K.STATIONS)
    assert all(a is not b for a, b in zip(chain, chain[1:]))


def test_no_gpu_test_of_the_new_module_carries_a_skip():
    tree = ast.parse(open(os.path.join(HERE, "test_gpu_carry.py")).read())
    names = {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute)} | {n.id for n in ast.walk(tree) if isinstance(n, ast.Name)}
    assert not names & {"skip", "skipif", "xfail", "importorskip"}
    tree = ast.parse(open(os.path.join(HERE, "carry_cases.py")).read())
    names = {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute)} | {n.id for n in ast.walk(tree) if isinstance(n, ast.Name)}
    assert not names & {"skip", "skipif", "xfail", "importorskip"}


def test_the_leaving_states_name_stations_that_exist():
    succ = [K.BY_NAME[n] for n in K.LEAVING_SUCCESSORS]
    assert any(s.dense for s in succ) and any(s.setter == "stencil" for s in succ) and any(s.setter == "identity" for s in succ)
    assert set(K.LEAVING_PREDECESSORS) <= {s.name for s in K.STATIONS} and "stencil lazy" in K.LEAVING_PREDECESSORS
    assert set(K.LEAVINGS) == {"after commit", "mid-attempt", "after an accelerated attempt"}


def test_the_stations_take_their_cases_from_the_home_modules():
    """a case object, not a copy of its numbers: a later change of a home case moves the station with it"""
    from tests import conv_cases as CV, dct2_cases as D2, dct_cases as D1, factor_cases as FC, fused_paths as FP, gap_cases as GC, mc_paths as MC
    from tests import completion_cases as CC, quad_cases as QC, run_paths as RP, sparse_lanes as SL, tv3d_cases as T3, tv_paths as TV
    assert all(s.home in K.HOME_MODULES for s in ALL)
    assert K.ONEPASS in FP.exact_step_cases() and K.ONEPASS_F32 in FP.exact_step_cases() and K.SETUP in FP.setup_cases() and K.RUN in RP.cases()
    assert (K.PAIR_TUNING, K.PAIR_KIND) in MC.vector_cases() and (K.RHS4, K.RHS4_NT) in MC.group_cases() and K.RHS4.L == 4
    assert K.CSR_RHS in SL.step_cases() and (K.CSR_G, 0, None, K.CSR_KIND) in SL.step_cases()
    assert K.QUAD1 in QC.cases() and K.QUAD2 in QC.rownorm_cases() and K.QUAD2[1] == 2 and K.FACTOR in FC.cases()
    assert (K.DCT_N, K.DCT_CAP) in D1.SIZES and K.DCT2_SHAPE in D2.SIZES and K.CONV in CV.SHAPES and K.ID_SHAPE in CC.STEP_SHAPES
    assert T3.RAGGED in T3.ALL_SHAPES and K.GAP_SHAPE in GC.SHAPES and TV.BACK_TO_BACK in TV.GEOMETRY and TV.BITS_GEOMETRY in TV.GEOMETRY
    assert TV.STATE[K.LAZY_STATE].accel and TV.STATE[K.LAZY_STATE].lagged


def test_the_chosen_cases_put_several_workgroups_on_their_launches():
    """what the GPU tier asserts through the context's shape queries, from the pure forms of the same rules"""
    from tests import conv_cases as CV, fused_paths as FP, mc_paths as MC, quad_cases as QC, run_paths as RP, factor_cases as FC, tv3d_cases as T3
    for case in (K.ONEPASS, K.ONEPASS_F32):
        sh = FP.shape_query(case, 256)
        assert sh == FP.expected_shape(case) and sh.TEAM >= 2 and sh.nteams >= 2 and 0 < case.cus <= 64
    sh = FP.shape_query(K.SETUP, 256)
    assert sh == FP.expected_shape(K.SETUP) and sh.grid >= 2 and sh.nteams >= 2
    sh = RP.shape_query(K.RUN)
    assert sh == RP.expected_shape(K.RUN) and sh.G - sh.empty_wgs >= 2
    sh = MC.expected_shape(K.RHS4, K.RHS4_NT)
    assert sh.nslab >= 2 and sh.last_slab_rows < sh.slab_rows and sh.ncc >= 2 and sh.fwd_grid >= 2 and sh.stages >= 2
    slab = K.PAIR_TUNING[hip.TUNE_ADJ_SLAB_ROWS]
    assert MC.VECTOR_M > slab and MC.VECTOR_M % slab and MC.VECTOR_N > 2 * 256 * K.PAIR_TUNING[hip.TUNE_ADJ_CPT]
    assert QC.expected_shape(K.QUAD1).fwd_grid >= 2 and QC.expected_shape(K.QUAD2_CASE).fwd_grid >= 2 and FC.expected_shape(K.FACTOR).grid >= 2
    sh = hip.tv3d_shape(*T3.RAGGED, planes=T3.PLANES)
    assert sh.chunks >= 2 and sh.tiles_h >= 2 and sh.tiles_w >= 2
    assert hip.dct_shape(K.DCT_N, K.DCT_CAP).levels == 2 and min(hip.dct_shape(K.DCT_N, K.DCT_CAP).grid1, hip.dct_shape(K.DCT_N, K.DCT_CAP).grid2) >= 2
    assert min(hip.dct2_shape(*K.DCT2_SHAPE).grid_h, hip.dct2_shape(*K.DCT2_SHAPE).grid_w) >= 2
    assert hip.conv_shape(*CV.shape2d(K.CONV[0]), *CV.shape2d(K.CONV[1])).grid >= 2 and hip.nuclear_shape(*K.ID_SHAPE).wgs_per_step >= 2
    assert 16384 < K.L1_DENSE_N <= 262144


def test_traces_compare_bit_for_bit():
    a, b = K.Trace(), K.Trace()
    for t in (a, b):
        t.put("s", [1.0, np.nan, -0.0])
        t.home("h", {"x": np.arange(3.0), "y": (np.ones(2), {"z": np.zeros(1)})})
    assert K.first_difference(a, b) is None and list(a) == ["s", "h.x", "h.y.0", "h.y.1.z"]
    b["h.x"][1] = np.nextafter(1.0, 2.0)
    assert "h.x: 1 entries differ, first at 1" in K.first_difference(a, b)
    b["h.x"][1] = 1.0
    b["s"][2] = 0.0                                                                 # (-0.0 == 0.0: values, as every home suite compares)
    assert K.first_difference(a, b) is None
    del b["s"]
    assert "names differ" in K.first_difference(a, b)
