"""CPU tier of the 3-D stencil operator (fh_set_stencil3d, csrc/fh_tv3d.h): the fixtures of scripts/make_tv3d_golden.py against the oracle and
the NumPy backend, the host face of GradDivMap, the launch geometry in its pure form, the loop-spill guard and the conditions the exact
GPU tests rest on.  No device is touched."""
import os
import shutil
import subprocess
import sys
import warnings

import numpy as np
import pytest

import fasta_python_amd as fa
from fasta_python_amd import hip
from oracle import fasta_np as fo
from oracle import problems as pr
from tests import helpers as H
from tests import tv3d_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def capture_script():
    """scripts/make_tv3d_golden.py as a module: its case table, constructor, closures and twin are the definition of the fixtures."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_tv3d_golden", os.path.join(ROOT, "scripts", "make_tv3d_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_fixture_set_is_the_capture_scripts_case_table():
    names = [case[0] for case in capture_script().case_table()]
    assert sorted(names) == T.CASES and len(names) == 6
    for name in names:
        meta, z, d = T.load(name)
        assert os.path.getsize(os.path.join(T.GOLDEN, name + ".npz")) < 64 * 1024
        assert d["M"].ndim == 3 and z["solution"].shape == d["M"].shape + (3,)
        assert ("twin_divergence" in meta) == bool(meta["options"].get("adaptive"))


def assert_same_run(c, z):
    assert c.iteration_count == int(z["iteration_count"]) and c.backtracks == int(z["backtracks"])
    for f in T.FIELDS:
        assert np.array_equal(getattr(c, f), z[f], equal_nan=True), f
    assert np.array_equal(c.solution, z["solution"])


@pytest.mark.parametrize("name", T.CASES)
def test_oracle_and_numpy_backend_reproduce_the_fixture_bit_for_bit(name):
    cap = capture_script()
    meta, z, d = T.load(name)
    np.random.seed(meta["problem_seed"])
    again = cap.construct(**{k: tuple(v) if isinstance(v, list) else v for k, v in meta["construct"].items()})
    assert np.array_equal(again["M"], d["M"]) and float(again["mu"]) == float(d["mu"])          # the stored inputs are the seeded ones
    assert_same_run(cap.oracle_run(d, meta["prox"], meta["options"], sseed=meta["solver_seed"]), z)
    # the package's generic host loop over GradDivMap's host face and the tagged loss / prox
    M, mu = d["M"], float(d["mu"])
    op = fa.GradDivMap(M.shape)
    loss, reg = fa.LeastSquares(M / mu), (fa.TVDualBall() if meta["prox"] == "ball" else fa.Box(-1.0, 1.0))
    np.random.seed(meta["solver_seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = fa.fasta(op, op.H, loss.f, loss.gradf, reg.g, reg.prox, np.zeros(M.shape + (3,)), backend="numpy", verbose=False, **meta["options"])
    assert_same_run(c, z)
    assert np.array_equal(M - mu * op(c.solution), z["primal"])
    assert op._ctx is None                                                                     # no device context was created


@pytest.mark.parametrize("name", [n for n in T.CASES if "adaptive" in n])
def test_the_twins_parting_iteration_is_the_stored_one(name):
    cap = capture_script()
    meta, z, d = T.load(name)
    assert cap.TWIN_AXES == T.TWIN_AXES
    k, bt = cap.twin_divergence(d, meta["prox"], meta["options"], meta["solver_seed"])
    assert (k, bt) == (meta["twin_divergence"], meta["backtracks_at_divergence"])
    assert k >= 40 or k == int(z["iteration_count"])                  # a prefix worth pinning a device run on
    # ... and up to there the run with L and tau0 passed in IS the fixture's run
    L, tau0 = cap.step_estimate(d, meta["prox"], meta["solver_seed"])
    head = cap.oracle_run(d, meta["prox"], dict(meta["options"], max_iters=max(k, 1), tolerance=0.0), L=L, tau0=tau0)
    assert np.array_equal(head.stepsizes[:k], z["stepsizes"][:k])


@pytest.mark.parametrize("shape", [(3, 4, 5), (2, 3, 1), (1, 1, 1), (6, 10, 12)])
def test_graddivmap_host_closures_are_the_oracles_grad_and_div(shape):
    rng = np.random.RandomState(5)
    Y, X = rng.randn(*shape, 3), rng.randn(*shape)
    op = fa.GradDivMap(shape)
    assert op.Vshape == tuple(shape) + (3,) and op.Wshape == tuple(shape) and op.image_shape == tuple(shape)
    assert np.array_equal(op(Y), pr.div(Y)) and np.array_equal(op.H(X), pr.grad(X))
    assert np.array_equal(T.div(Y), pr.div(Y)) and np.array_equal(T.grad(X), pr.grad(X))          # the exact model's dtype-preserving twins
    assert op._ctx is None


@pytest.mark.parametrize("shape", [(4,), (2, 3, 4, 5), ()])
def test_graddivmap_refuses_other_ranks_with_a_sentence(shape):
    with pytest.raises(ValueError, match="volume shape"):
        fa.GradDivMap(shape)


def test_the_binding_knows_the_new_entry_points():
    assert {"fh_set_stencil3d", "fh_tv3d_shape", "fh_tv3d_shape_for"} <= set(hip.SIGNATURES)
    assert hasattr(hip.HipContext, "set_stencil3d") and hasattr(hip.HipContext, "tv3d_shape") and hip.TUNE_TV3_PLANES == 21
    text = open(os.path.join(ROOT, "include", "fasta_hip.h")).read()
    assert "FH_TUNE_TV3_PLANES = 21" in text and f"#define FH_TV3D_SHAPE_LEN {hip.TV3D_SHAPE_LEN}" in text


@pytest.mark.parametrize("planes", [0, T.PLANES, 1])
@pytest.mark.parametrize("shape", T.ALL_SHAPES + [(128, 128, 128), (64, 2048, 2048), (768, 768, 768)], ids=str)
def test_every_voxel_has_exactly_one_owner(shape, planes):
    """fh_tv3d_shape_for, the rule both launchers call, walked over the GPU tier's shapes (and the measured ones): the tiles are those of
    csrc/fh_tv3d.h, the grid is chunks x tiles, no workgroup is empty and every voxel lies in exactly one."""
    sh = hip.tv3d_shape(*shape, planes=planes, ncu=256)
    D, Hh, W = shape
    assert (sh.tile_h, sh.tile_w) == (T.TILE_H, T.TILE_W)
    assert sh.tiles_h == -(-Hh // sh.tile_h) and sh.tiles_w == -(-W // sh.tile_w) and sh.chunks == -(-D // sh.planes)
    assert sh.grid == sh.chunks * sh.tiles_h * sh.tiles_w and 1 <= sh.planes <= D
    if planes:
        assert sh.planes == min(planes, D)
    if np.prod(shape) <= 1 << 21:
        assert np.all(T.owners(shape, sh) == 1)
    else:                                                  # the same count, axis by axis (the ownership is a product of three 1-D partitions)
        for n, step, parts in ((D, sh.planes, sh.chunks), (Hh, sh.tile_h, sh.tiles_h), (W, sh.tile_w, sh.tiles_w)):
            assert (parts - 1) * step < n <= parts * step


def test_the_ragged_shape_has_several_workgroups_and_a_ragged_last_tile_on_every_axis():
    sh = hip.tv3d_shape(*T.RAGGED, planes=T.PLANES)
    D, Hh, W = T.RAGGED
    assert sh.chunks >= 2 and sh.tiles_h >= 2 and sh.tiles_w >= 2
    assert D % sh.planes and Hh % sh.tile_h and W % sh.tile_w


def test_the_shape_rule_refuses_what_the_operator_refuses():
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        with pytest.raises(hip.HipError, match="D >= 1"):
            hip.tv3d_shape(*bad)
    with pytest.raises(hip.HipError, match="2\\^31"):
        hip.tv3d_shape(895, 895, 895)                      # 3 * 895^3 = 2 150 742 125 >= 2^31
    assert hip.tv3d_shape(894, 894, 894).grid > 0          # 3 * 894^3 = 2 143 544 952 <  2^31


def test_no_scratch_in_the_loops_of_the_3d_stencil_kernels():
    """scripts/loop_spills.py over every instantiation of k_tv3_fwd and k_tv3_adj (make -C fasta_python_amd/csrc tv3d-spills).  Needs hipcc,
    as the build does."""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs hipcc")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "fasta_python_amd", "csrc"), "tv3d-spills", f"PYTHON={sys.executable}"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("inside loops: none") == 6, r.stdout


@pytest.mark.parametrize("case", list(enumerate(T.ALL_SHAPES)), ids=lambda c: str(c[1]))
def test_the_exact_step_is_exact(case):
    """The condition of the GPU tier's `==` comparisons: on these operands the step in float64, in longdouble and in integer arithmetic (the
    operands scaled by 32) is the same numbers -- so no order of additions can change a sum."""
    i, shape = case
    kind = T.PROX_KINDS[i % len(T.PROX_KINDS)]
    x0, b = T.exact_operands(shape, 100 + i)
    assert np.array_equal(x0 * 2, np.round(x0 * 2)) and np.abs(x0).max() <= 2 and np.array_equal(b * 2, np.round(b * 2))
    runs = [(ops, T.exact_step(x0, b, kind, ops)) for ops in (T.FloatOps(np.float64), T.FloatOps(np.longdouble), T.IntOps())]
    (_, (blocks64, vec64)) = runs[0]
    for ops, (blocks, vec) in runs[1:]:
        for call, block in blocks.items():
            assert np.array_equal(T.block_as_float(block, ops), T.block_as_float(blocks64[call], runs[0][0])), (type(ops).__name__, call)
        for name, v in vec.items():
            assert np.array_equal(np.asarray(v, dtype=np.float64) / ops.unit, vec64[name]), (type(ops).__name__, name)
    # every vector entry is a multiple of 1/16, every sum far below 2^53 / 256
    for v in vec64.values():
        assert np.array_equal(v * 16, np.round(v * 16))
    assert max(abs(float(s)) for block in blocks64.values() for s in block) < 2.0 ** 40


def test_a_2_tuple_sets_the_2d_stencil_at_once_and_a_3_tuple_the_3d_one_on_first_use(monkeypatch):
    """The constructor's two routes on a stand-in context: (H, W) creates its context immediately and calls set_stencil, as before the 3-D
    form existed; (D, H, W) touches no context until `.ctx` is asked for, then calls set_stencil3d."""
    calls = []

    class Recorder:
        def __init__(self, *args, **kwargs):
            calls.append(("create",))

        def set_stencil(self, Hh, W):
            calls.append(("2d", Hh, W))

        def set_stencil3d(self, D, Hh, W):
            calls.append(("3d", D, Hh, W))

        def close(self):
            pass

    monkeypatch.setattr(hip, "HipContext", Recorder)
    op = fa.GradDivMap((6, 7))
    assert calls == [("create",), ("2d", 6, 7)]
    assert op.image_shape == (6, 7) and op.Vshape == (6, 7, 2) and op.Wshape == (6, 7)
    vol = fa.GradDivMap((2, 6, 7))
    assert len(calls) == 2 and vol._ctx is None
    vol.ctx
    assert calls[2:] == [("create",), ("3d", 2, 6, 7)]
