"""What tests/test_conv_cpu.py and tests/test_gpu_conv.py share about the periodic convolution operator (csrc/fh_conv.h): the fixtures of
scripts/make_conv_golden.py, the shapes the GPU tier walks, and the EXACT step -- operands that are multiples of 1/2 in [-2, 2], taps that are
small integers, a 0/1 mask, tau = 1/2, coef = 1/4 and an elementwise prox with thresholds that are multiples of 1/4, so that every vector entry
of init -> fwd -> adj -> fwd_adj -> adj(accel) is a multiple of 1/16 and every sum a multiple of 1/256 far below 2^53 of them: exactly representable
in float64 whatever the order of the additions.  The model is written once over an arithmetic (tests/tv3d_cases.py: `FloatOps` in float64 or
longdouble, `IntOps` in int64 on the operands scaled by 32, where every value is an integer); the CPU tier checks that the three agree, at 256
taps as well, the GPU tier compares the device with `==`."""
import glob
import json
import os

import numpy as np

from fasta_python_amd import hip
from tests.tv3d_cases import FloatOps, IntOps, block_as_float, prox_args, prox_of      # noqa: F401  (the arithmetics and the prox of the exact step)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv")
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
FIELDS = ("residuals", "norm_residuals", "stepsizes", "objectives")
TAU, COEF = 0.5, 0.25
PROX_KINDS = ("identity", "box", "shrink", "nonneg")            # rotating over the shapes
TILE_H, TILE_W = 32, 64                      # csrc/fh_host_launch.h: conv_shape_for (asserted against fh_conv_shape where they are used)
FLAT_W = 2048                                # ... and the tile of a signal (H == 1, kh == 1)
RAGGED = (2 * TILE_H + 3, 2 * TILE_W + 5)    # several workgroups on both axes and a ragged last tile on each

# (image shape, kernel shape, origin or None = (kh // 2, kw // 2), masked): where the kernels can go wrong
SHAPES = [
    ((1, 1), (1, 1), None, False),                      # one pixel, one tap
    ((1, 1), (3, 3), None, False),                      # every tap hits the one pixel
    ((1, 5), (1, 3), None, False), ((5, 1), (3, 1), None, True),
    ((1, 7), (3, 3), None, False),                      # H == 1 under a kernel with rows: not the flat tile
    ((2, 2), (5, 5), None, True),                       # the kernel is larger than the image: taps wrap more than once
    ((3, 4), (16, 16), None, False),                    # 256 taps
    ((4, 20), (16, 1), (3, 0), False), ((20, 3), (1, 16), (0, 12), True),
    ((7, 9), (2, 2), None, False), ((7, 9), (2, 2), (0, 0), True), ((7, 9), (2, 2), (1, 1), False),
    ((9, 11), (4, 6), None, True), ((9, 11), (4, 6), (0, 0), False), ((9, 11), (4, 6), (3, 5), False),
    ((TILE_H - 1, TILE_W - 1), (3, 3), None, False),    # one below, at, and one past the tile on each axis
    ((TILE_H, TILE_W), (3, 5), None, True),
    ((TILE_H + 1, TILE_W + 1), (5, 3), None, False),
    ((TILE_H + 1, TILE_W - 1), (16, 16), (2, 13), False),
    (RAGGED, (7, 9), None, True),
    ((300,), (15,), None, False),                       # a signal: the flat tile
    ((FLAT_W - 1,), (4,), (0,), True), ((FLAT_W,), (3,), None, False), ((FLAT_W + 1,), (16,), (15,), False),
]
IDS = ["x".join(map(str, s)) + "-k" + "x".join(map(str, k)) + ("" if o is None else "-o" + "_".join(map(str, o))) + ("-mask" if m else "")
       for s, k, o, m in SHAPES]


def shape2d(shape):
    return tuple(shape) if len(shape) == 2 else (1, shape[0])


def origin2d(kshape, origin):
    kh, kw = shape2d(kshape)
    if origin is None:
        return kh // 2, kw // 2
    return (0, origin[0]) if len(origin) == 1 else tuple(origin)


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return json.loads(str(z["meta"])), z, {k[3:]: z[k] for k in z.files if k.startswith("in_")}


def prefix_of(meta, z):
    """Iterations compared: all of them, or -- an adaptive run -- up to where the oracle parts from its twin."""
    return min(int(meta.get("twin_divergence", int(z["iteration_count"]))), int(z["iteration_count"]))


def owners(shape, sh):
    """How many workgroups of the geometry `sh` (hip.ConvShape) own each pixel: the launch rule of csrc/fh_conv.h:conv_tile restated."""
    H, W = shape2d(shape)
    count = np.zeros((H, W), dtype=np.int64)
    for th in range(sh.tiles_h):
        for tw in range(sh.tiles_w):
            h0, w0 = th * sh.tile_h, tw * sh.tile_w
            assert h0 < H and w0 < W, "an empty workgroup"
            count[h0:min(h0 + sh.tile_h, H), w0:min(w0 + sh.tile_w, W)] += 1
    return count


def conv(x, K, origin, mask=None, adjoint=False):
    """The operator's definition in the dtype of `x` (float64, longdouble or int64): NumPy's `out += K[a,b] * np.roll(...)`, a outer, b inner;
    the mask last in A, first in A^T."""
    shape = x.shape
    x = x.reshape(shape2d(shape))
    K = np.asarray(K).reshape(shape2d(np.shape(K)))
    oh, ow = origin
    if mask is not None:
        mask = np.asarray(mask).reshape(x.shape).astype(x.dtype)
    if adjoint and mask is not None:
        x = mask * x
    sign = -1 if adjoint else 1
    out = np.zeros(x.shape, dtype=x.dtype)
    for a in range(K.shape[0]):
        for b in range(K.shape[1]):
            out += K[a, b].astype(x.dtype) * np.roll(x, (sign * (a - oh), sign * (b - ow)), axis=(0, 1))
    if not adjoint and mask is not None:
        out = mask * out
    return out.reshape(shape)


def exact_operands(case, seed):
    """(x0, b, K, origin, mask) of a SHAPES entry: x0 and b multiples of 1/2 in [-2, 2], integer taps in [-2, 2], a 0/1 mask or None.  A kernel
    of more than 12 taps keeps about 12 of them non-zero (at seeded places; the device visits the zero taps all the same), or two applications
    of the operator and its adjoint would carry the sums of the step past 2^53 units."""
    shape, kshape, origin, masked = case
    rng = np.random.RandomState(seed)
    x0, b = rng.randint(-4, 5, size=shape) / 2.0, rng.randint(-4, 5, size=shape) / 2.0
    K = rng.randint(-2, 3, size=kshape).astype(np.float64)
    K *= rng.rand(*kshape) < 12.0 / K.size
    mask = (rng.rand(*shape) < 0.7).astype(np.float64) if masked else None
    return x0, b, K, origin2d(kshape, origin), mask


def exact_step(x0, b, K, origin, mask, kind, ops):
    """The scalar blocks and vectors of init -> fwd -> adj -> fwd_adj -> adj(accel) in the arithmetic `ops` (tests/tv3d_cases.py:exact_step over this
    operator).  Returns (blocks, vectors): blocks[call] is the 16-entry block as the C ABI returns it, with sums of products in units of
    ops.unit ** 2 and sums / maxima of magnitudes in units of ops.unit; vectors[name] in units of ops.unit."""
    x0, b = ops.arr(x0), ops.arr(b)
    Kt = np.asarray(K, dtype=x0.dtype)               # the taps are integers: never scaled
    assert np.array_equal(Kt, np.asarray(K))
    A = lambda v: conv(v, Kt, origin, mask)
    At = lambda v: conv(v, Kt, origin, mask, adjoint=True)
    prox = prox_of(kind, ops)
    sq = lambda v: (v * v).sum()
    blk = [ops.zero] * 16
    blocks, vec = {}, {}
    z0 = A(x0)
    g0 = At(z0 - b)
    blk[0:8] = [sq(z0 - b)] + [ops.zero] * 7
    blk[hip.S_ALPHA] = ops.zero
    blk[8:14] = [ops.zero, ops.zero, sq(z0 - b), ops.zero, ops.zero, ops.zero]
    blk[hip.S_GSUM], blk[hip.S_GMAX] = np.abs(x0).sum(), np.abs(x0).max()
    blocks["init"], vec["g0"] = list(blk), g0
    xhat = x0 - ops.times_tau(g0)
    xp = prox(xhat)
    z1 = A(xp)
    dx = xp - x0
    blk[0:8] = [sq(z1 - b), (dx * g0).sum(), sq(dx), sq(xp - xhat), sq(g0), np.abs(xp).sum(), np.abs(xp).max(), ((x0 - xp) * (xp - x0)).sum()]
    blk[hip.S_ALPHA] = ops.zero
    blocks["fwd"] = list(blk)
    vec.update(xhat=xhat, xprox=xp, z=z1)

    def adj(zq, x1):
        r = zq - b
        g1 = At(r)
        dg = g1 + ops.over_tau(xhat - x0)
        return g1, [(dx * dg).sum(), sq(dg), sq(r), sq(x1 - xhat), np.abs(x1).sum(), np.abs(x1).max()]
    g1, tail = adj(z1, xp)
    blk[8:14] = tail
    blocks["adj"], vec["g1"] = list(blk), g1
    blocks["fwd_adj"] = list(blk)                               # both launches under one synchronisation: the same block
    x1 = xp + ops.times_coef(xp - x0)
    zq = z1 + ops.times_coef(z1 - z0)
    g1a, tail = adj(zq, x1)
    blk[8:14] = tail
    blocks["adj_accel"] = list(blk)
    vec.update(x1=x1, g1_accel=g1a)
    return blocks, vec


# ---- the fixtures' problems (scripts/make_conv_golden.py captures them, both tiers solve them) ---------------------------------------------------
def problem_of(meta, d):
    """(ConvMap arguments, prox tag or None) of a fixture."""
    import fasta_python_amd as fa
    origin = tuple(meta["origin"]) if meta["origin"] is not None else None
    if origin is not None and d["b"].ndim == 1:
        origin = origin[0]
    kwargs = dict(shape=d["b"].shape, kernel=d["kernel"], origin=origin, mask=d.get("mask"))
    mu = float(d["mu"])
    lo, hi = (float(v) for v in meta.get("box", (0.0, 0.0)))
    tag = {"shrink": lambda: fa.Shrink(mu), "nonneg": fa.NonNeg, "box": lambda: fa.Box(lo, hi), "linf": lambda: fa.LinfProx(mu),
           "l1ball": lambda: fa.L1Ball(mu), "none": lambda: None}[meta["prox"]]()
    return kwargs, tag
