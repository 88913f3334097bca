"""What tests/test_tv3d_cpu.py and tests/test_gpu_tv3d.py share about the 3-D stencil operator (csrc/fh_tv3d.h): the fixtures of
scripts/make_tv3d_golden.py, the shapes the GPU tier walks, and the EXACT step -- operands that are multiples of 1/2 of small magnitude,
tau = 1/2, coef = 1/4 and an elementwise prox with thresholds that are multiples of 1/4, so that every vector entry of
init -> fwd -> adj -> fwd_adj -> adj(accel) is a multiple of 1/16 and every sum a small multiple of 1/256: exactly representable in float64 whatever
the order of the additions.  The model below is written once over an arithmetic (`FloatOps` in float64 or longdouble, `IntOps` in int64 on
the operands scaled by 32, where every value is an integer); the CPU tier checks that the three agree, the GPU tier compares the device with
`==`."""
import glob
import json
import os

import numpy as np

from fasta_python_amd import hip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tv3d")
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
FIELDS = ("residuals", "norm_residuals", "stepsizes", "objectives")
TWIN_AXES = (2, 0, 1)

# shapes where the kernels can go wrong: degenerate dimensions, dimensions of 2, sizes below / at / just past the 8 x 64 tile, several tiles
SHAPES = [(1, 1, 1), (1, 1, 5), (5, 1, 1), (2, 2, 2), (3, 4, 5), (5, 1, 7), (4, 33, 65), (17, 9, 130), (9, 40, 257)]
PLANES = 2                                   # FH_TUNE_TV3_PLANES of the GPU tier: several workgroups along d on these small volumes
TILE_H, TILE_W = 8, 64                       # csrc/fh_tv3d.h: TV3_TH, TV3_TW (asserted against fh_tv3d_shape where they are used)
# several workgroups on every axis and a ragged last tile on each
RAGGED = (2 * PLANES + 1, TILE_H + 1, 2 * TILE_W + 3)
ALL_SHAPES = SHAPES + [RAGGED]
TAU, COEF = 0.5, 0.25
PROX_KINDS = ("identity", "box", "shrink", "nonneg")            # rotating over the shapes


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return json.loads(str(z["meta"])), z, {k[3:]: z[k] for k in z.files if k.startswith("in_")}


def prefix_of(meta, z):
    """Iterations compared: all of them, or -- an adaptive run -- up to where the oracle parts from its twin."""
    return min(int(meta.get("twin_divergence", int(z["iteration_count"]))), int(z["iteration_count"]))


def owners(shape, sh):
    """How many workgroups of the geometry `sh` (hip.Tv3dShape) own each voxel: the launch rule of csrc/fh_tv3d.h:tv3_tile restated."""
    D, H, W = shape
    count = np.zeros(shape, dtype=np.int64)
    for ch in range(sh.chunks):
        for th in range(sh.tiles_h):
            for tw in range(sh.tiles_w):
                d0, h0, w0 = ch * sh.planes, th * sh.tile_h, tw * sh.tile_w
                assert d0 < D and h0 < H and w0 < W, "an empty workgroup"
                count[d0:min(d0 + sh.planes, D), h0:min(h0 + sh.tile_h, H), w0:min(w0 + sh.tile_w, W)] += 1
    return count


def div(Y):
    """oracle.problems.div in the dtype of its argument (the oracle's allocates float64)."""
    out = np.zeros(Y.shape[:-1], dtype=Y.dtype)
    for axis in range(Y.shape[-1]):
        comp = Y[..., axis]
        out += np.roll(comp, -1, axis=axis) - comp
    return out


def grad(X):
    """oracle.problems.grad in the dtype of its argument."""
    out = np.zeros(X.shape + (X.ndim,), dtype=X.dtype)
    for axis in range(X.ndim):
        out[..., axis] = np.roll(X, 1, axis=axis) - X
    return out


def exact_operands(shape, seed):
    """(x0, b): multiples of 1/2 in [-2, 2]."""
    rng = np.random.RandomState(seed)
    return rng.randint(-4, 5, size=tuple(shape) + (3,)) / 2.0, rng.randint(-4, 5, size=tuple(shape)) / 2.0


class FloatOps:
    """The step in a floating-point type, the operands as they are."""
    unit = 1

    def __init__(self, dtype=np.float64):
        self.dtype = dtype
        self.box = (dtype(-0.75), dtype(0.5))
        self.thr = dtype(TAU) * dtype(0.5)                  # tau * mu, mu = 1/2
        self.zero = dtype(0)

    def arr(self, a):
        return np.asarray(a, dtype=self.dtype)

    def times_tau(self, v):
        return self.dtype(TAU) * v

    def over_tau(self, v):
        return v / self.dtype(TAU)

    def times_coef(self, v):
        return self.dtype(COEF) * v


class IntOps:
    """The step in int64 on the operands scaled by 32: every vector entry is an integer, every division below is checked to be exact."""
    unit = 32

    def __init__(self):
        self.box = (-24, 16)
        self.thr = 8
        self.zero = 0

    def arr(self, a):
        s = np.asarray(a, dtype=np.float64) * 32
        assert np.array_equal(s, np.round(s))
        return s.astype(np.int64)

    @staticmethod
    def _exact_div(v, q):
        assert not np.any(v % q), "not a multiple"
        return v // q

    def times_tau(self, v):
        return self._exact_div(v, 2)

    def over_tau(self, v):
        return v * 2

    def times_coef(self, v):
        return self._exact_div(v, 4)


def prox_of(kind, ops):
    lo, hi = ops.box
    return {"identity": lambda x: x, "box": lambda x: np.minimum(np.maximum(x, lo), hi),
            "shrink": lambda x: np.sign(x) * np.maximum(np.abs(x) - ops.thr, ops.zero), "nonneg": lambda x: np.maximum(x, ops.zero)}[kind]


def prox_args(kind):
    """(kind, mu, lo, hi) of fh_set_prox for the exact step."""
    return {"identity": (hip.PROX_IDENTITY, 0.0, 0.0, 0.0), "box": (hip.PROX_BOX, 0.0, -0.75, 0.5), "shrink": (hip.PROX_SHRINK, 0.5, 0.0, 0.0),
            "nonneg": (hip.PROX_NONNEG, 0.0, 0.0, 0.0)}[kind]


def exact_step(x0, b, kind, ops):
    """The scalar blocks and vectors of init -> fwd -> adj -> fwd_adj -> adj(accel) in the arithmetic `ops`.  Returns (blocks, vectors): blocks[call] is
    the 16-entry block as the C ABI returns it (an entry a launch does not write keeps its value), with sums of products in units of
    ops.unit ** 2 and sums / maxima of magnitudes in units of ops.unit; vectors[name] in units of ops.unit."""
    x0, b = ops.arr(x0), ops.arr(b)
    prox = prox_of(kind, ops)
    sq = lambda v: (v * v).sum()
    blk = [ops.zero] * 16
    blocks, vec = {}, {}
    # fh_init: K-fwd of the plain operand (writes 0..7 and ALPHA), K-adj in mode 1 (writes 8..13), then the g terms of x0
    z0 = div(x0)
    g0 = grad(z0 - b)
    blk[0:8] = [sq(z0 - b)] + [ops.zero] * 7
    blk[hip.S_ALPHA] = ops.zero
    blk[8:14] = [ops.zero, ops.zero, sq(z0 - b), ops.zero, ops.zero, ops.zero]
    blk[hip.S_GSUM], blk[hip.S_GMAX] = np.abs(x0).sum(), np.abs(x0).max()
    blocks["init"], vec["g0"] = list(blk), g0
    # fh_fwd
    xhat = x0 - ops.times_tau(g0)
    xp = prox(xhat)
    z1 = div(xp)
    dx = xp - x0
    fwd = [sq(z1 - b), (dx * g0).sum(), sq(dx), sq(xp - xhat), sq(g0), np.abs(xp).sum(), np.abs(xp).max(), ((x0 - xp) * (xp - x0)).sum()]
    blk[0:8] = fwd
    blk[hip.S_ALPHA] = ops.zero
    blocks["fwd"] = list(blk)
    vec.update(xhat=xhat, xprox=xp, z=z1)
    # fh_adj, no acceleration
    def adj(zq, x1):
        r = zq - b
        g1 = grad(r)
        dg = g1 + ops.over_tau(xhat - x0)
        return g1, [(dx * dg).sum(), sq(dg), sq(r), sq(x1 - xhat), np.abs(x1).sum(), np.abs(x1).max()]
    g1, tail = adj(z1, xp)
    blk[8:14] = tail
    blocks["adj"], vec["g1"] = list(blk), g1
    blocks["fwd_adj"] = list(blk)                               # both launches under one synchronisation: the same block
    # fh_adj with the FISTA extrapolation (x_accel0 = x0 and z_accel0 = A x0 after fh_init)
    x1 = xp + ops.times_coef(xp - x0)
    zq = z1 + ops.times_coef(z1 - z0)
    g1a, tail = adj(zq, x1)
    blk[8:14] = tail
    blocks["adj_accel"] = list(blk)
    vec.update(x1=x1, g1_accel=g1a)
    return blocks, vec


PRODUCT_SLOTS = (hip.S_FSQ, hip.S_DXG0, hip.S_DX2, hip.S_XH2, hip.S_G02, hip.S_RDOT, hip.S_DXDG, hip.S_DG2, hip.S_FSQ_ADJ, hip.S_XH2_ADJ)


def block_as_float(block, ops):
    """A block of `exact_step` in the operands' own units, as float64 (exact: the integers involved are far below 2^53)."""
    out = np.zeros(16)
    for k, v in enumerate(block):
        unit = ops.unit ** 2 if k in PRODUCT_SLOTS else ops.unit
        if isinstance(v, (int, np.integer)):
            assert abs(int(v)) < 2 ** 53
            out[k] = int(v) / unit                              # (unit is a power of two: the quotient is exact)
        else:
            out[k] = np.float64(v)
            assert out[k] == v                                  # longdouble: the value is a float64
    return out
