"""The n-side arithmetic of one element as it ships -- fasta_python_amd/csrc/fh_nside.h: nside_fwd_sums and nside_adj_sums, which every second-tier
kernel calls -- built for the host from tests/csrc/nside_shim.cpp and checked against the reference's expressions (fasta/__init__.py:181-270):

  exactly representable inputs   every sum is exact in any order, so every slot must equal the NumPy expression bit for bit: which term goes
                                 to which slot, with and without acceleration, with and without the sum of |x|;
  general doubles                xhat, x1 and Dg must equal NumPy's two-rounding expressions bit for bit, and every fma sum the chain of
                                 ONCE-rounded exact values a*b + c (math.fma, or exact rationals), elements in index order.
A missing compiler is an error, not a skip.  No sanitizer: the library is loaded into this interpreter as it is."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_pd = C.POINTER(C.c_double)
N = 300


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("nside_shim")), "nside_shim.so")
    cmd = [os.environ.get("CXX") or "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas",
           "-I", os.path.join(ROOT, "fasta_python_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "csrc", "nside_shim.cpp")]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    lib.ns_shim_fwd_point.restype, lib.ns_shim_fwd_point.argtypes = None, [C.c_int, _pd, _pd, C.c_double, _pd]
    lib.ns_shim_dgrad.restype, lib.ns_shim_dgrad.argtypes = None, [C.c_int, _pd, _pd, _pd, C.c_double, _pd]
    lib.ns_shim_fwd_sums.restype, lib.ns_shim_fwd_sums.argtypes = None, [C.c_int, C.c_int, _pd, _pd, _pd, _pd, _pd, C.c_int, _pd]
    lib.ns_shim_adj_sums.restype = None
    lib.ns_shim_adj_sums.argtypes = [C.c_int, _pd, _pd, _pd, _pd, _pd, C.c_int, C.c_double, C.c_double, C.c_int, _pd, _pd]
    return lib


def _p(a):
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(_pd)


def fwd_point(lib, x0, g0, tau):
    out = np.empty_like(x0)
    lib.ns_shim_fwd_point(len(x0), _p(x0), _p(g0), tau, _p(out))
    return out


def dgrad(lib, g1, xhat, x0, tau):
    out = np.empty_like(x0)
    lib.ns_shim_dgrad(len(x0), _p(g1), _p(xhat), _p(x0), tau, _p(out))
    return out


def fwd_sums(lib, with_fsq, x0, g0, xhat, xp, xav, gsum=True):
    v = np.full(8, np.nan)
    lib.ns_shim_fwd_sums(len(x0), int(with_fsq), _p(x0), _p(g0), _p(xhat), _p(xp), _p(xav), int(gsum), _p(v))
    return v


def adj_sums(lib, g1, x0, xp, xacc0, xhat, accel, coef, tau, gsum=True):
    v, x1 = np.full(5, np.nan), np.empty_like(x0)
    lib.ns_shim_adj_sums(len(x0), _p(g1), _p(x0), _p(xp), _p(xacc0), _p(xhat), int(accel), coef, tau, int(gsum), _p(v), _p(x1))
    return v, x1


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def shrink(x, t):
    return np.sign(x) * np.maximum(np.abs(x) - t, 0.0)


# ---- exactly representable inputs ---------------------------------------------------------------------------------------------------------------
def exact_set(seed):
    """small integers times powers of two: every difference, product and partial sum below is exact (multiples of 2^-12 far below 2^53 * 2^-12)"""
    r = np.random.default_rng(seed)
    def draw():
        return r.integers(-12, 13, N).astype(np.float64) * 2.0 ** r.integers(-2, 3, N)
    x0, g0, xacc0, g1 = draw(), draw(), draw(), draw()
    x0[:3] = [0.0, -0.0, 3.0]
    return x0, g0, xacc0, g1


@pytest.mark.parametrize("with_fsq", [False, True])
@pytest.mark.parametrize("gsum", [True, False])
@pytest.mark.parametrize("tau", [0.25, 2.0])
def test_forward_slots_exact(shim, with_fsq, gsum, tau):
    x0, g0, xacc0, _ = exact_set(11)
    xhat = fwd_point(shim, x0, g0, tau)
    assert same_bits(xhat, x0 - tau * g0)                                                  # :181
    xp = shrink(xhat, 0.5)
    xp[5] = x0[5]                                                                            # an element the prox left where it was
    v = fwd_sums(shim, with_fsq, x0, g0, xhat, xp, xacc0, gsum)
    o = 1 if with_fsq else 0
    dx = xp - x0                                                                             # :186
    want = [np.sum(dx * g0), np.sum(dx * dx), np.sum((xp - xhat) ** 2), np.sum(g0 * g0),      # :200, :200, :274, :274
            np.sum(np.abs(xp)) if gsum else 0.0, np.max(np.abs(xp)),
            np.sum((x0 - xp) * (xp - xacc0))]                                                # :231
    assert same_bits(v[o:o + 7], np.array(want))
    assert same_bits(np.delete(v, np.arange(o, o + 7)), np.zeros(1))                         # the eighth slot is the caller's


@pytest.mark.parametrize("accel", [False, True])
@pytest.mark.parametrize("gsum", [True, False])
@pytest.mark.parametrize("tau,coef", [(0.5, 0.25), (4.0, 0.5)])
def test_adjoint_slots_exact(shim, accel, gsum, tau, coef):
    x0, g0, xacc0, g1 = exact_set(12)
    xhat = x0 - tau * g0
    xp = shrink(xhat, 0.5)
    xp[5] = x0[5]
    v, x1 = adj_sums(shim, g1, x0, xp, xacc0, xhat, accel, coef, tau, gsum)
    x1_np = xp + coef * (xp - xacc0) if accel else xp                                        # :242
    assert same_bits(x1, x1_np)
    dg = g1 + (xhat - x0) / tau                                                              # :254
    assert same_bits(dgrad(shim, g1, xhat, x0, tau), dg)
    dx = xp - x0
    want = [np.sum(dx * dg), np.sum(dg * dg), np.sum((x1_np - xhat) ** 2),                    # :255, :260, :274 at the extrapolated point
            np.sum(np.abs(x1_np)) if gsum else 0.0, np.max(np.abs(x1_np))]
    assert same_bits(v, np.array(want))


# ---- general doubles ----------------------------------------------------------------------------------------------------------------------------
def fma_once(a, b, c):
    """a*b + c rounded once"""
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def fma_chain(a, b):
    acc = 0.0
    for x, y in zip(a.tolist(), b.tolist()):
        acc = fma_once(x, y, acc)
    return acc


def add_chain(a):
    acc = 0.0
    for x in a.tolist():
        acc = acc + x
    return acc


def general_set(seed):
    r = np.random.default_rng(seed)
    def draw():
        return r.standard_normal(N) * 10.0 ** r.integers(-3, 4, N)
    x0, g0, xacc0, g1 = draw(), draw(), draw(), draw()
    x0[:4] = [0.0, -0.0, 5e-324, 1.5]
    g0[:4] = [-0.0, 0.0, 2.5e-310, -0.0]
    xacc0[:4] = [-0.0, 0.0, -5e-324, 1.5]
    return x0, g0, xacc0, g1


@pytest.mark.parametrize("tau", [0.3, 1.7e-3])
def test_forward_general(shim, tau):
    x0, g0, xacc0, _ = general_set(21)
    xhat = fwd_point(shim, x0, g0, tau)
    assert same_bits(xhat, x0 - tau * g0)                                                  # two roundings, never one
    xp = shrink(xhat, 0.05)
    xp[7] = x0[7]                                                                            # xp == x0: Dx = +0.0
    v = fwd_sums(shim, True, x0, g0, xhat, xp, xacc0)
    dx, dh = xp - x0, xp - xhat
    want = [0.0, fma_chain(dx, g0), fma_chain(dx, dx), fma_chain(dh, dh), fma_chain(g0, g0), add_chain(np.abs(xp)), np.max(np.abs(xp)),
            fma_chain(x0 - xp, xp - xacc0)]
    assert same_bits(v, np.array(want))


@pytest.mark.parametrize("accel", [False, True])
@pytest.mark.parametrize("tau,coef", [(0.3, 0.41), (1.7e-3, 0.93)])
def test_adjoint_general(shim, accel, tau, coef):
    x0, g0, xacc0, g1 = general_set(22)
    xhat = x0 - tau * g0
    xp = shrink(xhat, 0.05)
    xp[7] = x0[7]
    v, x1 = adj_sums(shim, g1, x0, xp, xacc0, xhat, accel, coef, tau)
    x1_np = xp + coef * (xp - xacc0) if accel else xp
    assert same_bits(x1, x1_np)
    dg = g1 + (xhat - x0) / tau
    assert same_bits(dgrad(shim, g1, xhat, x0, tau), dg)
    dx, dh = xp - x0, x1_np - xhat
    want = [fma_chain(dx, dg), fma_chain(dg, dg), fma_chain(dh, dh), add_chain(np.abs(x1_np)), np.max(np.abs(x1_np))]
    assert same_bits(v, np.array(want))
