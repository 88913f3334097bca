"""Shared by tests/test_softmax_cpu.py and tests/test_gpu_softmax.py: the softmax fixtures (tests/golden/softmax, captured by
scripts/make_softmax_golden.py), a `longdouble` evaluation of the loss, the error bounds of the issue, and a NumPy model of k_sm_rows
(csrc/fh_softmax.h): its lane layout, its exchanges and the order of every sum, in float64."""
import importlib.util
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "softmax")
CASES = ["group_60x40x3_adaptive", "group_60x40x3_accelerated", "group_60x40x3_plain", "group_60x40x3_backtracks", "group_50x70x5_adaptive",
         "l1_80x30x2_accelerated", "l1_97x33x16_adaptive", "sparse_120x90x7_adaptive", "sparse_120x90x7_accelerated", "noprox_40x20x4_plain",
         "estimated_60x40x3_adaptive"]
ALL_L = [2, 3, 4, 5, 8, 9, 16]                      # every LB (2, 4, 8, 16), with and without padding columns
WG = 256

_script = None


def capture_script():
    """scripts/make_softmax_golden.py as a module: the case table, the constructors and the closures are stated there, once."""
    global _script
    if _script is None:
        spec = importlib.util.spec_from_file_location("make_softmax_golden", os.path.join(ROOT, "scripts", "make_softmax_golden.py"))
        _script = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_script)
    return _script


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    return meta, z, {k[3:]: z[k] for k in z.files if k.startswith("in_")}


def lb_of(L):
    return 2 if L <= 2 else 4 if L <= 4 else 8 if L <= 8 else 16


# ---- longdouble evaluation -------------------------------------------------------------------------------------------------------------------
def longdouble_rows(Z, y):
    """(residual, per-row terms, per-row magnitudes |mx| + log s + |z_y|) in longdouble from the float64-rounded d = z - mx."""
    Z = np.asarray(Z, dtype=np.float64)
    m, L = Z.shape
    mx = Z.max(axis=1)
    d = (Z - mx[:, None]).astype(np.longdouble)
    e = np.exp(d)
    s = e.sum(axis=1)
    Y = np.zeros((m, L), dtype=np.longdouble)
    Y[np.arange(m), y] = 1
    zy = Z[np.arange(m), y].astype(np.longdouble)
    terms = (mx.astype(np.longdouble) + np.log(s)) - zy
    mags = np.abs(mx.astype(np.longdouble)) + np.log(s) + np.abs(zy)
    return e / s[:, None] - Y, terms, mags


def residual_bound(L):
    """Per-entry bound on the residual error: exp at 1 ulp, at most L - 1 additions, one division, one subtraction, probabilities <= 1; the
    factor 2 is margin."""
    return 2.0 * (L + 3) * 2.0 ** -53


def loss_bound(m, L, mags):
    return float(2.0 ** -52 * ((m + 4) * np.sum(mags) + m * (L + 2)))


# ---- the kernel, lane by lane ------------------------------------------------------------------------------------------------------------------
def _xor(v, mask):
    return v[np.arange(v.size) ^ mask]


def _wave_sum(v):
    """fh_device.h: wave_sum over 64 lanes."""
    i = np.arange(64)
    v = v + v[i ^ 1]
    v = v + v[i ^ 2]
    v = v + v[(i & ~7) | (7 - (i & 7))]
    v = v + v[(i & ~15) | (15 - (i & 15))]
    return ((v[0] + v[16]) + v[32]) + v[48]


def _block_sum(v):
    """fh_device.h: block_reduce<1> of a 256-thread workgroup (sum)."""
    w = [_wave_sum(v[64 * k:64 * k + 64]) for k in range(4)]
    return ((w[0] + w[1]) + w[2]) + w[3]


def ordered_records_sum(rec):
    """csrc/fh_softmax.h: sm_sum_records."""
    v = np.zeros(WG)
    for t in range(min(WG, rec.size)):
        for i in range(t, rec.size, WG):
            v[t] = v[t] + rec[i]
    return _block_sum(v)


def kernel_model(Z, y, L, zacc0=None, coef=0.0):
    """k_sm_rows<LB> on an (m, L) matrix: (R (m, LB), per-row terms, per-workgroup records, loss).  Every lane of a workgroup is simulated:
    thread t of workgroup w holds column pair (w * 256 + t) % C of row (w * 256 + t) // C."""
    Z = np.asarray(Z, dtype=np.float64)
    m = Z.shape[0]
    LB = lb_of(L)
    C = LB // 2
    Zp, Bp = np.zeros((m, LB)), np.zeros((m, LB))
    Zp[:, :L] = Z
    if zacc0 is not None:
        Ap = np.zeros((m, LB))
        Ap[:, :L] = zacc0
        Zp = Zp + coef * (Zp - Ap)                                         # extrapolate(): d = v - vprev, s = coef * d, v + s
    Bp[np.arange(m), y] = 1.0
    nwg = (m * C + WG - 1) // WG
    R, terms, rec = np.zeros((m, LB)), np.zeros(m), np.zeros(nwg)
    lane = np.arange(WG)
    c = lane % C
    for w in range(nwg):
        i = w * WG + lane
        live = i < m * C
        row = np.where(live, i // C, 0)
        zx = np.where(live, Zp[row, 2 * c], 0.0)
        zy_ = np.where(live, Zp[row, 2 * c + 1], 0.0)
        bx = np.where(live, Bp[row, 2 * c], 0.0)
        by = np.where(live, Bp[row, 2 * c + 1], 0.0)
        v0, v1 = 2 * c < L, 2 * c + 1 < L
        mx = np.maximum(np.where(v0, zx, -np.inf), np.where(v1, zy_, -np.inf))
        for mask in (1, 2, 4):
            if C > mask:
                mx = np.maximum(mx, _xor(mx, mask))
        with np.errstate(invalid="ignore"):
            e0 = np.where(v0, np.exp(zx - mx), 0.0)
            e1 = np.where(v1, np.exp(zy_ - mx), 0.0)
        a = np.zeros((LB, WG))
        a[0], a[1] = e0, e1
        cur = 2
        for mask in (1, 2, 4):                                             # sm_gather_step
            if cur < LB:
                upper = (c & mask) != 0
                for k in range(cur):
                    mine = a[k].copy()
                    theirs = _xor(mine, mask)
                    a[k] = np.where(upper, theirs, mine)
                    a[k + cur] = np.where(upper, mine, theirs)
                cur *= 2
        s = a[0].copy()
        for k in range(1, LB):
            s = s + a[k]
        t = np.where(bx == 1.0, zx, 0.0) + np.where(by == 1.0, zy_, 0.0)
        for mask in (1, 2, 4):                                             # spmc_tree<1, C>
            if C > mask:
                t = t + _xor(t, mask)
        rx = np.where(v0, e0 / s - bx, 0.0)
        ry = np.where(v1, e1 / s - by, 0.0)
        term = np.where(live & (c == 0), (mx + np.log(s)) - t, 0.0)
        for q in np.nonzero(live)[0]:
            R[row[q], 2 * c[q]], R[row[q], 2 * c[q] + 1] = rx[q], ry[q]
            if c[q] == 0:
                terms[row[q]] = term[q]
        rec[w] = _block_sum(term)
    return R, terms, rec, ordered_records_sum(rec)
