"""What tests/test_screen_cpu.py and tests/test_gpu_screen.py share: shapes, dyadic problems, the path problems and the exact evaluation of the
gap-safe test (fasta_python_amd/certificates.py: screen; csrc/fh_screen.h).

Geometry.  The norms kernel gives a lane one 16-byte piece (2 float64 or 4 float32 columns) of a tile of 256 pieces and a slab of rows that is a
multiple of 16; the test kernel one feature per lane, 256 per workgroup; the gather a slab of rows per workgroup and 16-byte pieces of the
destination row.  So a side of 1 is one lane, 15 / 16 / 17 end inside, at and behind the row padding (and one piece row of the destination),
63 / 64 / 65 around a wave, 255 / 256 / 257 around a workgroup of the test and half a tile of the norms, 1000 is two tiles with a ragged one;
(3, 65537) is 129 tiles and (65537, 3) 4097 padded row groups under one narrow tile.

Exactness.  tests/gap_cases.py: entries of A are k/8 with |k| <= 8, so a squared entry is a multiple of 2^-6 at most 1 and a column's sum of at
most 65537 of them is exact in any order; the certificate of such a problem is exact.  From there on the test is a chain of single rounded
operations, spelled alike on both sides, with correctly rounded square roots: device and host agree with `==`.

The four path problems ("the fixture problems"): the stored sparse_ls_64x128 fixture; the matrix and labels of the logistic_100x160 fixture under
the least-squares loss (screening serves least squares only); the dense 64 x 128 and the CSR 40 x 60 problem of tests/test_gpu_gap.py's path test.
"""
import decimal
from fractions import Fraction

import numpy as np

from tests import gap_cases as G

SIDES = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000)
COLUMNS = (1, 2, 3, 16)
# every side value three times on each side: (S[i], S[i + k]) for k = 0, 4, 7; plus the two long ones
PAIRS = [(SIDES[i], SIDES[(i + k) % len(SIDES)]) for k in (0, 4, 7) for i in range(len(SIDES))] + [(3, 65537), (65537, 3)]
SHAPES = [(m, n, COLUMNS[i % 4]) for i, (m, n) in enumerate(PAIRS)]
IDS = ["%dx%dx%d" % s for s in SHAPES]
assert all({s[k] for s in SHAPES} >= set(SIDES) for k in (0, 1)) and {s[2] for s in SHAPES} == set(COLUMNS) and len(SHAPES) == 35

ONE_PLUS = Fraction(1) + Fraction(1, 2 ** 48)


def dyadic_problem(m, n, L, seed, group=False):
    return G.dyadic_problem(m, n, L, seed, group=group)


def exact_norms2(A):
    """sum_i a_ij^2 per column in rational arithmetic."""
    out = []
    for j in range(A.shape[1]):
        out.append(sum((Fraction(float(v)) ** 2 for v in A[:, j]), Fraction(0)))
    return out


def decimal_mask(cert, g, norms2, mu, kappa, group):
    """(keep, smallest relative distance of a feature's left side from mu) of the test at 50 digits, from the certificate's float64 entries."""
    decimal.getcontext().prec = 50
    D = decimal.Decimal
    frac = lambda v: D(Fraction(float(v)).numerator) / D(Fraction(float(v)).denominator)
    if cert.omega == 0.0 and cert.scale == 1.0:
        gs = D(0)
    else:
        guard = D(kappa) * D(2) ** -52 * (frac(cert.primal) + frac(cert.f) + 2 * (frac(cert.f) * frac(cert.f0)).sqrt())
        gs = max(frac(cert.gap) + guard, D(0))
    rho = (2 * gs).sqrt()
    s, one = frac(cert.scale), D(1) + D(2) ** -48
    G2 = np.asarray(g, dtype=np.float64).reshape(len(norms2), -1)
    keep, margin = [], None
    for j in range(len(norms2)):
        d = rho * frac(norms2[j]).sqrt()
        if group:
            lhs = [(s * sum((frac(v) ** 2 for v in G2[j]), D(0)).sqrt() + d) * one]
        else:
            lhs = [(s * abs(frac(v)) + d) * one for v in G2[j]]
        keep.append(not all(t < D(mu) for t in lhs))
        for t in lhs:
            rel = abs(t - frac(mu)) / frac(mu)
            margin = rel if margin is None or rel < margin else margin
    return np.array(keep), float(margin)


def path_problems():
    """name -> (A, b): the four problems the screened path is held to."""
    from scipy import sparse as sp
    from tests import helpers as H
    out = {}
    for name in ("sparse_ls_64x128_adaptive", "logistic_100x160_adaptive"):
        meta, z = H.load_case(name)
        d = H.case_data(meta, z)
        out[name.rsplit("_", 1)[0]] = (np.asarray(d["A"], dtype=np.float64), np.asarray(d["b"], dtype=np.float64))
    for sparse in (False, True):
        rng = np.random.RandomState(8)
        if sparse:
            A = sp.random(40, 60, density=0.2, format="csr", random_state=rng, data_rvs=rng.standard_normal)
            n = 60
        else:
            A = rng.randn(64, 128) / 8.0
            n = 128
        xt = np.zeros(n)
        xt[rng.permutation(n)[:5]] = 2.0 * rng.randn(5)
        out["csr40x60" if sparse else "dense64x128"] = (A, A @ xt + 0.01 * rng.randn(A.shape[0]))
    return out


PATH_NAMES = ("sparse_ls_64x128", "logistic_100x160", "dense64x128", "csr40x60")
PATH_OPTS = dict(n_mus=6, ratio=1e-2, gap_tolerance=1e-7, max_iters=5000)
