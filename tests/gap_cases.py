"""What tests/test_gpu_gap.py shares: the shapes at which a slab, a wave or a tail of the certificate's launches (csrc/fh_gap.h) can go wrong,
dyadic problems on which the least-squares record is exact in float64, and the bounds the comparisons are held to.

Geometry (csrc/fasta_hip.hip: gap_slabs).  A side of R rows is cut into k = min(256, ceil(R / 256)) slabs of round_up(ceil(R / k), 64) rows, one
workgroup of 256 lanes (4 waves) each, a lane owning whole rows.  So R = 1 is one lane; 63 / 64 / 65 end inside, at and behind the first wave;
255 / 256 / 257 end inside, at and behind one pass of a workgroup and, at 257, open a second workgroup whose slab holds 65 rows; 1000 is four
slabs with a ragged last one; 65537 is 256 slabs of 320 rows of which the last 51 are EMPTY (205 * 320 >= 65537) and the 205th holds 257 rows.
Every value stands on each side at least once; L in {1, 2, 3, 16} covers the vector form and LB = 2, 4, 16 with and without padding columns.

Exactness.  Entries of A are k/8 with |k| <= 8, of b k/8 with |k| <= 16, x has at most 8 non-zero rows with entries k/8, |k| <= 8 (for the group
norm: integer multiples of (3, 4) / 8, (0, 5) / 8, (2, 3, 6) / 8 ..., whose row norms are rational).  Then z = A x is a multiple of 2^-6 below 2^4,
r = z - b below 2^5, g = A^T r a multiple of 2^-9 below 2^22; r^2 a multiple of 2^-12 below 2^10, and the sums over at most 65537 * 16 < 2^21 entries
stay below 2^31 at a resolution of 2^-12: 43 bits.  Every product and sum of the record is exact, whatever its order, so device and host agree with
`==` -- and so do the quotient s = mu / Omega°, a single correctly rounded division of equal operands, and the products formed from it in the same order.
"""
import math

import numpy as np

EPS = 2.0 ** -52

SIDES = (1, 63, 64, 65, 255, 256, 257, 1000, 65537)
COLUMNS = (1, 2, 3, 16)
# (m, n, L): not the full product; every value of SIDES on each side, every L
SHAPES = [(1, 65537, 1), (65537, 1, 1), (63, 64, 1), (64, 65, 2), (65, 63, 3), (255, 256, 16), (256, 257, 1), (257, 255, 2), (1000, 63, 3),
          (64, 1000, 16), (1, 65537, 3), (65537, 1, 16), (1000, 1000, 1)]
IDS = ["%dx%dx%d" % s for s in SHAPES]
assert {s[0] for s in SHAPES} == set(SIDES) == {s[1] for s in SHAPES} and {s[2] for s in SHAPES} == set(COLUMNS)

PATTERNS = {1: [[1], [2], [5]], 2: [[3, 4], [0, 5], [4, 3], [5, 0]], 3: [[3, 4, 0], [0, 0, 5], [2, 3, 6], [6, 2, 3]]}


def slabs(rows):
    """(workgroups, rows per slab) of one side: csrc/fasta_hip.hip:gap_slabs."""
    k = min(max(-(-rows // 256), 1), 256)
    return k, -(-(-(-rows // k)) // 64) * 64


def dyadic_problem(m, n, L, seed, group=False):
    """(A, b, x): A (m, n), b (m,) or (m, L), x (n,) or (n, L) as the module text says."""
    rng = np.random.RandomState(seed)
    A = rng.randint(-8, 9, size=(m, n)) / 8.0
    cols = () if L == 1 else (L,)
    b = rng.randint(-16, 17, size=(m,) + cols) / 8.0
    x = np.zeros((n, L))
    rows = rng.permutation(n)[:min(n, 8)]
    if group:                                      # rows with rational norms: an integer multiple of a pattern in the leading columns, zeros behind
        pats = PATTERNS[min(L, 3)]
        for j in rows:
            x[j, :min(L, 3)] = np.array(pats[rng.randint(len(pats))]) * rng.randint(-2, 3) / 8.0
            x[j] = np.roll(x[j], rng.randint(L))      # (anywhere in the row, padding columns' neighbours included)
    else:
        x[rows] = rng.randint(-8, 9, size=(len(rows), L)) / 8.0
    return A, b, x.reshape((n,) + cols)


def logistic_problem(m, n, seed):
    """(A, labels, x): |z| stays of order one, so that log(1 + e^z) - y z keeps most of its bits (the loss kernels' expression cancels for large y z)."""
    rng = np.random.RandomState(seed)
    A = rng.randn(m, n) / math.sqrt(n)
    x = rng.randn(n) * (rng.rand(n) < 0.5)
    labels = np.where(rng.rand(m) < 0.5, 1.0, -1.0)
    return A, labels, x


def fsum_bound(terms):
    """(math.fsum of the terms, 32 eps sum |term|): a few roundings per term, exp / log to an ulp, a summation tree of depth <= 32."""
    t = [float(v) for v in np.ravel(terms)]
    return math.fsum(t), 32 * EPS * math.fsum(abs(v) for v in t)
