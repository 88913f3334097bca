"""What tests/test_gpu_path_calls.py and the fixture tests/golden/path_calls.json share: eight calls of fasta_python_amd.path() and a HipContext
that writes down the name of every method called on it, in order.  Equal names in equal order on equal shapes are equal launches and equal
transfers: the fixture is what a change to regpath.py that is meant to cost nothing must reproduce with `==`.

    python -m tests.path_call_cases <commit>        # on the GPU, on the commit whose sequences are to be kept: writes the fixture

A record is "<k>:<method>": k counts the contexts of one path() call in the order they were created (0 the operator's, 1 the working
operator's of the screened path).  Only calls from outside the context are recorded (a method that calls another method of the context is one
call), properties are not.  The solves run under driver="library" with device_iters=10, so that the number of fh_iterate calls follows from the
iteration counts alone and not from how long a call took.

The data is seeded, 12 x 9, and chosen so that the screened cases pass through all three branches of a screening round
(tests/test_path_calls_cpu.py holds them to it on the host path): a round that compacts, a round that keeps more than half of the features and
runs on the full operator, and a point at which every feature is screened.  The last needs a warm start that is not zero above the critical mu, so the screened
vector cases pass their own grid of three and an x0; the others take the default grid from the critical mu, n_mus=3."""
import json
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "path_calls.json")
M, N = 12, 9
OPTS = dict(gap_tolerance=1e-8, max_iters=400, driver="library", device_iters=10)


def problem(sparse=False, columns=None):
    """(A, b, critical mu of the l1 / group problem, a small x0 that is not zero)."""
    rng = np.random.RandomState(5)
    A = rng.randn(M, N) / 3.0
    if sparse:
        from scipy import sparse as sp
        A = sp.csr_matrix(A * (rng.rand(M, N) < 0.45))
    xt = np.zeros((N,) + (() if columns is None else (columns,)))
    xt[[1, 6]] = 2.0 * rng.randn(*xt[[1, 6]].shape)
    b = A @ xt + 0.01 * rng.randn(*(A @ xt).shape)
    g = np.asarray(A.T @ b)
    mu_max = float(np.abs(g).max() if columns is None else np.sqrt((g * g).sum(axis=1)).max())
    x0 = np.zeros_like(xt)
    x0[3] = 1e-3
    return A, b, mu_max, x0


# id -> (sparse, columns, caller-owned map, keywords of path()); "grid": the case passes `mus`, in units of the critical mu, and `x0` (see the module text)
CASES = {
    "dense": (False, None, False, dict(screen=False)),
    "dense_screen": (False, None, False, dict(screen=True, grid=(1.25, 0.5, 0.05))),
    "dense_screen_standardize_intercept": (False, None, False, dict(screen=True, standardize=True, intercept=True)),
    "dense_group_screen": (False, 2, False, dict(screen=True, ratio=0.2)),
    "csr": (True, None, False, dict(screen=False)),
    "csr_screen": (True, None, False, dict(screen=True, grid=(1.25, 0.6, 0.3))),
    "csr_standardize": (True, None, False, dict(standardize=True)),
    "dense_map_of_the_caller": (False, None, True, dict(screen=False)),
}
assert len(CASES) == 8


def arguments(cid, backend):
    """(A, loss, prox class, keywords) of the case's path() call; a caller-owned case gets its DenseMatrixMap (lazy: no context yet)."""
    import fasta_python_amd as fa
    sparse, columns, owned, kw = CASES[cid]
    kw = dict(kw)
    A, b, mu_max, x0 = problem(sparse, columns)
    grid = kw.pop("grid", None)
    if grid is not None:
        kw.update(mus=[f * mu_max for f in grid], x0=x0)
    elif columns is not None:
        kw.update(x0=np.zeros((N, columns)))
    if owned:
        A = fa.DenseMatrixMap(A)
    return A, fa.LeastSquares(b), (fa.GroupShrink if columns is not None else fa.Shrink), dict(n_mus=3, backend=backend, **OPTS, **kw)


def run(cid, backend):
    import warnings
    import fasta_python_amd as fa
    A, loss, prox_class, kw = arguments(cid, backend)
    np.random.seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return A, fa.path(A, loss, prox_class, **kw)


# ---- the recording context ---------------------------------------------------------------------------------------------------------------------------
def recording(log):
    """A subclass of hip.HipContext that appends "<k>:<method>" to `log` for every public method called on it from outside."""
    from fasta_python_amd import hip
    base, depth, born = hip.HipContext, [0], [0]

    class Recording(base):
        def __init__(self, *args, **kwargs):
            object.__setattr__(self, "_k", born[0])
            born[0] += 1
            base.__init__(self, *args, **kwargs)

        def __del__(self):                              # (the collector's close() is nobody's call)
            depth[0] += 1
            try:
                base.__del__(self)
            finally:
                depth[0] -= 1

        def __getattribute__(self, name):
            attr = object.__getattribute__(self, name)
            if name.startswith("_") or name == "lib" or not callable(attr):
                return attr

            def call(*args, **kwargs):
                if depth[0] == 0:
                    log.append("%d:%s" % (object.__getattribute__(self, "_k"), name))
                depth[0] += 1
                try:
                    return attr(*args, **kwargs)
                finally:
                    depth[0] -= 1
            return call

    return Recording


def record(cid):
    """(the names, the map of a caller-owned case or None): the case's path() call with every context of the package a recording one."""
    from fasta_python_amd import hip
    log = []
    plain = hip.HipContext
    hip.HipContext = recording(log)
    try:
        A, out = run(cid, "hip")
    finally:
        hip.HipContext = plain
    assert len(out) == 3
    return log, (A if CASES[cid][2] else None)


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def write_golden(commit, cases):
    """One line per case."""
    with open(GOLDEN, "w") as f:
        f.write('{"commit": %s, "cases": {\n' % json.dumps(commit))
        f.write(",\n".join("%s: %s" % (json.dumps(cid), json.dumps(cases[cid])) for cid in sorted(cases)))
        f.write("\n}}\n")


def main(commit):
    cases = {}
    for cid in CASES:
        log, op = record(cid)
        cases[cid] = list(log)                          # (before the caller's own close(), which is not a call of path())
        if op is not None:
            op.close()
        print(cid, len(log), "calls", flush=True)
    write_golden(commit, cases)
    print("wrote", GOLDEN)


if __name__ == "__main__":
    main(sys.argv[1])
