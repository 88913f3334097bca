"""Regularisation paths:  min_x f(A x) + mu * Omega(x)  over a decreasing sequence of mu, each solve warm-started from the one before and
stopped by its duality gap (stopping.DualityGap).  The operator is built -- a matrix uploaded -- once, and the step-size estimate is made once.

screen=True (least squares): gap-safe screening (certificates.screen; on the device fh_screen / fh_gather_columns, csrc/fh_screen.h).  Per mu, in
rounds: certify the warm start on the FULL problem; if the gap is not met, discard the features the certificate proves zero, solve over the kept
columns in a second, working operator down to max(gap_tolerance * f0, screen_shrink * gap), scatter the solution back with zeros, certify again.  A
round that would discard fewer than SCREEN_MIN_DISCARD of the features runs on the full operator (the copy costs a pass and buys less than one);
after screen_max_rounds rounds the point is finished there.  The certificate a point reports is always the full problem's.

standardize=True / intercept=True: the problem solved is the one on standardised columns (preprocess.standardize; on the device fh_standardize,
csrc/fh_standardize.h, once, right after the upload) and, with an intercept, on b - mean(b); every point keeps the solution, the certificate and the
gaps of THAT problem -- the one the certificate certifies -- and gains `.coefficients` and `.intercept` in the caller's units."""

import numpy as np

from . import certificates, stopping
from .linalg import is_sparse_matrix
from .proximal import GroupShrink, Shrink

__all__ = ["path", "mu_grid"]


def mu_grid(mu_max, n_mus=20, ratio=1e-3):
    """A geometric grid of n_mus values from mu_max down to ratio * mu_max."""
    if not mu_max > 0:
        raise ValueError(f"path: the critical mu is {mu_max!r}: A^H grad f(0) = 0, the solution is zero for every mu")
    if not 0 < ratio < 1 or int(n_mus) < 1:
        raise ValueError("path: needs 0 < ratio < 1 and n_mus >= 1")
    return mu_max * np.geomspace(1.0, ratio, int(n_mus))


def _unknown_shape(A, loss, x0):
    if x0 is not None:
        return np.shape(x0)
    V = getattr(A, "Vshape", None)
    if V is not None:
        return tuple(V)
    return (A.shape[1],) + tuple(loss.b.shape[1:])


def _check_arguments(prox_class, backend):
    if prox_class not in (Shrink, GroupShrink):
        raise TypeError(f"path: prox_class must be proximal.Shrink or proximal.GroupShrink (got {getattr(prox_class, '__name__', prox_class)!r})")
    if backend not in ("auto", "hip", "numpy"):
        raise ValueError('backend must be "auto", "hip" or "numpy"')


def _recognised(A, loss, prox_class, x, build=True):
    """(device map, loss tag, whether the map is the path's to close) of the path's operands, or TypeError with the front end's sentence.
    build=False: the sentence or nothing (the standardised path builds its own map, and meets a shape that does not fit later, as path() does)."""
    from .solver import _front_end, _unrecognised
    probe = prox_class(1.0)
    found = (_front_end if build else _unrecognised)(A, None, loss.f, loss.gradf, probe.g, probe.prox, x)
    if isinstance(found, str):
        raise TypeError("path(): " + found + ' (backend="numpy" runs the path on the host loop)')
    return found and (found[0], found[1], found[3])


SCREEN_MIN_DISCARD = 0.5      # a round compacts only if at least this share of the features goes: below it the copy costs more than it saves


def path(A, loss, prox_class, mus=None, n_mus=20, ratio=1e-3, x0=None, gap_tolerance=1e-6, backend="auto", every=10,
         screen=False, screen_shrink=0.1, screen_max_rounds=8, standardize=False, intercept=False, **options):
    """Solve the problem for every mu of `mus` (default: mu_grid from the critical mu, above which the solution is zero, down to ratio times it).
    A: what fasta() takes as its operator; loss: a tagged LeastSquares / LogisticLoss; prox_class: proximal.Shrink or proximal.GroupShrink.
    Returns one Convergence per mu (with `.mu`, `.certificate`, `.gaps`); each solve starts from the previous solution and stops at
    gap <= gap_tolerance * f(0).  On the device the critical mu is element 5 of fh_dual_gap at x0 = 0, the context is created once, and L / tau0
    of the first solve's estimate serve the later ones.  backend="numpy" runs the same thing on the host loop.  Other options go to the solver.
    screen=True: gap-safe screening as the module text says; each Convergence then also carries `.kept` (features of the last working set) and
    `.rounds`, `.solution` has full length and `.certificate` is the full problem's.  screen=False is the path without any of it.
    intercept=True (LeastSquares without weights, a dense matrix): the columns are centred and the solve uses LeastSquares(b - mean(b)), the mean per
    column of b.  standardize=True (a dense matrix; a sparse one: scaling only): the columns are scaled to unit root-mean-square, about the mean with
    intercept=True.  A is then an ndarray or a scipy.sparse matrix -- the path uploads it and rewrites its own copy.  `.solution`, `.certificate` and
    `.gaps` are those of the standardised problem; each Convergence gains `.coefficients` and `.intercept` (a float, or L floats) in the caller's
    units, and the first one carries `.standardization` (preprocess.Standardization).  With both False nothing of this runs."""
    if standardize or intercept:
        return _standardized_path(A, loss, prox_class, bool(standardize), bool(intercept), x0, backend,
                                  dict(mus=mus, n_mus=n_mus, ratio=ratio, gap_tolerance=gap_tolerance, every=every, screen=screen,
                                       screen_shrink=screen_shrink, screen_max_rounds=screen_max_rounds, **options))
    _check_arguments(prox_class, backend)
    for name in ("stop_rule", "tolerance"):
        if name in options:
            raise TypeError(f"path: every solve is stopped by its duality gap (gap_tolerance); {name} does not apply")
    shape = _unknown_shape(A, loss, x0)
    x = np.zeros(shape) if x0 is None else np.array(x0, dtype=np.float64)
    options.setdefault("verbose", False)
    rule = stopping.DualityGap(gap_tolerance, every)
    if screen:
        from .losses import LeastSquares
        if type(getattr(loss, "__self__", loss)) is not LeastSquares:
            raise TypeError("path: screen=True is stated for losses.LeastSquares (the radius of the logistic loss has another constant)")
        if not 0 < screen_shrink < 1 or int(screen_max_rounds) < 0:
            raise ValueError("path: needs 0 < screen_shrink < 1 and screen_max_rounds >= 0")
    # the one warm-start loop: a side (host or device) solves a point, plainly or in screening rounds
    side = _HostSide(A, loss, prox_class, x, options, screen) if backend == "numpy" else _DeviceSide(A, loss, prox_class, x, options)
    try:
        if mus is None:
            mus = mu_grid(side.critical_mu(x.shape), n_mus, ratio)
        if screen:
            side.estimate(prox_class(float(mus[0])), x)
        out = []
        for mu in mus:
            reg = prox_class(float(mu))
            conv = _screened_point(side, reg, x, rule, float(screen_shrink), int(screen_max_rounds)) if screen else side.solve_full(reg, x, rule)
            conv.mu = float(mu)
            x = np.array(conv.solution, dtype=np.float64)
            out.append(conv)
        return out
    finally:
        side.close()


# ---- a point with gap-safe screening ----------------------------------------------------------------------------------------------------------
def _screened_point(side, reg, x, rule, shrink, max_rounds):
    from .solver import Convergence
    n = x.shape[0]
    parts, gaps, iters, rounds, kept = [], [], 0, 0, n
    while True:
        cert, keep = side.certify(reg, x, want_mask=lambda c: not rule.met(c) and rounds < max_rounds)
        gaps.append((iters, cert.gap))
        if rule.met(cert) or iters >= side.max_iters:
            break
        if keep is None:                                # the rounds are spent: finish on the full operator
            conv = side.solve_full(reg, x, rule)
        else:
            rounds += 1
            idx = np.flatnonzero(keep)
            target = stopping.DualityGap(max(rule.tolerance, shrink * cert.gap / cert.f0), rule.every)
            if idx.size == 0:                           # every feature is screened: the solution is zero
                x, kept = np.zeros_like(x), 0
                continue
            if n - idx.size < SCREEN_MIN_DISCARD * n:
                conv = side.solve_full(reg, x, target)
            else:
                kept = int(idx.size)
                conv = side.solve_kept(reg, idx, x[idx], target)
                full = np.zeros_like(x)
                full[idx] = conv.solution
                conv.solution = full
        x = np.array(conv.solution, dtype=np.float64)
        iters += conv.iteration_count
        parts.append(conv)
    cat = lambda name: np.concatenate([np.asarray(getattr(p, name))[:p.iteration_count] for p in parts]) if parts else np.zeros(0)
    conv = Convergence(cat("residuals"), cat("norm_residuals"), cat("stepsizes"), sum(p.backtracks for p in parts), cat("times"), iters, x)
    conv.certificate, conv.gaps, conv.kept, conv.rounds = cert, gaps, kept, rounds
    return conv


class _Side:
    """What the host and the device side of the path share: the options of every solve and the step-size estimate, made once."""

    def __init__(self, loss, prox_class, options):
        self.loss, self.prox_class, self.options = loss, prox_class, options
        self.L, self.tau0 = options.pop("L", None), options.pop("tau0", None)
        self.max_iters = options.get("max_iters", 1000)

    def estimate(self, reg, x):
        if not self.L or not self.tau0:
            solver = self._solver(self.op, reg, x, stopping.DualityGap(0.0, 1)).setup()
            self.L, self.tau0 = solver.L, solver.tau0

    def solve_full(self, reg, x, rule):
        """One solve on the full operator; the first one's L / tau0 serve the later ones."""
        solver = self._solver(self.op, reg, x, rule).setup()
        self.L, self.tau0 = solver.L, solver.tau0
        return solver.run()

    def close(self):
        pass


class _HostSide(_Side):
    """The host side: the generic host loop; with screening certificates.screen and column slices (only then must A give its columns)."""

    def __init__(self, A, loss, prox_class, x, options, screen):
        from .generic import host_map
        for name in ("fused", "device_iters", "driver"):
            options.pop(name, None)
        if screen:
            A = self.M = certificates._columns_of(A)
            self.norms2 = certificates.column_norms2(self.M)
        self.op = host_map(A, None, x)
        _Side.__init__(self, loss, prox_class, options)

    def critical_mu(self, shape):
        return certificates.critical_mu(self.op, self.loss, self.prox_class, shape)

    def _solver(self, op, reg, x, rule):
        from .generic import HostFBS
        return HostFBS(op, self.loss.f, self.loss.gradf, reg.g, reg.prox, x, L=self.L, tau0=self.tau0, stop_rule=rule, **self.options)

    def certify(self, reg, x, want_mask):
        sc = certificates.screen(self.M, self.loss, reg, x, norms2=self.norms2)
        return sc.certificate, (sc.keep if want_mask(sc.certificate) else None)

    def solve_kept(self, reg, idx, x, rule):
        from .generic import host_map
        return self._solver(host_map(self.M[:, idx], None, x), reg, x, rule).setup().run()


class _DeviceSide(_Side):
    """The device side: FBSolver on one context; with screening fh_init + fh_dual_gap + fh_screen on it, and the kept columns in a working context
    (device to device, fh_gather_columns, for a dense matrix; a host slice through the CSR setter for a sparse one).  One working operator per path."""

    def __init__(self, A, loss, prox_class, x, options):
        self.op, loss, self.owns = _recognised(A, loss, prox_class, x)
        self.work = None
        self.cols = x.shape[1] if x.ndim == 2 else None
        _Side.__init__(self, loss, prox_class, options)

    def _at(self, reg, x):
        from . import hip
        c = self.op.ctx
        self.loss.bind(c)
        c.set_prox(reg.kind, reg.mu, 0.0, 0.0)
        c.set_vector(hip.VEC_X0, x)
        c.init()
        return c

    def critical_mu(self, shape):
        return self._at(self.prox_class(1.0), np.zeros(shape)).dual_gap().dual_norm

    def _solver(self, op, reg, x, rule):
        from .solver import FBSolver
        return FBSolver(op, self.loss, reg, x, L=self.L, tau0=self.tau0, stop_rule=rule, **self.options)

    def certify(self, reg, x, want_mask):
        c = self._at(reg, x)
        cert = c.dual_gap()
        return cert, (c.screen()[0] if want_mask(cert) else None)

    def solve_kept(self, reg, idx, x, rule):
        from .linalg import DenseMatrixMap, SparseMatrixMap
        if isinstance(self.op, SparseMatrixMap):
            S = self.op.matrix[:, idx]
            if self.work is None:
                self.work = SparseMatrixMap(S, device=self.op.device, rhs=self.cols)
                self.work.ctx
            else:                                       # the same context takes the next slice through the CSR setter
                self.work.set_matrix(S)
        else:
            if self.work is None:
                self.work = DenseMatrixMap(_defer=True, device=self.op.device, storage=self.op.storage, rhs=self.cols)
            self.work.take_columns(self.op, idx)
        return self._solver(self.work, reg, x, rule).setup().run()

    def close(self):
        if self.work is not None:
            self.work.close()
        if self.owns:
            self.op.close()


# ---- the path on standardised features ----------------------------------------------------------------------------------------------------------
def _standardized_path(A, loss, prox_class, scale, center, x0, backend, keywords):
    """The refusals, the standardised operator (the device's own copy rewritten by fh_standardize, or preprocess.standardize on the host), the path
    on it through path() itself, then the way back to the caller's units."""
    from . import preprocess
    from .linalg import ShardedDenseMatrixMap, _DeviceMap
    from .losses import LeastSquares, LogisticLoss
    _check_arguments(prox_class, backend)
    tag = getattr(loss, "__self__", loss)
    if center and isinstance(tag, LogisticLoss):
        raise TypeError("path: intercept=True is served for losses.LeastSquares without weights on a dense matrix: the intercept of the logistic loss "
                        "has no closed form")
    if center and (type(tag) is not LeastSquares or tag.weights is not None):
        raise TypeError("path: intercept=True is served for losses.LeastSquares without weights on a dense matrix")
    if isinstance(A, ShardedDenseMatrixMap):
        raise TypeError("path: standardize / intercept are served for an ndarray (dense) or a scipy.sparse matrix (scaling only), not for a sharded map: "
                        "a row-sharded context holds row blocks, not columns")
    if isinstance(A, _DeviceMap):
        raise TypeError(f"path: standardize / intercept are served for an ndarray (dense) or a scipy.sparse matrix (scaling only): a {type(A).__name__} "
                        "owns its context, which is the caller's to rewrite -- call map.ctx.standardize() and map the coefficients back with "
                        "preprocess.Standardization")
    sparse = is_sparse_matrix(A)
    if not sparse and not isinstance(A, np.ndarray):
        raise TypeError("path: standardize / intercept are served for an ndarray (dense) or a scipy.sparse matrix (scaling only): a general map cannot "
                        "give its columns")
    if sparse and center:
        raise TypeError("path: intercept=True is served for losses.LeastSquares without weights on a dense matrix: " + preprocess.SPARSE_CENTER_REFUSAL
                        + " (standardize=True alone is served)")
    b_mean = 0.0 if tag.b.ndim == 1 else np.zeros(tag.b.shape[1])
    if center:
        b_mean = tag.b.mean(axis=0)
        b_mean = float(b_mean) if tag.b.ndim == 1 else b_mean
        loss = LeastSquares(tag.b - b_mean)
    if backend == "numpy":
        A_std, st = preprocess.standardize(A, center=center, scale=scale)
        out = path(A_std, loss, prox_class, x0=x0, backend=backend, **keywords)
    else:
        from .linalg import DenseMatrixMap, SparseMatrixMap
        shape = _unknown_shape(A, loss, x0)
        _recognised(A, loss, prox_class, np.zeros(shape), build=False)
        op = SparseMatrixMap(A) if sparse else DenseMatrixMap(A, rhs=shape[1] if len(shape) == 2 else None)
        try:
            st = preprocess.Standardization(*op.standardize(center=center, scale=scale), op.shape[0])
            out = path(op, loss, prox_class, x0=x0, backend=backend, **keywords)
        finally:
            op.close()
    for conv in out:
        conv.coefficients = st.coefficients(conv.solution)
        conv.intercept = st.intercept(conv.solution, b_mean)
    if out:
        out[0].standardization = st
    return out
