"""Regularisation paths:  min_x f(A x) + mu * Omega(x)  over a decreasing sequence of mu, each solve warm-started from the one before and
stopped by its duality gap (stopping.DualityGap).  The operator is built -- a matrix uploaded -- once, and the step-size estimate is made once."""

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


def path(A, loss, prox_class, mus=None, n_mus=20, ratio=1e-3, x0=None, gap_tolerance=1e-6, backend="auto", every=10, **options):
    """Solve the problem for every mu of `mus` (default: mu_grid from the critical mu, above which the solution is zero, down to ratio times it).
    A: what fasta() takes as its operator; loss: a tagged LeastSquares / LogisticLoss; prox_class: proximal.Shrink or proximal.GroupShrink.
    Returns one Convergence per mu (with `.mu`, `.certificate`, `.gaps`); each solve starts from the previous solution and stops at
    gap <= gap_tolerance * f(0).  On the device the critical mu is element 5 of fh_dual_gap at x0 = 0, the context is created once, and L / tau0
    of the first solve's estimate serve the later ones.  backend="numpy" runs the same thing on the host loop.  Other options go to the solver."""
    if prox_class not in (Shrink, GroupShrink):
        raise TypeError(f"path: prox_class must be proximal.Shrink or proximal.GroupShrink (got {getattr(prox_class, '__name__', prox_class)!r})")
    if backend not in ("auto", "hip", "numpy"):
        raise ValueError('backend must be "auto", "hip" or "numpy"')
    for name in ("stop_rule", "tolerance"):
        if name in options:
            raise TypeError(f"path: every solve is stopped by its duality gap (gap_tolerance); {name} does not apply")
    shape = _unknown_shape(A, loss, x0)
    x = np.zeros(shape) if x0 is None else np.array(x0, dtype=np.float64)
    options.setdefault("verbose", False)
    rule = stopping.DualityGap(gap_tolerance, every)
    if backend == "numpy":
        return _host_path(A, loss, prox_class, mus, n_mus, ratio, x, rule, options)
    return _device_path(A, loss, prox_class, mus, n_mus, ratio, x, rule, options)


def _host_path(A, loss, prox_class, mus, n_mus, ratio, x, rule, options):
    from .generic import HostFBS, host_map
    for name in ("fused", "device_iters", "driver"):
        options.pop(name, None)
    op = host_map(A, None, x)
    if mus is None:
        mus = mu_grid(certificates.critical_mu(op, loss, prox_class, x.shape), n_mus, ratio)
    out, L, tau0 = [], options.pop("L", None), options.pop("tau0", None)
    for mu in mus:
        reg = prox_class(float(mu))
        solver = HostFBS(op, loss.f, loss.gradf, reg.g, reg.prox, x, L=L, tau0=tau0, stop_rule=rule, **options).setup()
        L, tau0 = solver.L, solver.tau0
        conv = solver.run()
        conv.mu = float(mu)
        x = np.array(conv.solution, dtype=np.float64)
        out.append(conv)
    return out


def _device_path(A, loss, prox_class, mus, n_mus, ratio, x, rule, options):
    from . import hip
    from .solver import FBSolver, _recognise, _unrecognised
    probe = prox_class(1.0)
    why_not = _unrecognised(A, None, loss.f, loss.gradf, probe.g, probe.prox, x)
    if why_not is not None:
        raise TypeError("path(): " + why_not + ' (backend="numpy" runs the path on the host loop)')
    owns = isinstance(A, np.ndarray) or is_sparse_matrix(A)
    op, loss, _ = _recognise(A, None, loss.f, loss.gradf, probe.g, probe.prox, x)
    try:
        c = op.ctx
        if mus is None:                  # the critical mu from the device: x0 = 0, fh_init, element 5 of fh_dual_gap
            loss.bind(c)
            c.set_prox(probe.kind, 1.0, 0.0, 0.0)
            c.set_vector(hip.VEC_X0, np.zeros(x.shape))
            c.init()
            mus = mu_grid(c.dual_gap().dual_norm, n_mus, ratio)
        out, L, tau0 = [], options.pop("L", None), options.pop("tau0", None)
        for mu in mus:
            solver = FBSolver(op, loss, prox_class(float(mu)), x, L=L, tau0=tau0, stop_rule=rule, **options).setup()
            L, tau0 = solver.L, solver.tau0
            conv = solver.run()
            conv.mu = float(mu)
            x = np.array(conv.solution, dtype=np.float64)
            out.append(conv)
        return out
    finally:
        if owns:
            op.close()
