"""Stop rules with the reference's names and signature `(i, resid, norm_resid, max_resid, tolerance)`
(reference surface: fasta/stopping.py:6-51).  Pure host scalars -- nothing here touches the device.
`DualityGap(tolerance, every)` is not one of them: it is a TAG the loops recognise (certificates.py)."""

__all__ = ["residual", "norm_residual", "ratio_residual", "hybrid_residual", "DualityGap"]


class DualityGap:
    """Stop once the duality gap of the iterate is at most tolerance * f(0), checked at the start and after every `every` iterations
    (certificates.duality_gap on the host loop, HipContext.dual_gap on the device).  A tag, not a callable: pass it as `stop_rule`; the
    `tolerance` option of fasta() is then unused.  The solution returned is the iterate the last certificate was evaluated at."""

    def __init__(self, tolerance, every=10):
        if not float(tolerance) >= 0:
            raise ValueError(f"DualityGap: tolerance must be >= 0 (got {tolerance!r})")
        if int(every) != every or int(every) < 1:
            raise ValueError(f"DualityGap: every must be a positive integer (got {every!r})")
        self.tolerance, self.every = float(tolerance), int(every)

    def met(self, certificate):
        return bool(certificate.gap <= self.tolerance * certificate.f0)

    def next_check(self, i, max_iters):
        """The iteration index of the first check after iteration i: the next multiple of `every`, or the end of the solve."""
        return min((i // self.every + 1) * self.every, max_iters)

    def __repr__(self):
        return f"DualityGap({self.tolerance!r}, every={self.every})"


def residual(i, resid, norm_resid, max_resid, tolerance):
    """Stop once the residual ||x1 - x0|| / tau is below tolerance (stopping.py:6-15)."""
    return resid < tolerance


def norm_residual(i, resid, norm_resid, max_resid, tolerance):
    """Stop once the normalised residual is below tolerance (stopping.py:18-27)."""
    return norm_resid < tolerance


def ratio_residual(i, resid, norm_resid, max_resid, tolerance):
    """Stop once residual / largest-residual-so-far is below tolerance (stopping.py:30-39)."""
    return resid / max_resid < tolerance


def hybrid_residual(i, resid, norm_resid, max_resid, tolerance):
    """The reference default: ratio rule OR normalised rule (stopping.py:42-51)."""
    return ratio_residual(i, resid, norm_resid, max_resid, tolerance) or \
        norm_residual(i, resid, norm_resid, max_resid, tolerance)
