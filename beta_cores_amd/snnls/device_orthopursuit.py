from .orthopursuit import OrthoPursuit
from .snnls import register_hooks


class DeviceOrthoPursuit(OrthoPursuit):
    """OrthoPursuit with the NNLS refit on the device (include/beta_cores_nnls.h).

    Same constructor, selection and protocol as OrthoPursuit; what differs is `_reweight`: the refit of
    orthopursuit.py:37-41 is solved by the library (Lawson-Hanson on the Gram matrix of the cached columns, one thread
    block, warm-started) instead of SciPy on the host, so `build()` runs the whole guarded loop on the device like GIGA
    and FrankWolfe, and `optimize()` stays there too.  The weights are the NNLS minimiser -- SciPy's support, its values
    to rounding, not its bits.  Single rank, at most 128 list entries: a `comm` of world > 1 and a build that could
    outgrow the list raise ValueError (sharded or larger problems: OrthoPursuit)."""
    _alg = 'omp_dev'
    _fusable = True

    def __init__(self, A, b, check_error_monotone=True, comm=None, **kw):
        if comm is not None and comm.world > 1:
            raise ValueError('DeviceOrthoPursuit serves single-rank solvers (comm.world = %d): sharded solvers keep the '
                             'host refit, use OrthoPursuit' % comm.world)
        super().__init__(A, b, check_error_monotone=check_error_monotone, comm=comm, **kw)
        self._eng.enable_device_refit()

    def _reweight(self, f):
        self._eng.refit(f)

    def optimize(self, device=True):
        super().optimize(device=device)


register_hooks('omp_dev', DeviceOrthoPursuit)
