"""Sparse non-negative least-squares solvers with the matrix resident on the GPU.

The public names are the ones `bayesiancoresets.snnls` exposes (its __init__ lists FrankWolfe,
ImportanceSampling, UniformSampling, GIGA and OrthoPursuit), plus the shared base class and
DeviceOrthoPursuit (OrthoPursuit with its NNLS refit on the device: the fused loop).
"""
from .snnls import SparseNNLS
from .giga import GIGA
from .frankwolfe import FrankWolfe
from .orthopursuit import OrthoPursuit
from .device_orthopursuit import DeviceOrthoPursuit
from .sampling import ImportanceSampling, UniformSampling

__all__ = ['SparseNNLS', 'GIGA', 'FrankWolfe', 'OrthoPursuit', 'DeviceOrthoPursuit', 'ImportanceSampling', 'UniformSampling']
