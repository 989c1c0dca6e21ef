"""Worker for the two-rank full-data Laplace test (tests/test_gpu_laplace.py): one process per rank, gloo between them, the
rows sharded over the ranks on one GPU.  argv: out_prefix.  RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT from the environment."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shard_problem(n=40_000, d=9, seed=31):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, d)
    y = np.where(rng.rand(n) < 1. / (1. + np.exp(-X.dot(rng.randn(d)))), 1., -1.)
    w = rng.rand(n) * 3.
    w[rng.rand(n) < 0.2] = 0.
    return y[:, None] * X, w


def main():
    out = sys.argv[1]
    import torch.distributed as dist
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import beta_cores_amd as bc
    comm = bc.ShardComm()
    Z, w = shard_problem()
    bounds = bc.shard_bounds(Z.shape[0], world)
    lo, hi = bounds[rank], bounds[rank + 1]
    dz = bc.DeviceData(Z[lo:hi].copy(), row_offset=lo)
    res = {}
    for solver in ('newton', 'bfgs'):
        mu, LSig, LSigInv = bc.samplers.logistic_laplace(w[lo:hi], dz, np.zeros(Z.shape[1]), solver=solver, comm=comm)
        res[solver + '_mu'], res[solver + '_LSigInv'] = mu, LSigInv
    np.savez(out + '.rank%d.npz' % rank, **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
