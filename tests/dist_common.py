"""Spawn / collect helpers of the multi-rank tests (tests/test_dist_gloo.py on the numpy stand-in,
tests/test_gpu_two_ranks.py on the real kernels; both over gloo).  The worker functions are at module top level,
which torch.multiprocessing.spawn needs."""
import os
import socket
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def join_group(rank, world, port):
    """What every spawned worker does first: the repository on sys.path, the rendezvous address, the gloo group."""
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _model_kw(gpu):
    if gpu:
        return dict(device="cuda:0")
    from tests.cpu_backend import NumpyBackend
    return dict(device="cpu", backend=NumpyBackend())


def _fit(g, **kw):
    from tests.common import model_for
    r, c, v = g.train
    model = model_for(g, **kw)
    model.fit_coo(r, c, v, (g.m, g.n), features=g.features or None, tol=g.cfg["tol"], min_iters=g.cfg["min_iters"],
                  verbose=0)
    return model


def fit_worker(rank, world, port, name, gs_mode, gpu, outdir):
    """One rank of a sharded fit of fixture `name` (gpu: the HIP backend on cuda:0, else the numpy stand-in); its
    factors and history go to outdir/rank<rank>.npz."""
    import torch.distributed as dist
    join_group(rank, world, port)
    try:
        from tests.common import Golden
        g = Golden(name)
        model = _fit(g, gs_mode=gs_mode, process_group="world", **_model_kw(gpu))
        if gpu:
            assert model._eng.world == world and model._eng.multi
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), U=model.U, V=model.V, b_u=model.b_u, b_i=model.b_i,
                 mu=model.mu, rmse=np.asarray(model.history["train_rmse"]),
                 **{"W_" + f: model.W[f] for f in g.cfg["feats"]})
    finally:
        dist.destroy_process_group()


def spawn(worker, world, *args):
    """Run worker(rank, world, port, *args, outdir) on `world` processes; every rank's rank<r>.npz as a dict."""
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(worker, args=(world, free_port(), *args, d), nprocs=world, join=True)
        return [dict(np.load(os.path.join(d, f"rank{r}.npz"))) for r in range(world)]


def sharded_fit(name, gs_mode=None, world=2, gpu=False):
    return spawn(fit_worker, world, name, gs_mode, gpu)


def single_fit(name, gpu=False):
    """(fixture, model) of the one-process fit the sharded ones are compared with."""
    from tests.common import Golden
    g = Golden(name)
    return g, _fit(g, **_model_kw(gpu))
