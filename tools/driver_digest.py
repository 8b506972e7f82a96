#!/usr/bin/env python3
"""SHA-256 digests of what the sampler and training drivers return, through their public API only, so that the same file runs in a
checkout of another commit:  python3 tools/driver_digest.py > digest.json  there and here, then compare the two objects key by key.
One digest per history key (the per-trajectory entries stacked, as raw little-endian bytes with dtype and shape), per final field,
of the ft_run log's text and of the metadynamics table.  'dt' is a time and is left out; nothing else is.
The cases are the smallest that reach every branch of the drivers' host code (captured and eager, batch and single chain, a second
run from x_last, two chain groups, loops every third trajectory, instanton hits, two metadynamics phases, a tempering tail); behind
them the two trajectory sequences of csrc/api.hip through ops, on the branches the drivers do not reach (ops/...: B = 4, two table
rows of two chains; the sequenced plain path with a fresh x_new and with x itself; the flowed tuned, generic-net and no-layer branches
with and without a carried state; per-chain beta without layers)."""
import hashlib, json, os, sys, tempfile
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fthmc_amd import train as T
from fthmc_amd.config import Param, TrainConfig, lfConfig
from fthmc_amd.ft_hmc import FieldTransformation
from fthmc_amd.hmc import run_hmc
from fthmc_amd.local import run_local
from fthmc_amd import ops
from fthmc_amd.meta import MetaPotential, run_ft_meta, run_meta
from fthmc_amd.tempering import run_tempered
from fthmc_amd.utils import layers as LY
from fthmc_amd.utils import qed_helpers as qed
from oracle import ref_cpu as R

OUT = {}


def host(v):
    if torch.is_tensor(v):
        return v.detach().cpu().numpy()
    if isinstance(v, (list, tuple)):
        return np.stack([host(e) for e in v]) if len(v) else np.zeros(0)
    return np.asarray(v)


def put(key, v):
    a = np.ascontiguousarray(host(v))
    a = a.astype(a.dtype.newbyteorder('<'), copy=False)
    assert key not in OUT, key
    OUT[key] = hashlib.sha256(f'{a.dtype.str}{a.shape}'.encode() + a.tobytes()).hexdigest()


def put_history(name, h):
    for k in list(h.keys()):
        if k != 'dt':
            put(f'{name}/{k}', h[k])


def start(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.3 * (2 * torch.rand(B, 2, L, L, generator=g, dtype=torch.float64) - 1)).cuda()


def flow(L, beta, nl, B):
    cfg = TrainConfig(L=L, beta=beta, n_layers=nl, batch_size=B, print_freq=0)
    return cfg, T.get_model(cfg)


def ft_cases():
    for name, B, L, n, batch, loops in (('ft_batch', 4, 8, 7, True, (2, 3)), ('ft_single', 1, 8, 7, False, (2, 3)),
                                        ('ft_groups', 32, 64, 3, True, None)):
        for graph in (True, False):
            torch.manual_seed(101)
            cfg, model = flow(L, 3.0, 2, B)
            ft = FieldTransformation(flow=model.layers, config=cfg, lfconfig=lfConfig(tau=0.6, nstep=3))
            kw = dict(nprint=0, num_trajs=n, batch=batch, use_graph=graph, loops=loops, loops_every=3)
            tag = f'{name}/{"graph" if graph else "eager"}'
            put_history(f'{tag}/run1', ft.run(start(B, L, 5), **kw))
            put(f'{tag}/run1/x_last', ft.x_last)
            put_history(f'{tag}/run2', ft.run(ft.x_last, **kw))          # carries the state; the first history was read before
            put(f'{tag}/run2/x_last', ft.x_last)
            h3 = ft.run(ft.x_last, **kw)                                  # left unread: the next run reads it before the ring is reused
            h4 = ft.run(ft.x_last, **kw)
            put_history(f'{tag}/run3', h3)
            put_history(f'{tag}/run4', h4)
            put(f'{tag}/run4/x_last', ft.x_last)


def ft_run_case():
    for graph in (True, False):
        torch.manual_seed(102)
        cfg, model = flow(8, 3.0, 2, 1)
        par = Param(beta=3.0, L=8, tau=0.6, nstep=3, ntraj=3, nrun=2, seed=7)
        with tempfile.TemporaryDirectory() as d:
            log = os.path.join(d, 'ft_run.log')
            field, h = qed.ft_run(par, model.layers, start(1, 8, 6)[0], logfile=log, use_graph=graph, instanton=2)
            tag = f'ft_run/{"graph" if graph else "eager"}'
            put_history(tag, h)
            put(f'{tag}/field', field)
            put(f'{tag}/log', np.frombuffer(open(log, 'rb').read(), dtype=np.uint8))


def hmc_case():
    torch.manual_seed(103)
    par = Param(beta=3.0, L=8, tau=0.6, nstep=3, ntraj=4, nrun=2, seed=7, randinit=True, nprint=0)
    fields, hs = run_hmc(par, loops=2, overrelax=1, instanton=1)
    for n, h in hs.items():
        put_history(f'run_hmc/{n}', h)
        put(f'run_hmc/{n}/fields', fields[n])


def local_case():
    for graph in (True, False):
        torch.manual_seed(104)
        par = Param(beta=3.0, L=8, ntraj=7, nrun=2, seed=9)
        fields, hs = run_local(par, x=start(4, 8, 8), n_overrelax=2, loops=(3, 4), loops_every=3, instanton=2, use_graph=graph)
        for n, h in hs.items():
            put_history(f'run_local/{"graph" if graph else "eager"}/{n}', h)
            put(f'run_local/{"graph" if graph else "eager"}/{n}/field', fields[n])


def meta_case():
    for graph in (True, False):
        torch.manual_seed(105)
        pot = MetaPotential(41, 2.0, 10.0, groups=2)
        par = Param(beta=3.0, L=8, tau=0.6, nstep=3, ntraj=7, nrun=2, seed=5)
        fields, hs, pot = run_meta(par, x=start(6, 8, 9), potential=pot, n_build=9, w=0.05, integrator='omelyan', use_graph=graph)
        tag = f'run_meta/{"graph" if graph else "eager"}'
        for n, h in hs.items():
            put_history(f'{tag}/{n}', h)
            put(f'{tag}/{n}/field', fields[n])
        put(f'{tag}/table', pot.numpy())


def ft_meta_case():
    for small in (True, False):
        ops.set_small_path(small)
        try:
            for graph in (True, False):
                torch.manual_seed(108)
                _, model = flow(8, 3.0, 2, 6)
                pot = MetaPotential(41, 2.0, 10.0, groups=2)
                par = Param(beta=3.0, L=8, tau=0.6, nstep=3, ntraj=7, nrun=2, seed=5)
                fields, hs, pot = run_ft_meta(par, model.layers, x=start(6, 8, 10), potential=pot, n_build=9, w=0.05, integrator='omelyan',
                                              use_graph=graph)
                tag = f'run_ft_meta/{"small" if small else "tiled"}/{"graph" if graph else "eager"}'
                for n, h in hs.items():
                    put_history(f'{tag}/{n}', h)
                    put(f'{tag}/{n}/field', fields[n])
                put(f'{tag}/table', pot.numpy())
        finally:
            ops.set_small_path(True)


def ops_cases():
    B, G, beta, dt, nstep = 4, 2, 2.0, 0.1, 2
    g = torch.Generator().manual_seed(109)
    rough = torch.cumsum(6 * torch.rand(G, 41, generator=g, dtype=torch.float64) - 3, dim=1).cuda()
    tables = {'zero': (torch.zeros(G, 11, dtype=torch.float64).cuda(), 3.0, 0.0), 'rough': (rough, 2.0, 10.0)}

    def draw(L, amp):
        x = (amp * (2 * torch.rand(B, 2, L, L, generator=g, dtype=torch.float64) - 1)).cuda()
        return x, torch.randn(B, 2, L, L, generator=g, dtype=torch.float64).cuda(), torch.rand(B, generator=g, dtype=torch.float64).cuda()

    def put_all(tag, r):
        for k in sorted(r):
            put(f'{tag}/{k}', r[k])
    for integ in ('leapfrog', 'force_gradient'):
        x, v, u = draw(8, 1.5)
        for tk, tab in tables.items():
            put_all(f'ops/meta/{integ}/{tk}/fresh', ops.meta_trajectory(x, v, u, beta, dt, nstep, *tab, integrator=integ, path=2))
            xa = x.clone()
            put_all(f'ops/meta/{integ}/{tk}/alias', ops.meta_trajectory(xa, v, u, beta, dt, nstep, *tab, integrator=integ, path=2, out={'x_new': xa}))
        put_all(f'ops/hmc/{integ}/L128', ops.hmc_trajectory(*draw(128, 0.3), beta, dt, nstep, integrator=integ))
        bb = torch.tensor([1.5, 2.0, 2.5, 3.0], dtype=torch.float64).cuda()
        a = ops.ft_trajectory(x, v, u, None, 0, bb, dt, nstep, integrator=integ)
        put_all(f'ops/ft_pb_nolayers/{integ}/fresh', a)
        put_all(f'ops/ft_pb_nolayers/{integ}/carried', ops.ft_trajectory(a['x_new'].clone(), v, u, None, 0, bb, dt, nstep, integrator=integ,
                                                                         state_in=a['state'].clone()))
    ops.set_small_path(False)
    try:
        for name, L, nl, arch in (('tuned', 8, 2, None), ('tuned', 20, 2, None), ('generic', 8, 2, ((4, 6, 5), 5, 3)), ('nolayers', 8, 0, None)):
            wg = torch.Generator().manual_seed(110)
            kw = dict(hidden=arch[0], k=arch[1], n_mix=arch[2]) if arch else {}
            w = ops.pack_weights(R.default_flow(nl, wg, **kw), device='cuda') if nl else None
            for integ in ('leapfrog', 'force_gradient'):
                x, v, u = draw(L, 1.5)
                for tk, tab in tables.items():
                    a = ops.ft_meta_trajectory(x, v, u, w, nl, beta, dt, nstep, *tab, integrator=integ, arch=arch)
                    put_all(f'ops/ft_meta/{name}-L{L}/{integ}/{tk}/fresh', a)
                    put_all(f'ops/ft_meta/{name}-L{L}/{integ}/{tk}/carried',
                            ops.ft_meta_trajectory(a['x_new'].clone(), v, u, w, nl, beta, dt, nstep, *tab, integrator=integ, arch=arch,
                                                   state_in=a['state'].clone()))
                a = ops.ft_trajectory(x, v, u, w, nl, beta, dt, nstep, integrator=integ, arch=arch)
                put_all(f'ops/ft/{name}-L{L}/{integ}/fresh', a)
                put_all(f'ops/ft/{name}-L{L}/{integ}/carried', ops.ft_trajectory(a['x_new'].clone(), v, u, w, nl, beta, dt, nstep, integrator=integ,
                                                                                 arch=arch, state_in=a['state'].clone()))
    finally:
        ops.set_small_path(True)


def tempered_case():
    for captured in (True, False):
        torch.manual_seed(106)
        _, model = flow(8, 3.0, 2, 6)
        h = run_tempered(Param(L=8, tau=0.5, nstep=4, seed=143, randinit=True), model.layers, (1.0, 2.0, 3.0), 2, 7, swap_every=2,
                         captured=captured)
        put_history(f'run_tempered/{"captured" if captured else "eager"}', h)


def trainer_case():
    for graph in (True, False):
        torch.manual_seed(107)
        cfg, model = flow(8, 2.5, 2, 4)
        tr = T.GraphTrainer(model, cfg, T.make_optimizer(model, cfg), 4, seed=99, use_graph=graph, chunk=2)
        for _ in range(5):
            tr.step()
        tag = f'trainer/{"graph" if graph else "eager"}'
        put_history(tag, tr.history())
        put(f'{tag}/weights', LY.flow_weights(model.layers))


if __name__ == '__main__':
    for case in (ft_cases, ft_run_case, hmc_case, local_case, meta_case, ft_meta_case, tempered_case, trainer_case, ops_cases):
        case()
    torch.cuda.synchronize()
    print(json.dumps(OUT, sort_keys=True))
