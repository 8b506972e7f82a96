"""Local-update sampler of 2D U(1): heatbath sweeps, optionally mixed with overrelaxation (beyond the reference, which updates by
molecular dynamics only: fthmc/hmc.py, fthmc/ft_hmc.py know leapfrog).

A heatbath sweep draws every link from its conditional von Mises distribution exactly -- no step size, acceptance 1; an
overrelaxation sweep reflects every link about its conditional mode and leaves the action unchanged (csrc/local.hip).
The sampler shares no kernel with the MD path (no force, no integrator, no Metropolis step), so it is an independent check of the
same exact numbers (utils.observables.exact_wilson_loop).  It does NOT cure topological freezing: a local update changes the
charge no faster than HMC does; that stays with the flow and the beta ladder (tempering.py) -- and, for the plain action, with the
instanton hit (csrc/topo.hip), which does: run_local(instanton=k) puts k hits behind every update."""
from __future__ import annotations

import time
from typing import Optional

import numpy as np
import torch

from .config import Param
from .graph_loop import GraphLoop, Row, batched_start, chain_history, instanton_arg, loops_arg, run_graph_default


def run_local(param: Param, x: Optional[torch.Tensor] = None, n_overrelax: int = 0, sweeps_per_traj: int = 1, loops=None,
              loops_every: int = 1, use_graph: Optional[bool] = None, instanton: int = 0):
    """`param.nrun` runs of `param.ntraj` updates each; one update ("trajectory") is `sweeps_per_traj` compound sweeps of one
    heatbath sweep followed by `n_overrelax` overrelaxation sweeps, at param.beta (param.tau / nstep are not used: there is no MD).
    x: the start of every run, [2, L, L] or a batch [B, 2, L, L] (default param.initializer()).
    -> (fields_arr, histories): fields_arr[n] is the last field of run n; histories[n] has run_hmc's keys except 'dH' -- 'traj',
    'dt', 'acc' (identically 1), 'plaq', 'q', 'dq', one entry per update, per chain -- and 'wloops' where loops = (Rmax, Tmax) is
    given (one batch-mean table per `loops_every`-th update, as run_hmc).
    The seeds of update t are ops.chain_seeds(param.seed, chain, t), formed on the device; the sequence of one update is captured
    once (graph_loop) and replayed (`use_graph`, default on; FTHMC_RUN_GRAPH=0 turns it off): the same bits either way.
    instanton = k (default 0: nothing changes): k instanton hits (ops.instanton_hit) behind the sweeps of every update, inside the
    captured sequence, under the update's seeds (hit0 = 0: the seeds are fresh per update; the hit's counter plane is its own).  The
    history gains 'inst_acc' (accepted / k per chain) and 'inst_dq' (the applied charge per chain)."""
    from . import ops
    n_overrelax, sweeps_per_traj, loops_every = int(n_overrelax), int(sweeps_per_traj), max(1, int(loops_every))
    instanton = instanton_arg(instanton, 'run_local')
    if n_overrelax < 0 or sweeps_per_traj < 1:
        raise ValueError(f'run_local: n_overrelax >= 0 and sweeps_per_traj >= 1 expected, got {n_overrelax}, {sweeps_per_traj}')
    loops = loops_arg(loops, param.L)
    use_graph = run_graph_default() if use_graph is None else use_graph
    x0 = batched_start(param, x)
    dev, B = x0.device, x0.shape[0]
    histories, fields_arr = {}, []
    for n in range(param.nrun):
        t0 = time.time()
        xs = x0.clone()
        seeds = torch.empty(B, dtype=torch.int64, device=dev)
        counter = torch.full((1,), n * param.ntraj, dtype=torch.int64, device=dev)      # update t of the whole experiment
        row = Row(dev, plaq=B, Q=B, wloops=loops, k=B if instanton else 0, nacc=B if instanton else 0)
        q0 = ops.wilson_action_charge(xs, param.beta)[1].cpu().numpy()
        if instanton:
            iout = {'x': xs, 'k': torch.empty(B, dtype=torch.int32, device=dev), 'nacc': torch.empty(B, dtype=torch.int32, device=dev)}

        def enqueue():
            ops.chain_seeds(param.seed, 0, B, 0, counter=counter, advance=True, out=seeds)
            ops.local_update(xs, param.beta, seeds, n_hb=1, n_or=n_overrelax, nsweep=sweeps_per_traj, out=xs)
            if instanton:
                ops.instanton_hit(xs, param.beta, seeds, n_hit=instanton, out=iout)
                row['k'].copy_(iout['k'])
                row['nacc'].copy_(iout['nacc'])
            ops.wilson_action_charge(xs, param.beta, out={'plaq': row['plaq'], 'Q': row['Q']})

        def measure():
            ops.wilson_loops(xs, loops[0], loops[1], mean_out=row['wloops'])
        loop = GraphLoop(enqueue, row.flat, use_graph=use_graph, extra=measure if loops is not None else None, extra_every=loops_every)
        for _ in range(param.ntraj):
            loop.step()
        c = row.split(loop.rows())
        loop.join()
        dt = (time.time() - t0) / max(1, param.ntraj)
        late = {'inst_acc': c['nacc'] / instanton, 'inst_dq': c['k'].astype(np.int32)} if instanton else None
        histories[n] = chain_history(n * param.ntraj + 1, dt, q0, {'acc': np.ones_like(c['plaq']), 'plaq': c['plaq'], 'q': c['Q']},
                                     wloops=c.get('wloops'), loops_every=loops_every, late=late)
        fields_arr.append(xs.clone())
    return fields_arr, histories
