"""fthmc/hmc.py::run_hmc on the HIP path (plain HMC experiment loop, no plots)."""
from __future__ import annotations

import os
import time

import numpy as np
import torch

from .config import DTYPE, Param
from .graph_loop import instanton_arg, loops_arg
from .utils import qed_helpers as qed


def run_hmc(param: Param, x: torch.Tensor = None, plot_metrics: bool = False, figsize=None, use_title: bool = True,
            save_data: bool = False, nplot: int = 10, integrator: str = 'leapfrog', loops=None, loops_every: int = 1,
            overrelax: int = 0, instanton: int = 0):
    """hmc.py:57-175: `param.nrun` experiments of `param.ntraj` trajectories each.
    Returns (fields_arr, histories) with the reference's metric keys.
    integrator: 'leapfrog' | 'omelyan' | 'force_gradient' (beyond the reference: csrc/integrator.h).
    loops = (Rmax, Tmax) (default None: nothing changes): after every `loops_every`-th trajectory of a run the Wilson loops of the
    field are measured (ops.wilson_loops) and the history gains 'wloops', one [Rmax, Tmax] batch-mean table per measured
    trajectory (utils.observables.exact_wilson_loop has the exact expectation).
    overrelax = k (default 0: nothing changes): k overrelaxation sweeps (qed_helpers.overrelax) behind every trajectory, before it is
    measured; they leave the action where the trajectory put it and move the non-topological modes.
    instanton = k (default 0: nothing changes): k instanton hits (qed_helpers.instanton_hit) behind every trajectory and behind the
    overrelaxation sweeps, before the measurement: Metropolis steps across topological sectors, which the molecular dynamics does
    not cross at large beta.  The history gains 'inst_acc' (accepted / k per chain) and 'inst_dq' (the applied charge per chain)."""
    from . import ops
    ops.integrator_code(integrator)                                      # an unknown name raises before anything runs
    loops = loops_arg(loops, param.L)
    loops_every = max(1, int(loops_every))
    overrelax = int(overrelax)
    if overrelax < 0:
        raise ValueError(f'overrelax: a number of sweeps >= 0 expected, got {overrelax}')
    instanton = instanton_arg(instanton)
    action = qed.BatchAction(param.beta)
    histories, fields_arr, run_times = {}, [], []
    for n in range(param.nrun):
        t0 = time.time()
        x = param.initializer()
        q = qed.batch_charges(x)
        xarr, history = [], {}
        for i in range(param.ntraj):
            t1 = time.time()
            dH, exp_mdH, acc, x = qed.hmc(param, x, verbose=False, integrator=integrator)
            if overrelax:
                x = qed.overrelax(param, x, overrelax)
            if instanton:
                x, inst_k, inst_na = qed.instanton_hit(param, x, instanton)
            qold = history['q'][-1] if 'q' in history else q
            qnew = qed.batch_charges(x)
            dq = torch.sqrt((qnew - qold) ** 2)
            plaq = (-1.) * action(x) / (param.beta * param.volume)
            xarr.append(x)
            metrics = {'traj': n * param.ntraj + i + 1, 'dt': time.time() - t1, 'acc': acc.to(DTYPE), 'dH': dH,
                       'plaq': plaq, 'q': qnew, 'dq': dq}
            if instanton:
                metrics.update(inst_acc=inst_na.to(DTYPE) / instanton, inst_dq=inst_k)
            for k, v in metrics.items():
                history.setdefault(k, []).append(v)
            if loops is not None and i % loops_every == 0:
                table = torch.empty(loops, dtype=DTYPE, device=x.device)
                ops.wilson_loops(x.reshape((-1,) + tuple(x.shape[-3:])), loops[0], loops[1], mean_out=table)
                history.setdefault('wloops', []).append(table)
            if param.nprint and (i - 1) % param.nprint == 0:
                print(f"run {n} traj {i}: acc={float(acc):.0f} dH={float(dH):.4g} plaq={float(plaq):.6f} "
                      f"q={float(qnew):.2f}", flush=True)
        run_times.append(time.time() - t0)
        histories[n] = history
        fields_arr.append(xarr)
    if save_data:
        os.makedirs(param.logdir, exist_ok=True)
        np.savez(os.path.join(param.logdir, 'hmc_histories.npz'),
                 **{f'run{n}_{k}': (np.stack([v.cpu().numpy() for v in vals]) if k == 'wloops' else
                                    np.array([float(torch.as_tensor(v).reshape(-1)[0]) for v in vals]))
                    for n, h in histories.items() for k, vals in h.items()})
    return fields_arr, histories
