"""Annealed importance sampling of 2D U(1) (Neal 2001) with the Jarzynski work (Jarzynski 1997): beyond the reference, whose
samplers are Markov chains at the target beta.

A batch starts where the topological charge moves freely -- beta = 0, uniform links, or the samples of a trained flow -- and is
driven to the target beta through a ramp of heatbath (and overrelaxation) sweeps (ops.anneal, csrc/local.hip).  Every
chain carries the work W it took: it is an INDEPENDENT sample of the target with weight exp(-W), so nothing is autocorrelated
across topological sectors, and
    < exp(-W) > = Z(beta_1) / Z(beta_0)
is known exactly for this model (utils.observables.exact_log_partition): a check far sharper than < Q^2 >.  These are the
out-of-equilibrium evolutions of Caselle et al. (arXiv:2201.08862) and, started from a flow, the stochastic part of a stochastic
normalizing flow; Bonanno et al. (arXiv:2402.06561) use them against topological freezing.  Observables are reweighted with
utils.observables.reweighted_mean(values, -work)."""
from __future__ import annotations

import math
import time
from typing import Optional

import numpy as np
import torch

from .config import DTYPE, Param, device

KINDS = ('quadratic', 'linear')


def beta_schedule(beta0: float, beta1: float, n_step: int, kind: str = 'quadratic') -> np.ndarray:
    """beta_0 .. beta_n of a ramp beta0 -> beta1 in n_step steps, [n_step + 1] float64 with both ends exact:
        'linear'      beta_k = beta0 + (beta1 - beta0) k / n
        'quadratic'   beta_k = beta0 + (beta1 - beta0) (k / n)^2
    The work of a step is (beta_k - beta_{k+1}) sum cos P, whose variance is that of sum cos P: V / 2 at beta = 0, falling like
    1 / beta^2.  The quadratic ramp takes its small steps where that variance is large; from beta = 0 it is the default for that
    reason (L = 16, beta 0 -> 6: ESS / B = 0.5 with 2048 quadratic steps, 0.02 with 256 linear ones).  n_step = 0: the one entry
    beta0, which must be beta1."""
    beta0, beta1, n_step = float(beta0), float(beta1), int(n_step)
    if kind not in KINDS:
        raise ValueError(f'beta_schedule: kind in {KINDS} expected, got {kind!r}')
    if not (math.isfinite(beta0) and math.isfinite(beta1) and beta0 >= 0 and beta1 >= 0) or n_step < 0:
        raise ValueError(f'beta_schedule: finite betas >= 0 and n_step >= 0 expected, got {beta0}, {beta1}, {n_step}')
    if n_step == 0:
        if beta0 != beta1:
            raise ValueError(f'beta_schedule: no step leads from {beta0} to {beta1}')
        return np.array([beta0])
    t = np.arange(n_step + 1, dtype=np.float64) / n_step
    b = beta0 + (beta1 - beta0) * (t * t if kind == 'quadratic' else t)
    b[0], b[-1] = beta0, beta1
    return b


def run_annealed(param: Param, n_step: int, beta0: float = 0.0, kind: str = 'quadratic', x: Optional[torch.Tensor] = None, model=None,
                 n_overrelax: int = 0, sweeps_per_step: int = 1, steps_per_call: int = 256):
    """`param.nrun` independent annealed ensembles from beta0 to param.beta in `n_step` steps of beta_schedule(kind); a step is
    `sweeps_per_step` compound sweeps of one heatbath and `n_overrelax` overrelaxation sweeps at the step's new beta.
    The start of every chain must be a sample at beta0:
        x given        a batch [B, 2, L, L] drawn at beta0 by the caller (every run starts from it), work 0;
        model given    a flow (what FieldTransformation takes: a list of coupling layers): x = F(z) of uniform z drawn on the device,
                       with the work W_0 = -beta0 sum cos P(F(z)) - log det J(z) of a proposal of density 1 / det J in the measure
                       prod dx / 2 pi -- < exp(-W) > is then Z(param.beta) itself, whatever beta0, and the ESS at a given n_step
                       against the ESS without the flow is what the flow saves;
        neither        uniform links drawn on the device (ops.random_uniform): beta0 must be 0.
    Without x an ensemble has param.ntraj chains (a chain is one non-equilibrium trajectory).  The seeds of run n are
    ops.chain_seeds(param.seed, chain, n): one seed per chain for the draw of the start and every heatbath sweep of the ramp.
    The ramp is cut into calls of at most `steps_per_call` steps (the cut is bit-exact by fthmc_anneal's contract: no launch runs
    for seconds, whatever n_step).
    -> (fields_arr, histories): fields_arr[n] the final fields of run n; histories[n] = {'work', 'plaq', 'q': per chain (CPU
    tensors [B]); 'ess', 'logZ', 'logZ_err': numbers (utils.observables.work_ess, jarzynski_log_mean); 'betas'; 'dt': seconds}."""
    from . import ops
    from .utils import observables as O
    n_step, n_overrelax, sweeps_per_step, steps_per_call = int(n_step), int(n_overrelax), int(sweeps_per_step), int(steps_per_call)
    if n_step < 0 or n_overrelax < 0 or sweeps_per_step < 1 or steps_per_call < 1:
        raise ValueError(f'run_annealed: n_step, n_overrelax >= 0 and sweeps_per_step, steps_per_call >= 1 expected, got {n_step}, '
                         f'{n_overrelax}, {sweeps_per_step}, {steps_per_call}')
    if x is not None and model is not None:
        raise ValueError('run_annealed: a start x or a model, not both')
    if x is None and model is None and float(beta0) != 0.0:
        raise ValueError('run_annealed: uniform links are a sample at beta0 = 0 only; give x (drawn at beta0) or a model')
    betas = beta_schedule(beta0, param.beta, n_step, kind)
    dev = device()
    if x is not None:
        x0 = (x if x.dim() == 4 else x[None]).to(device=dev, dtype=DTYPE).contiguous()
        B = x0.shape[0]
    else:
        B = int(param.ntraj)
    L = param.L
    if model is not None:
        from .utils.layers import flow_weights
        nl = len(model)
        wflow = flow_weights(model, dev) if nl else None
    bt = torch.from_numpy(betas).to(dev)
    histories, fields_arr = {}, []
    for n in range(param.nrun):
        t0 = time.time()
        seeds = ops.chain_seeds(param.seed, 0, B, n, device=dev)
        work = torch.zeros(B, dtype=DTYPE, device=dev)
        if x is not None:
            xs = x0.clone()
        else:
            xs = ops.random_uniform(seeds, (B, 2, L, L), -math.pi, math.pi)
            if model is not None and nl:
                xs, logdet = ops.flow_forward(xs, wflow, nl)
                c0 = ops.anneal(xs, bt[:1], None, n_hb=0, n_or=1, trace=True)['trace'][:, 0]
                work = -(float(betas[0]) * c0) - logdet
        out = {'x': xs, 'work': work}
        for m in range(0, n_step, steps_per_call):
            k = min(steps_per_call, n_step - m)
            ops.anneal(xs, bt[m:m + k + 1], seeds, n_hb=1, n_or=n_overrelax, nsweep=sweeps_per_step, sweep0=m * sweeps_per_step,
                       work=work, out=out)
        _, Q, plaq = ops.wilson_action_charge(xs, param.beta)
        w = work.cpu()
        logz, logz_err = O.jarzynski_log_mean(w.numpy())
        histories[n] = {'work': w, 'plaq': plaq.cpu(), 'q': Q.cpu(), 'ess': O.work_ess(w.numpy()), 'logZ': logz, 'logZ_err': logz_err,
                        'betas': betas, 'dt': time.time() - t0}
        fields_arr.append(xs)
    return fields_arr, histories
