#!/usr/bin/env python3
"""Measurements of replica exchange over a beta ladder on the bench shapes.

    python tools/tempering_ab.py [--config 3] [--config 2] [--rounds 5] [--physics] [--out FILE]

For bench.py's config 3 (BASELINE.json configs[2]: L = 64, 128 chains, 8 layers, tau = 1, 10 steps, two chain groups) and config 2
(L = 16, 32 chains, 4 layers), seeded inputs (uniform links in +-0.3, the synthetic flow of bench.py's init):
  (b) the per-chain-beta trajectory (ops.ft_trajectory with a beta tensor holding ONE value) against the scalar one, same build,
      in `rounds` alternating blocks of `reps` calls each, device events around each block -> ms per trajectory, both, and the ratio;
  (c) the swap round alone (ops.replica_swap on the batch's ladders, both parities alternating) -> microseconds per round;
  (d) --physics, config-2 shape only: tempered ftHMC over a ladder up to the config's beta against untempered ftHMC at that beta
      with the same batch (all B chains cold, against B / K cold chains of the tempered run) and the same number of trajectories: dQ^2 of the cold rung per force evaluation
      (utils/observables.change_sqr, lag 1) and the round trips per ladder.  A physics record, no bar.
Prints one JSON document (also to --out)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SEED = 1331
CONFIGS = {2: dict(L=16, beta=4.0, n_layers=4, B=32, groups=1), 3: dict(L=64, beta=6.0, n_layers=8, B=128, groups=2)}
TAU, NSTEP = 1.0, 10


def make_flow(gen, n_layers):
    sizes, flow = [2, 8, 8, 3], []
    for _ in range(n_layers):
        w = []
        for ci, co in zip(sizes[:-1], sizes[1:]):
            bound = 1.0 / math.sqrt(ci * 9)
            w.append((torch.rand(co, ci, 3, 3, generator=gen, dtype=torch.float64) * 2 - 1) * bound)
            w.append((torch.rand(co, generator=gen, dtype=torch.float64) * 2 - 1) * bound)
        flow.append(tuple(w))
    return flow


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def ab(ops, cfg, rounds, reps):
    L, B, nl, beta, G = cfg['L'], cfg['B'], cfg['n_layers'], cfg['beta'], cfg['groups']
    gen = torch.Generator().manual_seed(SEED)
    flow = make_flow(gen, nl)
    w = ops.pack_weights(flow, device='cuda')
    x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * 0.3).cuda()
    v = torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64).cuda()
    u = torch.rand(B, generator=gen, dtype=torch.float64).cuda()
    bb = torch.full((B,), beta, dtype=torch.float64, device='cuda')
    dt = TAU / NSTEP
    calls = {'scalar': lambda: ops.ft_trajectory(x, v, u, w, nl, beta, dt, NSTEP, groups=G, wkey=1),
             'per_chain': lambda: ops.ft_trajectory(x, v, u, w, nl, bb, dt, NSTEP, groups=G, wkey=1)}
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            ms[k].append(timed(fn, reps))
    res = {k: {'ms_per_traj_blocks': t, 'ms_per_traj': float(np.median(t))} for k, t in ms.items()}
    res['per_chain_over_scalar'] = res['per_chain']['ms_per_traj'] / res['scalar']['ms_per_traj']
    # (c) the swap round alone
    K = 4
    lad = ops.ladder_init(np.linspace(beta / 2, beta, K), B // K, device='cuda')
    C = torch.randn(B, dtype=torch.float64, device='cuda')
    us = torch.rand(B // K, K - 1, dtype=torch.float64, device='cuda')
    o = {}
    par = [0]

    def swap():
        ops.replica_swap(lad['betas'], C, us, lad['beta_b'], lad['rung'], lad['chain_of'], par[0], out=o)
        par[0] ^= 1
    swap(); torch.cuda.synchronize()
    res['swap_round_us'] = [1e3 * timed(swap, 200) for _ in range(rounds)]
    return res


def physics(ops, cfg, ntraj, K):
    from fthmc_amd.config import Param
    from fthmc_amd.tempering import run_tempered
    from fthmc_amd.utils.observables import change_sqr
    L, nl, beta, B = cfg['L'], cfg['n_layers'], cfg['beta'], cfg['B']
    flow = make_flow(torch.Generator().manual_seed(SEED), nl)
    M = B // K
    betas = list(np.linspace(beta / 2, beta, K))
    p = Param(L=L, tau=TAU, nstep=NSTEP, seed=SEED, randinit=False)
    h = run_tempered(p, flow, betas, M, ntraj)
    cold = h['Q'][ntraj // 10:, K - 1, :]
    res = {'betas': betas, 'ladders': M, 'ntraj': ntraj,
           'tempered_cold_dQ2': change_sqr(cold, 1), 'swap_acc': h['swap_acc'].tolist(),
           'round_trips_per_ladder': float(h['round_trips'].sum()) / M, 'hmc_acc_per_rung': h['acc'].mean(axis=(0, 2)).tolist(),
           'force_evaluations_per_cold_trajectory_tempered': NSTEP * K}
    # untempered: the same number of chains, all at the cold beta, through the scalar entry point
    gen = torch.Generator().manual_seed(SEED)
    w = ops.pack_weights(flow, device='cuda')
    x = torch.zeros(B, 2, L, L, dtype=torch.float64, device='cuda')
    qs, st = [], None
    for t in range(ntraj):
        v = torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64).cuda()
        u = torch.rand(B, generator=gen, dtype=torch.float64).cuda()
        r = ops.ft_trajectory(x, v, u, w, nl, beta, TAU / NSTEP, NSTEP, state_in=st, wkey=1)
        x, st = r['x_new'], r['state']
        qs.append(r['Q'].cpu().numpy())
    q = np.stack(qs)[ntraj // 10:]
    res['untempered_dQ2'] = change_sqr(q, 1)
    res['force_evaluations_per_trajectory_untempered'] = NSTEP
    res['cold_dQ2_per_force_tempered'] = res['tempered_cold_dQ2'][0] / (NSTEP * K)
    res['dQ2_per_force_untempered'] = res['untempered_dQ2'][0] / NSTEP
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', type=int, action='append', choices=sorted(CONFIGS))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--physics', action='store_true')
    ap.add_argument('--ntraj', type=int, default=2000)
    ap.add_argument('--rungs', type=int, default=4)
    ap.add_argument('--out')
    args = ap.parse_args()
    from fthmc_amd import ops
    doc = {'device': torch.cuda.get_device_name(0), 'tau': TAU, 'nstep': NSTEP}
    for c in args.config or [3, 2]:
        doc[f'config{c}'] = ab(ops, CONFIGS[c], args.rounds, args.reps)
    if args.physics:
        doc['physics_config2'] = physics(ops, CONFIGS[2], args.ntraj, args.rungs)
    s = json.dumps(doc, indent=1)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(s + '\n')


if __name__ == '__main__':
    main()
