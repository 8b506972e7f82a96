#!/usr/bin/env python3
"""A/B of the MD integrators (leapfrog, Omelyan 2MN, force-gradient) at matched force budgets on the bench workloads.

    python tools/integrator_ab.py [--config 3] [--config 2] [--budgets 10,20,40] [--rounds 5] [--out FILE]

For bench.py's config 3 (BASELINE.json configs[2]: L = 64, 128 chains, 8 layers, beta = 6, tau = 1, two chain groups) and config 2
(L = 16, 32 chains, 4 layers, beta = 4, tau = 1): seeded inputs prepared as bench.py prepares them (near-cold start, plain-HMC
thermalization, untrained flow), then for every (integrator, nstep) setting a chain of its own from that start, advanced in
`rounds` alternating blocks -- every round runs every setting once, so drift of the device's clocks falls on all of them alike.
A setting gets at least 1 s of timed work and at least 50 trajectories in all.  Per setting:
    ms per trajectory (device events around each block; momentum refresh and the running sums included, alike for all), ms per force evaluation,
    mean acceptance and <|dH|> over the setting's trajectories and chains,
    the ratio of its ms per force evaluation to the leapfrog's at the same budget,
and for the force-gradient settings the cost of the shift launch, derived: (ms per force - leapfrog's ms per force) x forces /
nstep (one shift launch per step; a direct timing would need an entry point of its own).
Prints one JSON document (also to --out)."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SEED = 1331
CONFIGS = {2: dict(L=16, beta=4.0, n_layers=4, B=32), 3: dict(L=64, beta=6.0, n_layers=8, B=128)}
TAU = 1.0


def nstep_for(name, budget):
    """the nstep whose force count is closest to (not above, where possible) the budget"""
    if name == 'leapfrog':
        return budget
    if name == 'omelyan':
        return max(1, budget // 2)
    return max(1, (budget - 1) // 3)


def make_flow(gen, n_layers):
    """bench.py's synthetic flow: PyTorch's default Conv2d init for the s/t net 2 -> 8 -> 8 -> 3, k = 3, drawn from `gen`"""
    sizes, flow = [2, 8, 8, 3], []
    for _ in range(n_layers):
        w = []
        for ci, co in zip(sizes[:-1], sizes[1:]):
            bound = 1.0 / math.sqrt(ci * 9)
            w.append((torch.rand(co, ci, 3, 3, generator=gen, dtype=torch.float64) * 2 - 1) * bound)
            w.append((torch.rand(co, generator=gen, dtype=torch.float64) * 2 - 1) * bound)
        flow.append(tuple(w))
    return flow


def prepare(ops, parallel, cfg, dev, thermalize):
    L, B, beta = cfg['L'], cfg['B'], cfg['beta']
    gen = torch.Generator(device='cpu').manual_seed(SEED)
    flow = make_flow(gen, cfg['n_layers'])
    w = ops.pack_weights(flow, device=dev)
    g0, _ = ops.random_momenta(parallel.chain_seeds(SEED + 1, 0, B, 0).to(dev), (B, 2, L, L), need_u=False)
    x = (0.1 * torch.erf(g0 / math.sqrt(2.0))).contiguous()
    for it in range(thermalize):
        vt, ut = ops.random_momenta(parallel.chain_seeds(SEED + 7, 0, B, it).to(dev), (B, 2, L, L))
        x = ops.hmc_trajectory(x, vt, ut, beta, 0.05, 20)['x_new']
    return w, x


def run_config(ci, args, ops, parallel, dev):
    cfg = CONFIGS[ci]
    L, B, beta, nl = cfg['L'], cfg['B'], cfg['beta'], cfg['n_layers']
    w, x0 = prepare(ops, parallel, cfg, dev, args.thermalize)
    G = ops.default_groups(B, L)
    wkey = ('integrator_ab', ci, time.time_ns())
    settings = []
    for budget in args.budgets:
        for name in ('leapfrog', 'omelyan', 'force_gradient'):
            nstep = nstep_for(name, budget)
            settings.append(dict(integrator=name, budget=budget, nstep=nstep, forces=ops.integrator_forces(name, nstep),
                                 x=x0.clone(), state=None, traj=0, ms=0.0, acc=0.0, adh=0.0, blocks=[]))
    seeds = torch.empty(B, dtype=torch.int64, device=dev)
    v = torch.empty_like(x0)
    u = torch.empty(B, dtype=torch.float64, device=dev)

    def block(s, n):
        """n chained trajectories of setting s -> ms on the device's clock"""
        acc = torch.zeros((), dtype=torch.float64, device=dev)
        adh = torch.zeros((), dtype=torch.float64, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            ops.chain_seeds(SEED + 11, 0, B, traj=s['traj'], out=seeds)
            ops.random_momenta(seeds, (B, 2, L, L), out_v=v, out_u=u)
            r = ops.ft_trajectory(s['x'], v, u, w, nl, beta, TAU / s['nstep'], s['nstep'], state_in=s['state'], groups=G, wkey=wkey,
                                  integrator=s['integrator'])
            s['x'], s['state'] = r['x_new'], r['state']
            s['traj'] += 1
            acc += r['acc'].mean(); adh += r['dH'].abs().mean()
        e1.record()
        e1.synchronize()
        s['acc'] += float(acc); s['adh'] += float(adh)
        return e0.elapsed_time(e1)

    # pilot: two trajectories per setting (untimed: allocations, the weight expansion), then two timed ones to size the blocks
    for s in settings:
        block(s, 2)
        t = block(s, 2) / 2
        s['per_round'] = max(1, math.ceil(max(args.min_traj, args.min_ms / t) / args.rounds))
        s['traj_counted'] = 0
        s['acc'] = s['adh'] = 0.0
    for _ in range(args.rounds):
        for s in settings:
            ms = block(s, s['per_round'])
            s['ms'] += ms; s['traj_counted'] += s['per_round']
            s['blocks'].append(round(ms / s['per_round'], 5))
    rows = []
    for s in settings:
        n = s['traj_counted']
        rows.append(dict(integrator=s['integrator'], budget=s['budget'], nstep=s['nstep'], forces=s['forces'], trajectories=n,
                         timed_ms=round(s['ms'], 2), ms_per_traj=s['ms'] / n, ms_per_force=s['ms'] / n / s['forces'],
                         ms_per_traj_blocks=s['blocks'], acceptance=s['acc'] / n, mean_abs_dH=s['adh'] / n))
    for r in rows:
        lf = next(q for q in rows if q['budget'] == r['budget'] and q['integrator'] == 'leapfrog')
        r['ms_per_force_vs_leapfrog'] = r['ms_per_force'] / lf['ms_per_force']
        if r['integrator'] == 'force_gradient':
            r['shift_launch_ms_derived'] = (r['ms_per_force'] - lf['ms_per_force']) * r['forces'] / r['nstep']
    return dict(config=ci, **cfg, tau=TAU, groups=G, rows=rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--config', type=int, action='append', choices=sorted(CONFIGS))
    ap.add_argument('--budgets', type=lambda t: [int(b) for b in t.split(',')], default=[10, 20, 40])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--min-ms', type=float, default=1000.0, help='timed work per setting, at least')
    ap.add_argument('--min-traj', type=int, default=50, help='trajectories per setting, at least')
    ap.add_argument('--thermalize', type=int, default=60)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from fthmc_amd import _lib, ops, parallel
    assert torch.cuda.is_available(), 'needs the GPU'
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    doc = dict(tool='tools/integrator_ab.py', library=_lib.load().fthmc_version().decode(), device=torch.cuda.get_device_name(0),
               budgets=args.budgets, rounds=args.rounds, results=[run_config(ci, args, ops, parallel, dev) for ci in (args.config or [3, 2])])
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
