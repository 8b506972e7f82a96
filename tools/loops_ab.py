#!/usr/bin/env python3
"""Cost of the Wilson-loop table (fthmc_wilson_loops, csrc/loops.hip) next to the trajectory that produces a configuration.

    python tools/loops_ab.py [--min-ms 1000] [--parent-tree DIR [--bench-steps 100] [--bench-rounds 2]] [--out FILE]

With HIP events around repeated calls (at least --min-ms of them per setting, after a warm-up):
  * one fthmc_wilson_loops call at the headline shape (128 chains, L = 64) for the 8 x 8 and the 32 x 32 table, and at
    config 2 (32 chains, L = 16) for 8 x 8 and 16 x 16, each with the batch mean;
  * one headline ftHMC trajectory (8 layers, beta = 6, tau = 1 in 10 leapfrog steps, two chain groups, carried state) for scale;
  * the achieved fp64 rate of the table against the VALU-FMA peak of DESIGN 4 (68 TFLOP/s): the walk's 6 FMAs per loop
    (12 FLOP) and the ~90 FLOP of the two sincos per site and extent R.
--parent-tree DIR: a built checkout of the parent commit; `bench.py --gpus 1` of DIR and of this tree run alternately (child
processes, --bench-rounds of each), their result lines side by side: nothing on the timed path changed, they must agree.
Prints one JSON document (also to --out)."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SEED = 1331
VALU_PEAK_TFLOPS = 68.0
SINCOS_FLOP = 45.0           # common.h ft_sincos: ~35 DP operations, 10 of them FMAs


def timed(fn, min_ms, warm=3):
    """mean ms of fn() on the device's clock: blocks of calls between two events until min_ms of them have run"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    n = max(5, int(math.ceil(min_ms / max(e0.elapsed_time(e1), 1e-3) / 5)))
    blocks = []
    for _ in range(5):
        e0.record()
        for _ in range(n):
            fn()
        e1.record(); e1.synchronize()
        blocks.append(e0.elapsed_time(e1) / n)
    return sum(blocks) / len(blocks), blocks, 5 * n


def loops_rows(ops, dev, min_ms):
    rows = []
    for name, B, L, tables in (('headline', 128, 64, ((8, 8), (32, 32))), ('config 2', 32, 16, ((8, 8), (16, 16)))):
        gen = torch.Generator().manual_seed(SEED)
        x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).to(dev)
        for Rmax, Tmax in tables:
            W = torch.empty(B, Rmax, Tmax, dtype=torch.float64, device=dev)
            mean = torch.empty(Rmax, Tmax, dtype=torch.float64, device=dev)
            ms, blocks, calls = timed(lambda: ops.wilson_loops(x, Rmax, Tmax, out=W, mean_out=mean), min_ms)
            loops = B * Rmax * Tmax * L * L
            flop = 12.0 * loops + 2 * SINCOS_FLOP * B * Rmax * L * L
            rows.append(dict(shape=name, B=B, L=L, Rmax=Rmax, Tmax=Tmax, ms_per_call=ms, ms_blocks=[round(b, 5) for b in blocks], calls=calls,
                             loops=loops, ns_per_kiloloop=ms * 1e6 / loops * 1e3, fp64_tflops=flop / (ms * 1e-3) * 1e-12,
                             fraction_of_valu_peak=flop / (ms * 1e-3) * 1e-12 / VALU_PEAK_TFLOPS,
                             lds_read_GBps=loops * 32.0 / (ms * 1e-3) * 1e-9))
    return rows


def trajectory_row(ops, parallel, dev, min_ms):
    from integrator_ab import CONFIGS, prepare
    cfg = CONFIGS[3]
    L, B, beta, nl = cfg['L'], cfg['B'], cfg['beta'], cfg['n_layers']
    w, x0 = prepare(ops, parallel, cfg, dev, 60)
    G = ops.default_groups(B, L)
    wkey = ('loops_ab', time.time_ns())
    seeds = torch.empty(B, dtype=torch.int64, device=dev)
    v, u = torch.empty_like(x0), torch.empty(B, dtype=torch.float64, device=dev)
    s = dict(x=x0, state=None, traj=0)

    def one():
        ops.chain_seeds(SEED + 11, 0, B, traj=s['traj'], out=seeds)
        ops.random_momenta(seeds, (B, 2, L, L), out_v=v, out_u=u)
        r = ops.ft_trajectory(s['x'], v, u, w, nl, beta, 0.1, 10, state_in=s['state'], groups=G, wkey=wkey)
        s['x'], s['state'], s['traj'] = r['x_new'], r['state'], s['traj'] + 1
    ms, blocks, calls = timed(one, min_ms)
    return dict(workload='headline ftHMC trajectory (eager launches, momentum refresh included)', B=B, L=L, n_layers=nl, beta=beta, nstep=10,
                groups=G, ms_per_trajectory=ms, ms_blocks=[round(b, 4) for b in blocks], trajectories=calls)


def bench_ab(parent, steps, warmup, rounds):
    def run(tree):
        r = subprocess.run([sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup),
                            '--no-cpu-baseline'], cwd=tree, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f'bench.py of {tree} failed ({r.returncode}): {r.stderr[-2000:]}')
        line = [t for t in r.stdout.strip().splitlines() if t.startswith('{')][-1]
        return json.loads(line)
    out = {'parent': [], 'this': []}
    for _ in range(rounds):
        for name, tree in (('parent', parent), ('this', ROOT)):
            d = run(tree)
            out[name].append({k: d.get(k) for k in ('metric', 'value', 'unit', 'ms_per_trajectory', 'trajectories_per_second') if k in d})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--min-ms', type=float, default=1000.0, help='timed work per setting, at least')
    ap.add_argument('--parent-tree', default=None, help='a built checkout of the parent commit (bench.py A/B)')
    ap.add_argument('--bench-steps', type=int, default=100)
    ap.add_argument('--bench-warmup', type=int, default=10)
    ap.add_argument('--bench-rounds', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    doc = dict(tool='tools/loops_ab.py')
    if args.parent_tree:                                                # first, in child processes: this one has not opened the GPU yet
        doc['bench'] = bench_ab(os.path.abspath(args.parent_tree), args.bench_steps, args.bench_warmup, args.bench_rounds)
    from fthmc_amd import _lib, ops, parallel
    assert torch.cuda.is_available(), 'needs the GPU'
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    doc.update(library=_lib.load().fthmc_version().decode(), device=torch.cuda.get_device_name(0), valu_peak_tflops=VALU_PEAK_TFLOPS,
               loops=loops_rows(ops, dev, args.min_ms), trajectory=trajectory_row(ops, parallel, dev, args.min_ms))
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
