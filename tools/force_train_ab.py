#!/usr/bin/env python3
"""A/B of the force-norm training step: ops.train_force_grad with the fused dual kernels (csrc/flow_dual.hip) against the plain
dual sweep (csrc/flow_generic.hip), one process, one device.

Each setting of `ops.set_dual_path` is timed with HIP events over at least `--seconds` of back-to-back calls after a warm-up,
and the settings alternate `--rounds` times (>= 4), so drift of the device shows up as spread inside a setting rather than as a
difference between them.  `ops.ft_force` and `ops.train_grad` are timed at the same shapes for scale.  Prints one line per
(shape, setting, round) and a summary per shape; `--out FILE` keeps a copy.

    python tools/force_train_ab.py                       # config 2, config 3, the config-5 shard; generic / 8 x 8 / 8 x 16 / default
    python tools/force_train_ab.py --shapes config3 --paths 2,3 --seconds 0.3      # a short run, e.g. under a kernel trace
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {'config2': (16, 32, 4), 'config3': (64, 128, 8), 'config5_shard': (256, 32, 16)}     # L, B, layers
PATH_NAMES = {0: 'generic', 1: 'fused (default tile)', 2: 'fused 8x8', 3: 'fused 8x16'}


def timed(fn, seconds, min_calls=3):
    """ms per call: HIP events around batches of calls until `seconds` of device time have passed"""
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    one = max(e0.elapsed_time(e1), 1e-3)
    n = max(min_calls, int(seconds * 1e3 / one) + 1)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='config2,config3,config5_shard')
    ap.add_argument('--paths', default='0,2,3,1')
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from fthmc_amd import ops
    from oracle import ref_cpu as R
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    paths = [int(p) for p in args.paths.split(',')]
    say(f'# {ops._lib.load().fthmc_version().decode()}  device {torch.cuda.get_device_name(0)}')
    before = ops.get_dual_path()
    try:
        for tag in args.shapes.split(','):
            L, B, nl = SHAPES[tag]
            gen = torch.Generator().manual_seed(L + B + nl)
            w = ops.pack_weights(R.default_flow(nl, gen), device='cuda')
            x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * 3.14159).cuda()
            t_force, _ = timed(lambda: ops.ft_force(x, w, nl, 2.0), args.seconds / 4)
            t_kl, _ = timed(lambda: ops.train_grad(x, w, nl, 2.0), args.seconds / 4)
            say(f'{tag}: L={L} B={B} layers={nl}  ft_force {t_force:.4f} ms  train_grad {t_kl:.4f} ms')
            res = {p: [] for p in paths}
            wsb, served = {}, {}
            for rnd in range(args.rounds):
                for p in paths:
                    ops.set_dual_path(p)
                    wsb[p] = ops.train_force_ws_bytes(B, L, nl)
                    served[p] = ops.train_force_path(B, L)
                    ms, n = timed(lambda: ops.train_force_grad(x, w, nl, 2.0), args.seconds)
                    res[p].append(ms)
                    say(f'  {tag} round {rnd} {PATH_NAMES[p]:<20} {ms:10.4f} ms/call  ({n} calls, fused={served[p]}, ws {wsb[p] / 2**20:.1f} MiB)')
            summ = {}
            for p in paths:
                v = res[p]
                summ[PATH_NAMES[p]] = {'min': min(v), 'max': max(v), 'mean': sum(v) / len(v), 'spread': max(v) - min(v),
                                       'x_ft_force': sum(v) / len(v) / t_force, 'ws_bytes': wsb[p], 'fused': served[p]}
            if 0 in paths:
                g = summ['generic']
                for p in paths:
                    if p == 0:
                        continue
                    f = summ[PATH_NAMES[p]]
                    f['speedup_vs_generic'] = g['mean'] / f['mean']
                    f['every_fused_below_every_generic'] = f['max'] < g['min']
                    f['gap_over_larger_spread'] = (g['min'] - f['max']) / max(g['spread'], f['spread'], 1e-12)
            say(f'  {tag} summary ' + json.dumps({'ft_force_ms': t_force, 'train_grad_ms': t_kl, **summ}))
    finally:
        ops.set_dual_path(before)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    t0 = time.time()
    main()
    print(f'# wall {time.time() - t0:.1f} s', flush=True)
