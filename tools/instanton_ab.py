#!/usr/bin/env python3
"""Cost and effect of the instanton hit (fthmc_instanton_hit, csrc/topo.hip).

    python tools/instanton_ab.py [--min-ms 1000] [--parent-tree DIR [--bench-steps 100] [--bench-rounds 2]] [--ntraj 400] [--out FILE]

With HIP events around repeated calls (at least --min-ms of them per setting, after a warm-up, five blocks), at the headline batch
(128 chains, L = 64) and at config 2 (32 chains, L = 16), on fields thermalised by heatbath sweeps at beta = 2 and 6:
  * one call with n_hit = 1 and with n_hit = 8, in place, one workgroup per chain and the split form;
  * the hit acceptance and the mean |k| of an n_hit = 8 call, over 64 calls with fresh draws on the thermalised field;
  * the yardstick: one reduction pass and one elementwise pass over the same batch -- wilson_action_charge and regularize -- timed in
    blocks that ALTERNATE with blocks of the hit (n_hit = 1, in place, one workgroup per chain), both into preallocated outputs.
    --parent-tree DIR: the two calls come from DIR/fthmc_amd/libfthmc_hip.so (the parent commit's library, loaded next to this
    one), otherwise from this library.
    pass = median(hit) <= median(action_charge) + median(regularize) + the spread (max - min) of their sum;
  * the mean |dQ| per trajectory of run_hmc at beta = 6, L = 16 (ONE chain: run_hmc's configuration; --ntraj trajectories from a
    cold start, tau = 1, 10 steps; every figure over the trajectories behind the first quarter) with and without instanton=2.
--parent-tree DIR also runs `bench.py --gpus 1` of DIR and of this tree alternately (child processes, --bench-rounds of each), their
result lines side by side: only a translation unit was added, they must agree.
Prints one JSON document (also to --out)."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import torch  # noqa: E402

from loops_ab import bench_ab, timed  # noqa: E402

SEED = 31415


def yardstick(ops, parent):
    """-> (action_charge(x, beta, S, Q, plaq), regularize(x, out), label): the parent library's entry points, or this one's"""
    if parent is None:
        from fthmc_amd import _lib
        from fthmc_amd.ops import _p, _stream, check

        def reg_own(x, out):
            check(_lib.load().fthmc_regularize(_p(x), _p(out), x.numel(), _stream(x)), 'fthmc_regularize')
        return (lambda x, beta, o: ops.wilson_action_charge(x, beta, out=o)), reg_own, 'this library'
    lib = ctypes.CDLL(os.path.join(parent, 'fthmc_amd', 'libfthmc_hip.so'))
    V, I, Dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.fthmc_wilson_action_charge.argtypes = [V, I, I, Dbl, V, V, V, V]
    lib.fthmc_regularize.argtypes = [V, V, ctypes.c_size_t, V]
    lib.fthmc_version.restype = ctypes.c_char_p

    def action(x, beta, o):
        s = torch.cuda.current_stream(x.device).cuda_stream
        assert lib.fthmc_wilson_action_charge(x.data_ptr(), x.shape[0], x.shape[2], beta, o['S'].data_ptr(), o['Q'].data_ptr(), o['plaq'].data_ptr(), s) == 0

    def reg(x, out):
        assert lib.fthmc_regularize(x.data_ptr(), out.data_ptr(), x.numel(), torch.cuda.current_stream(x.device).cuda_stream) == 0
    return action, reg, 'parent library ' + lib.fthmc_version().decode()


def blocks_of(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / n


def rows_for(ops, dev, name, B, L, beta, min_ms, action, reg):
    gen = torch.Generator().manual_seed(SEED)
    x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).to(dev)
    seeds = ops.chain_seeds(SEED, 0, B, 0, device=dev)
    ops.local_update(x, beta, seeds, n_hb=1, n_or=1, nsweep=200, out=x)               # thermalise
    rows = []
    for n_hit in (1, 8):
        for path, pname in ((1, 'one workgroup per chain'), (2, 'split')):
            y = x.clone()
            o = {'x': y, 'k': torch.empty(B, dtype=torch.int32, device=dev), 'nacc': torch.empty(B, dtype=torch.int32, device=dev)}
            ms, blocks, calls = timed(lambda: ops.instanton_hit(y, beta, seeds, n_hit=n_hit, path=path, out=o), min_ms)
            rows.append(dict(shape=name, B=B, L=L, beta=beta, kind=f'hit, n_hit = {n_hit}, in place', path=pname, ms_per_call=ms,
                             ms_min=min(blocks), ms_max=max(blocks), calls=calls, ns_per_link=ms * 1e6 / (B * 2 * L * L)))
    na, ka = 0.0, 0.0
    for t in range(64):
        _, k, nacc = ops.instanton_hit(x, beta, seeds, n_hit=8, hit0=8 * t)
        na += float(nacc.sum()); ka += float(k.abs().sum())
    rows.append(dict(shape=name, B=B, L=L, beta=beta, kind='acceptance of a hit (64 calls of n_hit = 8)', acceptance=na / (64 * 8 * B), mean_abs_k=ka / (64 * B)))
    # the yardstick, alternating
    y, out = x.clone(), torch.empty_like(x)
    o = {'x': y, 'k': torch.empty(B, dtype=torch.int32, device=dev), 'nacc': torch.empty(B, dtype=torch.int32, device=dev)}
    obs = {k: torch.empty(B, dtype=torch.float64, device=dev) for k in ('S', 'Q', 'plaq')}
    fns = dict(hit=lambda: ops.instanton_hit(y, beta, seeds, n_hit=1, path=1, out=o), action_charge=lambda: action(x, beta, obs),
               regularize=lambda: reg(x, out))
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    n = max(5, int(math.ceil(min_ms / 5 / max(blocks_of(fns['hit'], 5), 1e-3))))
    t = {k: [] for k in fns}
    for _ in range(5):
        for k, f in fns.items():
            t[k].append(blocks_of(f, n))
    med = {k: statistics.median(v) for k, v in t.items()}
    both = [a + b for a, b in zip(t['action_charge'], t['regularize'])]
    limit = med['action_charge'] + med['regularize'] + (max(both) - min(both))
    rows.append(dict(shape=name, B=B, L=L, beta=beta, kind='hit (n_hit = 1, in place) against action_charge + regularize, alternating blocks',
                     median_ms=med, blocks_ms={k: [round(b, 6) for b in v] for k, v in t.items()}, limit_ms=limit, calls_per_block=n,
                     passed=bool(med['hit'] <= limit)))
    return rows


def hmc_rows(ntraj):
    from fthmc_amd.config import Param
    from fthmc_amd.hmc import run_hmc
    rows = []
    for inst in (0, 2):
        param = Param(beta=6.0, L=16, tau=1.0, nstep=10, ntraj=ntraj, nrun=1, nprint=0)
        torch.manual_seed(SEED)
        _, h = run_hmc(param, instanton=inst)
        w = slice(ntraj // 4, None)                                         # one window for every figure; run_hmc runs ONE chain
        one = lambda v: float(torch.as_tensor(v).reshape(-1)[0])
        dq, q, acc = ([one(v) for v in h[0][key][w]] for key in ('dq', 'q', 'acc'))
        row = dict(kind=f'run_hmc(instanton={inst}), beta 6, L 16, one chain', trajectories=len(dq), mean_abs_dQ=sum(dq) / len(dq),
                   mean_Q2=sum(v * v for v in q) / len(q), hmc_acceptance=sum(acc) / len(acc))
        if inst:
            ia = [one(v) for v in h[0]['inst_acc'][w]]
            row['hit_acceptance'] = sum(ia) / len(ia)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--min-ms', type=float, default=1000.0, help='timed work per setting, at least')
    ap.add_argument('--parent-tree', default=None, help='a built checkout of the parent commit (yardstick calls, bench.py A/B)')
    ap.add_argument('--bench-steps', type=int, default=100)
    ap.add_argument('--bench-warmup', type=int, default=10)
    ap.add_argument('--bench-rounds', type=int, default=2)
    ap.add_argument('--ntraj', type=int, default=400)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    doc = dict(tool='tools/instanton_ab.py')
    parent = os.path.abspath(args.parent_tree) if args.parent_tree else None
    if parent and args.bench_rounds > 0:                                # first, in child processes: this one has not opened the GPU yet
        doc['bench'] = bench_ab(parent, args.bench_steps, args.bench_warmup, args.bench_rounds)
    from fthmc_amd import _lib, ops
    assert torch.cuda.is_available(), 'needs the GPU'
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    action, reg, label = yardstick(ops, parent)
    doc.update(library=_lib.load().fthmc_version().decode(), device=torch.cuda.get_device_name(0), yardstick=label, rows=[])
    for name, B, L in (('headline', 128, 64), ('config 2', 32, 16)):
        for beta in (2.0, 6.0):
            doc['rows'] += rows_for(ops, dev, name, B, L, beta, args.min_ms, action, reg)
    if args.ntraj > 0:
        doc['run_hmc'] = hmc_rows(args.ntraj)
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
