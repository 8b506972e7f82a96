#!/usr/bin/env python3
"""Cost of the annealing ramp (fthmc_anneal, csrc/local.hip) next to the sweeps it is made of, and what a ramp buys.

    python tools/anneal_ab.py [--min-ms 1000] [--parent-tree DIR [--bench-steps 100] [--bench-rounds 2]] [--out FILE]

With HIP events around repeated calls (at least --min-ms of them per setting, after a warm-up), at config 2 (32 chains, L = 16) and at
the headline batch (128 chains, L = 64), one heatbath sweep per step, 256 steps per call:
  * a CONSTANT schedule (beta = 2 and 6, thermalised fields): the call runs exactly the sweeps of local_update(nsweep = 256) and the
    chain sum of cos P on top -- the time per step of the one-launch ramp (path 1) and of the sequenced one (path 2) against
    local_update of this tree and, with --parent-tree, of the PARENT's library (loaded beside this one, the same process, the same
    fields): what the reduction costs, and that the kernels local_update runs cost what they did;
  * the ramp itself, beta 0 -> 6 quadratic from uniform links, on both paths;
  * ESS / B, log Z and its error against the number of steps for both kinds of schedule at L = 16, 1024 chains.
--parent-tree DIR: a built checkout of the parent commit; besides the library above, `bench.py --gpus 1` of DIR and of this tree run
alternately (child processes, --bench-rounds of each), their result lines side by side: only code was added, they must agree.
Prints one JSON document (also to --out)."""
import argparse
import ctypes
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import torch  # noqa: E402

from loops_ab import bench_ab, timed  # noqa: E402

SEED = 2718
STEPS = 256
BETA1 = 6.0


def parent_library(tree):
    """the parent's libfthmc_hip.so beside this tree's, with the one entry point the comparison calls"""
    from fthmc_amd import _lib
    lib = ctypes.CDLL(os.path.join(tree, 'fthmc_amd', 'libfthmc_hip.so'))
    lib.fthmc_local_update.argtypes = _lib.SIGNATURES['fthmc_local_update']
    lib.fthmc_local_update.restype = ctypes.c_int
    lib.fthmc_version.restype = ctypes.c_char_p
    return lib


def cost_rows(ops, plib, dev, name, B, L, min_ms):
    from fthmc_amd.anneal import beta_schedule
    gen = torch.Generator().manual_seed(SEED)
    x0 = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).to(dev)
    seeds = ops.chain_seeds(SEED, 0, B, 0, device=dev)
    out = {'x': torch.empty_like(x0), 'work': torch.empty(B, dtype=torch.float64, device=dev)}
    rows = []

    def row(kind, beta, ms, blocks, calls, **kw):
        rows.append(dict(shape=name, B=B, L=L, beta=beta, kind=kind, us_per_step=ms / STEPS * 1e3, us_blocks=[round(b / STEPS * 1e3, 4) for b in blocks],
                         calls=calls, ns_per_link=ms / STEPS * 1e6 / (B * 2 * L * L), **kw))
    for beta in (2.0, 6.0):
        x = ops.local_update(x0, beta, seeds, n_hb=1, n_or=1, nsweep=200)            # thermalised
        bt = torch.full((STEPS + 1,), beta, dtype=torch.float64, device=dev)
        base = {}
        ms, blocks, calls = timed(lambda: ops.local_update(x, beta, seeds, n_hb=1, nsweep=STEPS, sweep0=200, out=out['x']), min_ms)
        row('local_update, one launch, this tree', beta, ms, blocks, calls); base['this'] = ms
        if plib is not None:
            st = torch.cuda.current_stream(dev).cuda_stream

            def parent_call():
                rc = plib.fthmc_local_update(x.data_ptr(), B, L, beta, None, seeds.data_ptr(), 1, 0, STEPS, 200, 15, out['x'].data_ptr(), st)
                assert rc == 0, rc
            ms, blocks, calls = timed(parent_call, min_ms)
            row('local_update, one launch, PARENT library', beta, ms, blocks, calls); base['parent'] = ms
            ref = out['x'].clone()
            ops.local_update(x, beta, seeds, n_hb=1, nsweep=STEPS, sweep0=200, out=out['x'])
            assert torch.equal(ref, out['x']), 'the parent library and this tree differ in local_update'
        for path in (1, 2):
            ms, blocks, calls = timed(lambda: ops.anneal(x, bt, seeds, n_hb=1, sweep0=200, path=path, out=out), min_ms)
            row(f'anneal, constant schedule, path {path}', beta, ms, blocks, calls,
                over_local_update={k: round(ms / v - 1.0, 4) for k, v in base.items()})
    bt = torch.from_numpy(beta_schedule(0.0, BETA1, STEPS)).to(dev)
    for path in (1, 2):
        ms, blocks, calls = timed(lambda: ops.anneal(x0, bt, seeds, n_hb=1, path=path, out=out), min_ms)
        row(f'anneal, ramp 0 -> {BETA1:g} quadratic, path {path}', None, ms, blocks, calls)
    return rows


def ess_rows(L=16, B=1024):
    from fthmc_amd.anneal import run_annealed
    from fthmc_amd.config import Param
    from fthmc_amd.utils import observables as O
    exact = O.exact_log_partition(BETA1, L)
    rows = []
    for kind in ('quadratic', 'linear'):
        for n_step in (64, 256, 1024, 2048, 4096):
            _, h = run_annealed(Param(beta=BETA1, L=L, ntraj=B, nrun=1, nprint=0, seed=SEED), n_step, kind=kind)
            h = h[0]
            rows.append(dict(L=L, B=B, beta=BETA1, kind=kind, n_step=n_step, ess_over_B=h['ess'] / B, logZ=h['logZ'], logZ_err=h['logZ_err'],
                             logZ_exact=exact, seconds=h['dt']))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--min-ms', type=float, default=1000.0, help='timed work per setting, at least')
    ap.add_argument('--parent-tree', default=None, help='a built checkout of the parent commit (its library, and bench.py A/B)')
    ap.add_argument('--bench-steps', type=int, default=100)
    ap.add_argument('--bench-warmup', type=int, default=10)
    ap.add_argument('--bench-rounds', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    doc = dict(tool='tools/anneal_ab.py')
    if args.parent_tree and args.bench_rounds > 0:                      # first, in child processes: this one has not opened the GPU yet
        doc['bench'] = bench_ab(os.path.abspath(args.parent_tree), args.bench_steps, args.bench_warmup, args.bench_rounds)
    from fthmc_amd import _lib, ops
    assert torch.cuda.is_available(), 'needs the GPU'
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    plib = parent_library(os.path.abspath(args.parent_tree)) if args.parent_tree else None
    doc.update(library=_lib.load().fthmc_version().decode(), parent_library=plib.fthmc_version().decode() if plib else None,
               device=torch.cuda.get_device_name(0), steps_per_call=STEPS, rows=[])
    for name, B, L in (('config 2', 32, 16), ('headline', 128, 64)):
        doc['rows'] += cost_rows(ops, plib, dev, name, B, L, args.min_ms)
    doc['ess'] = ess_rows()
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
