#!/usr/bin/env python3
"""Cost of the local updates (fthmc_local_update, csrc/local.hip) next to the plain-HMC trajectory of the same batch.

    python tools/local_ab.py [--min-ms 1000] [--parent-tree DIR [--bench-steps 100] [--bench-rounds 2]] [--out FILE]

With HIP events around repeated calls (at least --min-ms of them per setting, after a warm-up), at the headline batch (128 chains,
L = 64) and at config 2 (32 chains, L = 16), on thermalised fields at beta = 2 and 6:
  * one overrelaxation sweep and one heatbath sweep, each as ONE call of 10 sweeps on the one-launch kernel (the chain in LDS) and
    on the class kernels (one launch per class), per sweep;
  * one plain-HMC trajectory (10 leapfrog steps, tau = 1) of the same batch, for scale;
  * the attempts of the rejection loop per link, mean and maximum, from the numpy twin of the tests on 4 chains of the field.
--parent-tree DIR: a built checkout of the parent commit; `bench.py --gpus 1` of DIR and of this tree run alternately (child
processes, --bench-rounds of each), their result lines side by side: only a translation unit was added, they must agree.
Prints one JSON document (also to --out)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402

from loops_ab import bench_ab, timed  # noqa: E402

SEED = 2718
NSWEEP = 10


def rows_for(ops, dev, name, B, L, beta, min_ms):
    import numpy as np
    import local_update_cases as LC
    gen = torch.Generator().manual_seed(SEED)
    x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).to(dev)
    seeds = ops.chain_seeds(SEED, 0, B, 0, device=dev)
    ops.local_update(x, beta, seeds, n_hb=1, n_or=1, nsweep=200, out=x)               # thermalise
    out, rows = torch.empty_like(x), []
    for kind, n_hb, n_or in (('overrelaxation', 0, 1), ('heatbath', 1, 0)):
        for resident in (True, False):
            ops.set_small_path(resident)
            ms, blocks, calls = timed(lambda: ops.local_update(x, beta, seeds, n_hb=n_hb, n_or=n_or, nsweep=NSWEEP, sweep0=200, out=out), min_ms)
            ops.set_small_path(True)
            rows.append(dict(shape=name, B=B, L=L, beta=beta, kind=kind, path='one launch' if resident else 'class kernels',
                             ms_per_sweep=ms / NSWEEP, ms_blocks=[round(b / NSWEEP, 6) for b in blocks], calls=calls,
                             ns_per_link=ms / NSWEEP * 1e6 / (B * 2 * L * L)))
    v, u = torch.randn_like(x), torch.rand(B, dtype=torch.float64, device=dev)
    res = {'x_new': torch.empty_like(x)}
    ms, blocks, calls = timed(lambda: ops.hmc_trajectory(x, v, u, beta, 0.1, 10, out=res), min_ms)
    rows.append(dict(shape=name, B=B, L=L, beta=beta, kind='plain-HMC trajectory, 10 leapfrog steps', ms_per_trajectory=ms,
                     ms_blocks=[round(b, 6) for b in blocks], calls=calls))
    xs = x[:4].cpu().numpy()
    sd = seeds[:4].cpu().numpy()
    att = np.concatenate([LC.class_update(xs, mu, p, 'hb', beta, sd, 200)['attempts'].ravel() for mu, p in LC.CLASSES])
    rows.append(dict(shape=name, B=B, L=L, beta=beta, kind='attempts per link (twin, 4 chains, one sweep)', mean=float(att.mean()), max=int(att.max()),
                     links=int(att.size)))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--min-ms', type=float, default=1000.0, help='timed work per setting, at least')
    ap.add_argument('--parent-tree', default=None, help='a built checkout of the parent commit (bench.py A/B)')
    ap.add_argument('--bench-steps', type=int, default=100)
    ap.add_argument('--bench-warmup', type=int, default=10)
    ap.add_argument('--bench-rounds', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    doc = dict(tool='tools/local_ab.py')
    if args.parent_tree:                                                # first, in child processes: this one has not opened the GPU yet
        doc['bench'] = bench_ab(os.path.abspath(args.parent_tree), args.bench_steps, args.bench_warmup, args.bench_rounds)
    from fthmc_amd import _lib, ops
    assert torch.cuda.is_available(), 'needs the GPU'
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    doc.update(library=_lib.load().fthmc_version().decode(), device=torch.cuda.get_device_name(0), sweeps_per_call=NSWEEP, rows=[])
    for name, B, L in (('headline', 128, 64), ('config 2', 32, 16)):
        for beta in (2.0, 6.0):
            doc['rows'] += rows_for(ops, dev, name, B, L, beta, args.min_ms)
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
