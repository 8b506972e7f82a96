#!/usr/bin/env python3
"""SHA-256 digests of what the one-launch plain trajectory kernels (csrc/traj_resident.h: wilson.hip k_hmc_trajectory and
k_hmc_trajectory_sched<PB>, meta.hip k_meta_trajectory) return, through ops only, so that the same file runs against another build
of the library:

    FTHMC_LIB=PARENT/fthmc_amd/libfthmc_hip.so python tools/resident_digest.py --out a.json
    python tools/resident_digest.py --out b.json
    python tools/resident_digest.py --compare a.json b.json --out profiles/resident_plan_digest.json

One digest per output (x_new, dH, acc, H0, H1, and qm, vbias of the biased calls), of its raw uint64 words.  Cases: B = 3 chains at
L = 4, 8, 36, 60, 64 (one partial wave, ragged passes over the owned sites, all slots full) with leapfrog, Omelyan and force-gradient,
scalar beta (leapfrog: k_hmc_trajectory, the others: the schedule kernel) and per-chain beta (the schedule kernel's other instance),
and the biased call (path 1) with the zero and the rough table of tests/meta_cases.py.  --compare: every key of both documents
must be there and equal; exit status 1 otherwise."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

B, LS, INTEGRATORS = 3, (4, 8, 36, 60, 64), ('leapfrog', 'omelyan', 'force_gradient')
BETA, BETAS, DT, NSTEP = 2.0, (1.5, 2.0, 3.0), 0.1, 3


def digests():
    import numpy as np
    import torch
    import meta_cases as M
    from fthmc_amd import _lib, ops
    dev = torch.device('cuda:0')
    out = {}

    def put(tag, r):
        for k in sorted(r):
            a = np.ascontiguousarray(r[k].detach().cpu().numpy()).view(np.uint64)
            out[f'{tag}/{k}'] = hashlib.sha256(a.astype('<u8', copy=False).tobytes()).hexdigest()
    bb = torch.tensor(BETAS, dtype=torch.float64, device=dev)
    for L in LS:
        x = torch.from_numpy(M.links(B, L, 100 + L, np.pi)).to(dev)
        v, u = (torch.from_numpy(a).to(dev) for a in M.draws(B, L, 200 + L))
        for integ in INTEGRATORS:
            put(f'L{L}/{integ}/beta', ops.hmc_trajectory(x, v, u, BETA, DT, NSTEP, integrator=integ))
            put(f'L{L}/{integ}/beta_b', ops.hmc_trajectory(x, v, u, bb, DT, NSTEP, integrator=integ))
            for tk in ('zero', 'rough'):
                t = M.table(tk, 1)
                put(f'L{L}/{integ}/bias_{tk}', ops.meta_trajectory(x, v, u, BETA, DT, NSTEP, torch.from_numpy(t.V).to(dev), t.qmax, t.wall,
                                                                   integrator=integ, path=1))
    torch.cuda.synchronize()
    return dict(tool='tools/resident_digest.py', library=_lib.load().fthmc_version().decode(), device=torch.cuda.get_device_name(0), digests=out)


def compare(pa, pb):
    a, b = (json.load(open(p)) for p in (pa, pb))
    keys = sorted(set(a['digests']) | set(b['digests']))
    differ = [k for k in keys if a['digests'].get(k) != b['digests'].get(k)]
    return dict(tool='tools/resident_digest.py', parent_library=a['library'], library=b['library'], device=b['device'], keys=len(keys),
                all_equal=not differ and a['device'] == b['device'], differ=differ, digests=b['digests'])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--compare', nargs=2, metavar=('PARENT.json', 'NEW.json'))
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    doc = compare(*args.compare) if args.compare else digests()
    text = json.dumps(doc, indent=1, sort_keys=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text if not args.compare else json.dumps({k: doc[k] for k in ('keys', 'all_equal', 'differ')}))
    return 0 if not args.compare or doc['all_equal'] else 1


if __name__ == '__main__':
    sys.exit(main())
