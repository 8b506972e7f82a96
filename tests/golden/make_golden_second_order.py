#!/usr/bin/env python3
"""Generate tests/golden/second_order_L8.npz and second_order_steep_L8.npz from the REAL reference: second derivatives through
the flowed action.

Runs only in the build container (the reference never travels to the GPU box), like make_golden.py, with the same three
import-time stubs and the dtype order of SURVEY Q1 (fthmc.config first, then fp64).  The fixture holds the inputs (field,
conv weights, a fixed cotangent g and per-chain weights gS) and what the reference's own autograd returns for

    F = qed_helpers.ft_force(param, flow, field, create_graph=True)                 (qed_helpers.py:226-242)
    grad((F * g).sum(), [field] + params)              -> H g and d/dw <g, F>
    grad((ft_action(param, flow, x) * gS).sum(), [x] + params)                      (qed_helpers.py:212-223)

The reference's ft_force turns requires_grad off on the field as it returns (qed_helpers.py:240): it is turned back on
before differentiating.

second_order_steep_L8.npz is the hard case of tests/second_order_cases.py from the reference itself: 8 layers (every (mu, off)), the
module's parameters multiplied by 3 in place (saturated sigmoids, steep transforms), links pinned 1e-9 from +-pi
(x[0, 0, 0, :] = pi - 1e-9, x[0, 1, :, 0] = -pi + 1e-9), and in addition grad((F ** 2).sum(), params), the with_force loss of
make_golden_force_train.py.  Its seed is chosen by the reference's conditioning alone (tests/test_second_order_hard.py asserts it):
of the seeds 5308 .. 5312 the one at which the results move least, 5e-13 per tensor at most, when every input moves by one relative
2^-52 (the others: 0.8 .. 1.9e-12, at the edge of what a 1e-9 bound per tensor allows).

    cd <repo> && python tests/golden/make_golden_second_order.py
"""
import math
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, OUT, _stub_modules  # noqa: E402


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    import torch
    _stub_modules()
    os.chdir(tempfile.mkdtemp(prefix='fthmc_golden_'))

    import fthmc.config as cfg          # resets default dtype to fp32 (Q1)
    torch.set_default_dtype(torch.float64)
    import fthmc.utils.qed_helpers as qed
    import fthmc.utils.layers as layers

    def npy(t):
        return t.detach().cpu().numpy().astype(np.float64)

    def write(name, nl, beta, seed, scale=1.0, pin=False, force_loss=False):
        B, L, act = 2, 8, 'silu'
        torch.manual_seed(seed)
        flow = layers.make_u1_equiv_layers(n_layers=nl, n_mixture_comps=2, lattice_shape=(L, L), hidden_sizes=[8, 8],
                                           kernel_size=3, activation_fn=act)
        params = list(flow.parameters())
        if scale != 1.0:
            with torch.no_grad():
                for p in params:
                    p.mul_(scale)
        param = cfg.Param(beta=beta, L=L)
        x = torch.empty(B, 2, L, L).uniform_(-math.pi, math.pi)
        if pin:
            x[0, 0, 0, :] = math.pi - 1e-9
            x[0, 1, :, 0] = -math.pi + 1e-9
        g = torch.randn(B, 2, L, L)
        gS = torch.tensor([0.7, -1.3])

        field = x.clone()
        F = qed.ft_force(param, flow, field, create_graph=True)
        field.requires_grad_(True)
        fgrads = torch.autograd.grad((F * g).sum(), [field] + params, retain_graph=force_loss)
        qgrads = torch.autograd.grad((F ** 2).sum(), params) if force_loss else None

        xa = x.clone().requires_grad_(True)
        S = qed.ft_action(param, flow, xa)
        agrads = torch.autograd.grad((S * gS).sum(), [xa] + params)

        d = {'x': npy(x), 'g': npy(g), 'gS': npy(gS), 'beta': np.float64(beta), 'act': act, 'n_layers': np.int64(nl),
             'S_eff': npy(S), 'F': npy(F), 'Hg': npy(fgrads[0]), 'ga_x': npy(agrads[0])}
        if force_loss:
            d['force_sq'] = npy((F ** 2).sum(dim=(1, 2, 3)))
        k = 0
        for li, layer in enumerate(flow):
            for pi, p in enumerate(layer.parameters()):
                d[f'w{li}_{pi}'] = npy(p)
                d[f'gw{li}_{pi}'] = npy(fgrads[1 + k])
                d[f'ga_w{li}_{pi}'] = npy(agrads[1 + k])
                if force_loss:
                    d[f'gq{li}_{pi}'] = npy(qgrads[k])
                k += 1
        path = os.path.join(OUT, name + '.npz')
        np.savez_compressed(path, **d)
        print(f'{name}: {os.path.getsize(path) / 1024:.1f} KiB')

    only = sys.argv[1:]
    if not only or 'second_order_L8' in only:
        write('second_order_L8', 2, 2.5, 5301)
    if not only or 'second_order_steep_L8' in only:
        write('second_order_steep_L8', 8, 2.0, 5310, scale=3.0, pin=True, force_loss=True)

if __name__ == '__main__':
    main()
