#!/usr/bin/env python3
"""Generate tests/golden/second_order_L8.npz from the REAL reference: second derivatives through the flowed action.

Runs only in the build container (the reference never travels to the GPU box), like make_golden.py, with the same three
import-time stubs and the dtype order of SURVEY Q1 (fthmc.config first, then fp64).  The fixture holds the inputs (field,
conv weights, a fixed cotangent g and per-chain weights gS) and what the reference's own autograd returns for

    F = qed_helpers.ft_force(param, flow, field, create_graph=True)                 (qed_helpers.py:226-242)
    grad((F * g).sum(), [field] + params)              -> H g and d/dw <g, F>
    grad((ft_action(param, flow, x) * gS).sum(), [x] + params)                      (qed_helpers.py:212-223)

The reference's ft_force turns requires_grad off on the field as it returns (qed_helpers.py:240): it is turned back on
before differentiating.

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

    B, L, nl, beta, act = 2, 8, 2, 2.5, 'silu'
    torch.manual_seed(5301)
    flow = layers.make_u1_equiv_layers(n_layers=nl, n_mixture_comps=2, lattice_shape=(L, L), hidden_sizes=[8, 8],
                                       kernel_size=3, activation_fn=act)
    params = list(flow.parameters())
    param = cfg.Param(beta=beta, L=L)
    x = torch.empty(B, 2, L, L).uniform_(-math.pi, math.pi)
    g = torch.randn(B, 2, L, L)
    gS = torch.tensor([0.7, -1.3])

    field = x.clone()
    F = qed.ft_force(param, flow, field, create_graph=True)
    field.requires_grad_(True)
    fgrads = torch.autograd.grad((F * g).sum(), [field] + params)

    xa = x.clone().requires_grad_(True)
    S = qed.ft_action(param, flow, xa)
    agrads = torch.autograd.grad((S * gS).sum(), [xa] + params)

    d = {'x': npy(x), 'g': npy(g), 'gS': npy(gS), 'beta': np.float64(beta), 'act': act, 'n_layers': np.int64(nl),
         'S_eff': npy(S), 'F': npy(F), 'Hg': npy(fgrads[0]), 'ga_x': npy(agrads[0])}
    k = 0
    for li, layer in enumerate(flow):
        for pi, p in enumerate(layer.parameters()):
            d[f'w{li}_{pi}'] = npy(p)
            d[f'gw{li}_{pi}'] = npy(fgrads[1 + k])
            d[f'ga_w{li}_{pi}'] = npy(agrads[1 + k])
            k += 1
    path = os.path.join(OUT, 'second_order_L8.npz')
    np.savez_compressed(path, **d)
    print(f'second_order_L8: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
