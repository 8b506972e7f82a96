#!/usr/bin/env python3
"""Generate tests/golden/force_train_L8.npz from the REAL reference: the force-norm training loss and its parameter gradients.

Runs only in the build container (the reference never travels to the GPU box), like make_golden_second_order.py, with the same
three import-time stubs and the dtype order of SURVEY Q1 (fthmc.config first, then fp64).  The fixture holds the inputs (field,
conv weights of 8 layers, so that every (mu, off) pair of the stripe masks occurs) and what the reference's own autograd
returns for the with_force branch of ipynb/ft_hmc.py:253-299:

    F = qed_helpers.ft_force(param, flow, x, create_graph=True)                     (qed_helpers.py:226-242)
    force_sq[b] = sum over the links of F_b^2
    grad((F ** 2).sum(), params)

    cd <repo> && python tests/golden/make_golden_force_train.py
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

    B, L, nl, beta, act = 2, 8, 8, 2.0, 'silu'
    torch.manual_seed(7411)
    flow = layers.make_u1_equiv_layers(n_layers=nl, n_mixture_comps=2, lattice_shape=(L, L), hidden_sizes=[8, 8],
                                       kernel_size=3, activation_fn=act)
    params = list(flow.parameters())
    param = cfg.Param(beta=beta, L=L)
    x = torch.empty(B, 2, L, L).uniform_(-math.pi, math.pi)

    F = qed.ft_force(param, flow, x.clone(), create_graph=True)
    grads = torch.autograd.grad((F ** 2).sum(), params)

    d = {'x': npy(x), 'beta': np.float64(beta), 'act': act, 'n_layers': np.int64(nl), 'F': npy(F),
         'force_sq': npy((F ** 2).sum(dim=(1, 2, 3)))}
    k = 0
    for li, layer in enumerate(flow):
        for pi, p in enumerate(layer.parameters()):
            d[f'w{li}_{pi}'] = npy(p)
            d[f'gw{li}_{pi}'] = npy(grads[k])
            k += 1
    path = os.path.join(OUT, 'force_train_L8.npz')
    np.savez_compressed(path, **d)
    print(f'force_train_L8: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
