#!/usr/bin/env python3
"""Generate tests/golden/first_order_steep_L8.npz from the REAL reference: the first-order quantities at the hard case of
tests/first_order_cases.py.

Runs only in the build container (the reference never travels to the GPU box), like make_golden_second_order.py, with the same
three import-time stubs and the dtype order of SURVEY Q1 (fthmc.config first, then fp64).  The inputs are those of
second_order_steep_L8.npz, drawn the same way from the same seed (tests/test_first_order_hard.py asserts that they are the same
bits): L = 8, B = 2, 8 layers (every (mu, off)), the module's parameters multiplied by 3 in place (saturated sigmoids, steep
transforms), links pinned 1e-9 from +-pi (x[0, 0, 0, :] = pi - 1e-9, x[0, 1, :, 0] = -pi + 1e-9), beta = 2.  The fixture holds them
and what the reference returns for

    F = qed_helpers.ft_force(param, flow, x)                                        (qed_helpers.py:226-242)
    S_eff = qed_helpers.ft_action(param, flow, x)                                   (qed_helpers.py:212-223)
    train.train_step(model, config, BatchAction(beta), SGD(lr = 0), B, xi = x)      (train.py:162-228)
        -> loss_dkl, logq, logp and the gradients loss_dkl.backward() leaves on the parameters (the optimizer's step moves
           nothing: the stored weights are asserted unchanged)

    cd <repo> && python tests/golden/make_golden_first_order_steep.py
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
    import fthmc.utils.samplers as samplers
    import fthmc.train as train
    from fthmc.utils.distributions import MultivariateUniform
    cfg.DTYPE = torch.float64
    samplers.DTYPE = torch.float64

    def npy(t):
        return t.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(t) else np.asarray(t, dtype=np.float64)

    B, L, nl, beta, act, seed, scale = 2, 8, 8, 2.0, 'silu', 5310, 3.0
    torch.manual_seed(seed)
    flow = layers.make_u1_equiv_layers(n_layers=nl, n_mixture_comps=2, lattice_shape=(L, L), hidden_sizes=[8, 8],
                                       kernel_size=3, activation_fn=act)
    with torch.no_grad():
        for p in flow.parameters():
            p.mul_(scale)
    param = cfg.Param(beta=beta, L=L)
    x = torch.empty(B, 2, L, L).uniform_(-math.pi, math.pi)
    x[0, 0, 0, :] = math.pi - 1e-9
    x[0, 1, :, 0] = -math.pi + 1e-9

    d = {'x': npy(x), 'beta': np.float64(beta), 'act': act, 'n_layers': np.int64(nl)}
    for li, layer in enumerate(flow):
        for pi, p in enumerate(layer.parameters()):
            d[f'w{li}_{pi}'] = npy(p)

    d['F'] = npy(qed.ft_force(param, flow, x.clone()))
    with torch.no_grad():
        d['S_eff'] = npy(qed.ft_action(param, flow, x.clone()))

    tc = cfg.TrainConfig(L=L, beta=beta, debug=True, n_layers=nl, batch_size=B, base_lr=0.0)
    prior = MultivariateUniform(-math.pi * torch.ones((2, L, L)), math.pi * torch.ones((L, L)))
    model = cfg.FlowModel(prior=prior, layers=flow)
    optimizer = torch.optim.SGD(flow.parameters(), lr=0.0)
    metrics = train.train_step(model, tc, qed.BatchAction(beta), optimizer, B, xi=x.clone())
    for li, layer in enumerate(flow):
        for pi, p in enumerate(layer.parameters()):
            assert np.array_equal(npy(p), d[f'w{li}_{pi}'])             # lr = 0: the step moved nothing
            d[f'gw{li}_{pi}'] = npy(p.grad)
    for k in ('loss_dkl', 'logq', 'logp'):
        d[k] = npy(metrics[k])
    path = os.path.join(OUT, 'first_order_steep_L8.npz')
    np.savez_compressed(path, **d)
    print(f'first_order_steep_L8: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
