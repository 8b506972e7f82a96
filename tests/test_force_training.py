"""CPU-only tests of the force-norm training path (TrainConfig.with_force; ipynb/ft_hmc.py:253-299): the C ABI declares and
exports it, the ctypes signatures, the workspace sizes, the fixture against the oracle, the gradient identity the GPU tests
lean on, and the routing of `train()` / `train_step`."""
import inspect
import os
import re

import numpy as np
import torch

from conftest import ROOT, golden_flow, load_golden

NEW = ('fthmc_train_force_grad', 'fthmc_train_force_ws_bytes', 'fthmc_set_dual_path', 'fthmc_get_dual_path', 'fthmc_train_force_path')


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def test_header_library_and_signatures_carry_the_force_training_entry_points():
    from fthmc_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'fthmc_hip.h')).read()
    declared = set(re.findall(r'\b(fthmc_[a-z0-9_]+)\s*\(', header))
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES['fthmc_train_force_grad']) == 14
    assert _lib.SIGNATURES['fthmc_train_force_ws_bytes'] == _lib.SIGNATURES['fthmc_ws_bytes']
    assert _lib.SIGNATURES['fthmc_set_dual_path'] == _lib.SIGNATURES['fthmc_set_small_path']
    # every new declaration cites the notebook's lines
    for name in NEW:
        i = header.index(name + '(')
        assert 'ipynb/ft_hmc.py:253-299' in header[max(0, i - 2500):i + 400], name


def test_the_switch_defaults_to_on_and_takes_only_its_values():
    from fthmc_amd import _lib, ops
    lib = _lib.load()
    assert ops.get_dual_path() == 1
    try:
        for v in (0, 2, 3, 1):
            ops.set_dual_path(v)
            assert ops.get_dual_path() == v
        assert lib.fthmc_set_dual_path(4) == lib.fthmc_set_dual_path(-1) != 0 and ops.get_dual_path() == 1
        # which sweep serves a shape: the fused kernels need the default net and 8 x 8 tiles that divide the lattice
        assert [ops.train_force_path(2, L) for L in (4, 8, 12, 16, 24, 64, 256)] == [0, 1, 0, 1, 1, 1, 1]
        assert ops.train_force_path(2, 8, ((4, 6), 5, 3)) == 0
        ops.set_dual_path(0)
        assert [ops.train_force_path(2, L) for L in (8, 16, 64)] == [0, 0, 0]
    finally:
        ops.set_dual_path(1)


def test_train_force_workspace_sizes():
    from fthmc_amd import _lib, ops
    lib = _lib.load()
    head = int(lib.fthmc_ws_head_bytes())
    try:
        for path in (1, 0, 2, 3):
            ops.set_dual_path(path)
            for a in (None, ((4, 6), 5, 3)):
                ap = ops._arch(a)
                prev = 0
                for B, L, nl in ((1, 8, 0), (1, 8, 1), (2, 8, 1), (2, 16, 1), (2, 16, 2), (8, 64, 2), (8, 64, 8), (32, 256, 16)):
                    n = int(lib.fthmc_train_force_ws_bytes(ap, B, L, nl))
                    assert n >= head and n > prev and n > int(lib.fthmc_ws_bytes(ap, B, L, nl)), (path, a, B, L, nl, n, prev)
                    prev = n
                assert ops.train_force_ws_bytes(4, 16, 3, a) == lib.fthmc_train_force_ws_bytes(ap, 4, 16, 3)
            # refused L, B, layer count; sizes beyond size_t
            for B, L, nl in ((0, 8, 2), (2, 6, 2), (2, 0, 2), (2, 8, -1), (4194304, 8, 1), (2, 32768, 1), (4194303, 32764, 64),
                             (1 << 20, 32764, 1 << 20)):
                assert lib.fthmc_train_force_ws_bytes(None, B, L, nl) == 0, (path, B, L, nl)
            assert lib.fthmc_train_force_ws_bytes(ops._arch(((8, 8), 17, 2)), 2, 8, 2) == 0      # a refused arch
            assert lib.fthmc_train_force_ws_bytes(ops._arch(((4,), 15, 2)), 2, 4, 2) == 0       # circular pad wider than the lattice
        # the fused sweep keeps the dual checkpoint chain only: far below the plain sweep's activation planes
        ops.set_dual_path(1)
        fused = ops.train_force_ws_bytes(32, 256, 16)
        ops.set_dual_path(0)
        assert fused < ops.train_force_ws_bytes(32, 256, 16) // 2
    finally:
        ops.set_dual_path(1)


def _oracle_force_loss(x, flow, beta, act='silu', detach_one=False):
    from oracle import ref_cpu as R
    fl = [tuple(t.detach().clone().requires_grad_(True) for t in layer) for layer in flow]
    params = [t for layer in fl for t in layer]
    xg = x.detach().clone().requires_grad_(True)
    F, = torch.autograd.grad(R.ft_action(xg, fl, beta, act).sum(), xg, create_graph=True)
    loss = (F * F.detach()).sum() if detach_one else (F ** 2).sum()
    return F.detach(), torch.autograd.grad(loss, params)


def test_oracle_reproduces_the_force_training_fixture():
    g = load_golden('force_train_L8')
    nl, beta = int(g['n_layers']), float(g['beta'])
    assert (nl, g['x'].shape, str(g['act'])) == (8, (2, 2, 8, 8), 'silu')
    F, grads = _oracle_force_loss(torch.as_tensor(g['x']), golden_flow(g), beta)
    assert rel(F, g['F']) < 1e-12
    assert rel((F ** 2).sum((1, 2, 3)), g['force_sq']) < 1e-12
    ref = np.concatenate([g[f'gw{li}_{pi}'].reshape(-1) for li in range(nl) for pi in range(6)])
    assert rel(torch.cat([t.reshape(-1) for t in grads]), ref) < 1e-12


def test_oracle_confirms_the_gradient_identity():
    """d/dw sum_b |F_b|^2 = 2 d/dw <F, F_detached>: what fthmc_train_force_grad computes (one force, one dual sweep seeded with
    it) IS the gradient of the notebook's loss, and 2 * ft_force_vjp(g = F) is a fair cross-check of it"""
    from oracle import ref_cpu as R
    for L, B, nl, act in ((8, 2, 3, 'silu'), (12, 2, 2, 'relu')):
        gen = torch.Generator().manual_seed(17 * L + nl)
        flow = R.default_flow(nl, gen)
        x = (torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * 3.14159
        _, full = _oracle_force_loss(x, flow, 2.0, act)
        _, half = _oracle_force_loss(x, flow, 2.0, act, detach_one=True)
        a, b = torch.cat([t.reshape(-1) for t in full]), torch.cat([2 * t.reshape(-1) for t in half])
        assert rel(b, a) < 1e-13


def test_train_step_and_ops_carry_the_new_arguments():
    from fthmc_amd import ops, train as T
    sig = inspect.signature(T.train_step)
    assert list(sig.parameters)[-1] == 'with_force' and sig.parameters['with_force'].default is False
    sig = inspect.signature(ops.train_force_grad)
    assert list(sig.parameters) == ['xi', 'w', 'n_layers', 'beta', 'act', 'need_gw', 'out_gw', 'arch']
    for name in ('train_force_ws_bytes', 'set_dual_path', 'get_dual_path'):
        assert callable(getattr(ops, name))


def test_train_step_refuses_a_scaler_with_the_force_step():
    import pytest
    from fthmc_amd import train as T
    with pytest.raises(ValueError, match='GradScaler'):
        T.train_step(None, None, None, None, 4, scaler=object(), with_force=True)


def test_train_honours_config_with_force(monkeypatch):
    """TrainConfig(with_force=True) reaches train()'s branch: every epoch a reverse-KL step, then a force-norm step on a second
    optimizer at base_lr / 100 (ipynb/ft_hmc.py:321, 338-343)"""
    from fthmc_amd import train as T
    from fthmc_amd.config import TrainConfig
    calls = []

    def fake_step(model, config, action, optimizer, batch_size, **kw):
        calls.append((bool(kw.get('with_force', False)), optimizer, float(optimizer.param_groups[0]['lr'])))
        out = {'loss_dkl': np.float64(1.0), 'ess': np.float64(0.5), 'plaq': np.zeros(batch_size)}
        if kw.get('with_force'):
            out['force'] = np.float64(3.0)
        return out

    monkeypatch.setattr(T, 'train_step', fake_step)
    cfg = TrainConfig(L=8, beta=2.0, n_layers=2, batch_size=4, n_era=1, n_epoch=3, print_freq=0, with_force=True, base_lr=1e-3)
    torch.manual_seed(1)
    from fthmc_amd.config import FlowModel
    layers = torch.nn.ModuleList([torch.nn.Conv2d(2, 3, 3, dtype=torch.float64)])      # train() itself only hands the model on
    out = T.train(cfg, model=FlowModel(prior=None, layers=layers), verbose=False)      # a host model: the fake step runs no kernel
    assert [c[0] for c in calls] == [False, True] * 3
    assert len(out['history']['force']) == 3 and len(out['history']['loss_dkl']) == 3
    kl_opt, wf_opt = calls[0][1], calls[1][1]
    assert out['optimizer'] is kl_opt and out['optimizer_wf'] is wf_opt
    assert kl_opt is not wf_opt and type(kl_opt) is type(wf_opt)
    assert calls[0][2] == 1e-3 and abs(calls[1][2] - 1e-5) < 1e-20
    # without the flag: no force step (the loop runs through GraphTrainer, which the fake never sees)
    calls.clear()
    assert not TrainConfig(L=8, beta=2.0, n_layers=2, batch_size=4).with_force
