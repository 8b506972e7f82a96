"""GPU tests of the force-norm training path (TrainConfig.with_force; ipynb/ft_hmc.py:253-299): fthmc_train_force_grad against
the reference fixture and the oracle's double backward, the fused dual kernels (csrc/flow_dual.hip) against the plain dual sweep
and against 2 * ft_force_vjp(g = F), determinism and chain independence, edge inputs, train_step(with_force=True) against the
oracle's Adam step, and train() with config.with_force.

Tolerance of every comparison with the oracle: 1e-9 relative on max-norm, the figure tests/test_second_order_gpu.py uses for the same
quantities against the same oracle."""
import math

import numpy as np
import pytest
import torch

from conftest import golden_flow, load_golden
from gpu_support import D, R, module_defaults, ops, switches

pytestmark = pytest.mark.gpu
_defaults = module_defaults(dual=1)

TOL = 1e-9


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def field(B, L, gen, scale=math.pi):
    return (torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * scale


def oracle_force_loss(x, flow, beta, act='silu'):
    """CPU double backward of oracle.ref_cpu.ft_action: F, sum F_b^2, d/dw sum_b |F_b|^2 (flat, canonical order)"""
    fl = [tuple(t.detach().clone().requires_grad_(True) for t in layer) for layer in flow]
    params = [t for layer in fl for t in layer]
    xg = x.detach().cpu().clone().requires_grad_(True)
    F, = torch.autograd.grad(R.ft_action(xg, fl, beta, act).sum(), xg, create_graph=True)
    g = torch.autograd.grad((F ** 2).sum(), params) if params else []
    cat = torch.cat([t.reshape(-1) for t in g]) if g else torch.zeros(0, dtype=torch.float64)
    return F.detach(), (F.detach() ** 2).sum((1, 2, 3)), cat


# ---------------------------------------------------------------- 1. fixture
def test_matches_the_reference_fixture():
    """tests/golden/force_train_L8.npz: the reference's own autograd through ft_force(create_graph=True) and (F ** 2).sum()"""
    g = load_golden('force_train_L8')
    nl, beta = int(g['n_layers']), float(g['beta'])
    w = ops.pack_weights(golden_flow(g), device='cuda')
    gw_ref = np.concatenate([g[f'gw{li}_{pi}'].reshape(-1) for li in range(nl) for pi in range(6)])
    assert ops.train_force_path(2, 8) == 1
    r = ops.train_force_grad(D(g['x']), w, nl, beta)
    errs = [rel(r['F'], g['F']), rel(r['force_sq'], g['force_sq']), rel(r['gw'], gw_ref)]
    print('fixture errors (F, force_sq, gw):', errs)
    assert max(errs) < TOL, errs


# ---------------------------------------------------------------- 2. oracle double backward, 3. fused against generic
SHAPES = [  # (L, B, layers, act, arch)
    (8, 2, 8, 'silu', None),                 # one tile wrapping onto itself
    (16, 2, 8, 'silu', None),                # several tiles, every stripe phase
    (24, 2, 3, 'leaky_relu', None),          # several tiles, not a power of two
    (16, 3, 2, 'relu', None),
    (12, 3, 2, 'silu', None),                # 8 x 8 tiles do not divide 12: the plain dual sweep
    (8, 2, 2, 'silu', ((4, 6), 5, 3)),       # another net shape: the plain dual sweep
]
_CASES = {}


def _case(i):
    """inputs and the oracle's results of shape i, computed once and never modified"""
    if i not in _CASES:
        L, B, nl, act, arch = SHAPES[i]
        gen = torch.Generator().manual_seed(1000 * L + 10 * nl + B)
        flow = R.default_flow(nl, gen) if arch is None else R.default_flow(nl, gen, hidden=arch[0], k=arch[1], n_mix=arch[2])
        x = field(B, L, gen)
        _CASES[i] = (flow, x, oracle_force_loss(x, flow, 2.0, act))
    return _CASES[i]


@pytest.mark.parametrize('i', range(len(SHAPES)))
def test_matches_the_oracle_double_backward(i):
    L, B, nl, act, arch = SHAPES[i]
    flow, x, (F_r, fs_r, gw_r) = _case(i)
    w = ops.pack_weights(flow, device='cuda')
    r = ops.train_force_grad(D(x), w, nl, 2.0, act)
    errs = [rel(r['F'], F_r), rel(r['force_sq'], fs_r), rel(r['gw'], gw_r)]
    print(f'L={L} B={B} layers={nl} {act} fused={ops.train_force_path(B, L, arch)}: errors (F, force_sq, gw)', errs)
    assert max(errs) < TOL, errs
    # the same bound for every layer's every parameter tensor and every chain's force on its own (tests/second_order_cases.py)
    import second_order_cases as C
    each = C.per_tensor(C.split(r['gw'], flow), C.split(gw_r, flow))
    each.update(C.per_chain(r['F'], F_r, 'F'))
    assert C.hold(each, TOL, 'per tensor') < TOL


def test_fused_kernels_agree_with_the_plain_dual_sweep_and_serve_their_shapes():
    fused = 0
    for i, (L, B, nl, act, arch) in enumerate(SHAPES):
        with switches(dual=1):
            if ops.train_force_path(B, L, arch) != 1:
                continue
            fused += 1
            flow, x, (F_r, fs_r, gw_r) = _case(i)
            w = ops.pack_weights(flow, device='cuda')
            on = ops.train_force_grad(D(x), w, nl, 2.0, act)
        with switches(dual=0):
            assert ops.train_force_path(B, L, arch) == 0
            off = ops.train_force_grad(D(x), w, nl, 2.0, act)
            vjp = 2 * ops.ft_force_vjp(D(x), w, nl, 2.0, on['F'], act, need_gx=False)[1]
        assert torch.equal(on['F'], off['F']) and torch.equal(on['force_sq'], off['force_sq'])
        assert torch.equal(off['gw'], vjp)                    # the plain sweep IS the force VJP's, seeded with F, times two
        errs = [rel(on['gw'], off['gw']), rel(on['gw'], vjp), rel(off['gw'], gw_r)]
        print(f'L={L} B={B} layers={nl} {act}: fused vs plain, fused vs 2 vjp, plain vs oracle', errs)
        assert max(errs) < TOL, errs
        for tile in (2, 3):                                   # 8 x 8 tiles always / 8 x 16 tiles where they divide L
            with switches(dual=tile):
                assert rel(ops.train_force_grad(D(x), w, nl, 2.0, act)['gw'], off['gw']) < TOL
    assert fused >= 3, fused            # a silent fallback to the plain sweep cannot pass


# The walk of a workgroup over SEVERAL (chain, tile) items -- register sums carried across items, the LDS planes reused behind the
# loop's barrier, one partial row per workgroup --, the gather's own-and-both-neighbours branch (more than three tiles per
# dimension) and 8 x 16 tiles side by side without wrap need more items than the backward has workgroups (512 / 256) and
# L >= 32: L = 64 with 9 chains is 576 items of 8 x 8 tiles and 288 of 8 x 16, eight / four tiles per dimension; 288 also makes the
# default setting pick the 8 x 16 tiles.  65 chains are 4160 items of 8 x 8 tiles: beyond the forward's 4096 workgroups.
def test_many_items_per_workgroup_agree_with_the_plain_sweep_and_the_oracle():
    L, B, nl, act = 64, 9, 3, 'silu'
    gen = torch.Generator().manual_seed(640903)
    flow = R.default_flow(nl, gen)
    w = ops.pack_weights(flow, device='cuda')
    x = field(B, L, gen)
    F_r, fs_r, gw_r = oracle_force_loss(x, flow, 2.0, act)
    x = D(x)
    with switches(dual=0):
        assert ops.train_force_path(B, L) == 0
        off = ops.train_force_grad(x, w, nl, 2.0, act)
        vjp = 2 * ops.ft_force_vjp(x, w, nl, 2.0, off['F'], act, need_gx=False)[1]
        assert torch.equal(off['gw'], vjp)
    wsb = {}
    for path in (1, 2, 3):
        with switches(dual=path):
            assert ops.train_force_path(B, L) == 1
            wsb[path] = ops.train_force_ws_bytes(B, L, nl)
            on = ops.train_force_grad(x, w, nl, 2.0, act)
            again = ops.train_force_grad(x, w, nl, 2.0, act)
        assert torch.equal(on['gw'], again['gw']) and torch.equal(on['F'], off['F'])
        errs = [rel(on['gw'], off['gw']), rel(on['gw'], vjp), rel(on['gw'], gw_r), rel(on['F'], F_r), rel(on['force_sq'], fs_r)]
        print(f'L={L} B={B} layers={nl} path {path}: fused vs plain, vs 2 vjp, vs oracle; F, force_sq vs oracle', errs)
        assert max(errs) < TOL, (path, errs)
    # the default picked the 8 x 16 tiles here: its workspace is theirs, not the 8 x 8 tiles'
    assert wsb[1] == wsb[3] != wsb[2]
    # more items than the forward kernel has workgroups
    B2, nl2 = 65, 2
    w2 = ops.pack_weights(R.default_flow(nl2, gen), device='cuda')
    x2 = D(field(B2, L, gen))
    with switches(dual=0):
        off2 = ops.train_force_grad(x2, w2, nl2, 2.0, 'relu')
    with switches(dual=2):
        assert ops.train_force_path(B2, L) == 1
        on2 = ops.train_force_grad(x2, w2, nl2, 2.0, 'relu')
        vjp2 = 2 * ops.ft_force_vjp(x2, w2, nl2, 2.0, on2['F'], 'relu', need_gx=False)[1]
    errs = [rel(on2['gw'], off2['gw']), rel(on2['gw'], vjp2)]
    print(f'L={L} B={B2} layers={nl2} path 2: fused vs plain, vs 2 vjp', errs)
    assert max(errs) < TOL and torch.equal(on2['F'], off2['F']), errs


# ---------------------------------------------------------------- 4. determinism and independence
def test_determinism_chain_independence_and_the_other_switches():
    L, B, nl = 16, 3, 4
    gen = torch.Generator().manual_seed(77)
    w = ops.pack_weights(R.default_flow(nl, gen), device='cuda')
    x = D(field(B, L, gen))
    a = ops.train_force_grad(x, w, nl, 2.0)
    b = ops.train_force_grad(x, w, nl, 2.0)
    assert all(torch.equal(a[k], b[k]) for k in ('F', 'force_sq', 'gw'))
    ones = [ops.train_force_grad(x[c:c + 1].contiguous(), w, nl, 2.0) for c in range(B)]
    assert torch.equal(torch.cat([o['F'] for o in ones]), a['F'])
    assert torch.equal(torch.cat([o['force_sq'] for o in ones]), a['force_sq'])
    assert rel(sum(o['gw'] for o in ones), a['gw']) < 1e-12
    # the first-order force may differ between the variants and the small path by its own rounding, gw follows at 1e-9
    for variant, small in ((0, True), (1, False), (0, False)):
        with switches(variant=variant, small=small):
            c = ops.train_force_grad(x, w, nl, 2.0)
            assert rel(c['F'], ops.ft_force(x, w, nl, 2.0)) == 0.0
        assert rel(c['F'], a['F']) < TOL and rel(c['force_sq'], a['force_sq']) < TOL and rel(c['gw'], a['gw']) < TOL


# ---------------------------------------------------------------- 5. edge inputs
def test_edge_inputs():
    from fthmc_amd import _lib, ops
    L, B, nl = 8, 2, 2
    gen = torch.Generator().manual_seed(5)
    w = ops.pack_weights(R.default_flow(nl, gen), device='cuda')
    x = D(field(B, L, gen))
    # no layers: the Wilson force, gw untouched
    r0 = ops.train_force_grad(x, None, 0, 1.7)
    assert torch.equal(r0['F'], ops.wilson_force(x, 1.7)) and r0['gw'] is None
    assert rel(r0['force_sq'], (r0['F'] ** 2).sum((1, 2, 3))) < 1e-14
    lib = _lib.load()
    sentinel = torch.full((7,), 3.25, dtype=torch.float64, device='cuda')
    F, fsq = torch.empty_like(x), torch.empty(B, dtype=torch.float64, device='cuda')
    nb = ops.train_force_ws_bytes(B, L, 0)
    ws = torch.zeros(nb // 8 + 1, dtype=torch.float64, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    assert lib.fthmc_train_force_grad(x.data_ptr(), None, None, 0, B, L, 0, 1.7, F.data_ptr(), fsq.data_ptr(), sentinel.data_ptr(),
                                      ws.data_ptr(), nb, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(F, r0['F']) and bool((sentinel == 3.25).all())
    # gw not wanted: the same F and force_sq, bit for bit; F not wanted: the same force_sq and gw
    full = ops.train_force_grad(x, w, nl, 2.0)
    nogw = ops.train_force_grad(x, w, nl, 2.0, need_gw=False)
    assert nogw['gw'] is None and torch.equal(nogw['F'], full['F']) and torch.equal(nogw['force_sq'], full['force_sq'])
    out = torch.zeros(w.numel() + 3, dtype=torch.float64, device='cuda')
    into = ops.train_force_grad(x, w, nl, 2.0, out_gw=out[:w.numel()])
    assert into['gw'].data_ptr() == out.data_ptr() and torch.equal(out[:w.numel()], full['gw']) and bool((out[w.numel():] == 0).all())
    nb = ops.train_force_ws_bytes(B, L, nl)
    ws = torch.zeros(nb // 8 + 1, dtype=torch.float64, device='cuda')
    gw = torch.empty_like(w)
    args = (x.data_ptr(), w.data_ptr(), None, nl, B, L, 0, 2.0)
    assert lib.fthmc_train_force_grad(*args, None, fsq.data_ptr(), gw.data_ptr(), ws.data_ptr(), nb, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(fsq, full['force_sq']) and torch.equal(gw, full['gw'])
    # a short workspace
    E_WS = -4
    assert lib.fthmc_train_force_grad(*args, F.data_ptr(), fsq.data_ptr(), gw.data_ptr(), ws.data_ptr(), nb - 8, st) == E_WS
    assert lib.fthmc_train_force_grad(*args, F.data_ptr(), fsq.data_ptr(), gw.data_ptr(), ws.data_ptr(), ops.ws_bytes(B, L, nl), st) == E_WS
    assert lib.fthmc_train_force_grad(*args, F.data_ptr(), fsq.data_ptr(), gw.data_ptr(), None, nb, st) == E_WS
    with pytest.raises(ops.FthmcError):
        ops.train_force_grad(x, w, nl, 2.0, out_gw=torch.zeros(5, dtype=torch.float64, device='cuda'))


# ---------------------------------------------------------------- 6. train_step(with_force=True)
def _model(L, nl, B, seed, beta=2.0):
    from fthmc_amd import train as T
    from fthmc_amd.config import TrainConfig
    cfg = TrainConfig(L=L, beta=beta, n_layers=nl, batch_size=B, print_freq=0, base_lr=1e-3)
    torch.manual_seed(seed)
    return cfg, T.get_model(cfg)


def _oracle_flow(layers):
    from fthmc_amd.utils.layers import net_weights
    return [tuple(p.detach().cpu().clone() for p in net_weights(layer.plaq_coupling.net)) for layer in layers]


def test_train_step_with_force_takes_the_oracles_adam_step():
    from fthmc_amd import ops, train as T
    from fthmc_amd.utils import qed_helpers as qed
    from fthmc_amd.utils.layers import flow_weights
    L, B, nl, beta, lr = 8, 4, 4, 2.0, 1e-3
    cfg, model = _model(L, nl, B, 11)
    oflow = _oracle_flow(model.layers)
    xi = D(field(B, L, torch.Generator().manual_seed(12)))
    F_r, fs_r, gw_r = oracle_force_loss(xi, oflow, beta)
    opt = T.FlatAdam(model.layers, lr=lr)
    w0 = flow_weights(model.layers, 'cuda').clone()
    out = T.train_step(model, cfg, qed.BatchAction(beta), opt, B, xi=xi, with_force=True)
    # torch's Adam, first step: m = (1 - b1) g, v = (1 - b2) g^2, w -= lr (m / (1 - b1)) / (sqrt(v / (1 - b2)) + eps)
    g = gw_r.cuda()
    want = w0 - lr * g / (g.abs() + 1e-8)
    w1 = flow_weights(model.layers, 'cuda')
    # the gradient itself, where the optimizer reads it: the flat buffer and every parameter's .grad view of it (a first Adam step
    # alone depends on little more than the gradient's signs)
    from fthmc_amd.utils.layers import flow_grad_buffer, net_weights
    assert rel(flow_grad_buffer(model.layers), gw_r) < TOL
    grads = torch.cat([p.grad.reshape(-1) for layer in model.layers for p in net_weights(layer.plaq_coupling.net)])
    assert rel(grads, gw_r) < TOL
    assert rel(w1 - w0, want - w0) < TOL and rel(w1, want) < TOL, (rel(w1 - w0, want - w0), rel(w1, want))
    assert abs(float(out['force']) - float(fs_r.sum())) < TOL * float(fs_r.sum()) and float(out['loss']) == float(out['force'])
    # the other metrics: those of a reverse-KL evaluation at the same xi with the weights before the step
    r = ops.train_grad(xi, w0, nl, beta, need_gw=False)
    m = T._metrics_dict(ops.train_metrics(xi, r['x'], r['logq'], r['logp'], beta, 1.0).cpu().numpy(), B)
    for k in T.METRIC_KEYS:
        assert np.array_equal(np.asarray(out[k]), np.asarray(m[k])), k
    assert set(out) == set(T.METRIC_KEYS) | {'force', 'loss', 'dt'}
    # the autograd route (fused=False) takes the same step
    cfg2, model2 = _model(L, nl, B, 11)
    opt2 = torch.optim.Adam(model2.layers.parameters(), lr=lr)
    out2 = T.train_step(model2, cfg2, qed.BatchAction(beta), opt2, B, xi=xi, fused=False, with_force=True)
    grads2 = torch.cat([p.grad.reshape(-1) for layer in model2.layers for p in net_weights(layer.plaq_coupling.net)])
    assert rel(grads2, gw_r) < TOL
    # a second step on either route: Adam's moments now weigh two different gradients, so their magnitudes matter
    xi2 = D(field(B, L, torch.Generator().manual_seed(13)))
    T.train_step(model, cfg, qed.BatchAction(beta), opt, B, xi=xi2, with_force=True)
    T.train_step(model2, cfg2, qed.BatchAction(beta), opt2, B, xi=xi2, fused=False, with_force=True)
    assert rel(flow_weights(model.layers, 'cuda'), flow_weights(model2.layers, 'cuda')) < TOL
    assert rel(flow_weights(model2.layers, 'cuda'), want) > 1e-6           # the second step moved them
    assert abs(float(out2['force']) - float(out['force'])) < TOL * float(out['force'])


def test_train_step_without_the_flag_returns_what_it_returned():
    from fthmc_amd import train as T
    from fthmc_amd.utils import qed_helpers as qed
    L, B, nl, beta = 8, 4, 2, 2.0
    cfg, model = _model(L, nl, B, 21)
    xi = D(field(B, L, torch.Generator().manual_seed(22)))
    out = T.train_step(model, cfg, qed.BatchAction(beta), T.FlatAdam(model.layers, lr=1e-3), B, xi=xi)
    assert set(out) == set(T.METRIC_KEYS) | {'dt'}
    out = T.train_step(model, cfg, qed.BatchAction(beta), T.FlatAdam(model.layers, lr=1e-3), B, xi=xi, with_force=False)
    assert set(out) == set(T.METRIC_KEYS) | {'dt'}


def test_train_step_with_force_and_a_pre_model_follows_the_notebook(monkeypatch):
    """xi = the pre-model's prior through the pre-model's layers, then back through the inverse of the model being trained
    (ipynb/ft_hmc.py:258-262): flow_forward(model, xi) returns to flow_forward(pre_model, pre_xi)"""
    from fthmc_amd import ops, train as T
    from fthmc_amd.utils import qed_helpers as qed
    from fthmc_amd.utils.layers import flow_weights
    L, B, nl, beta = 8, 4, 2, 2.0
    cfg, model = _model(L, nl, B, 31)
    _, pre = _model(L, nl, B, 32)
    w_model, w_pre = flow_weights(model.layers, 'cuda').clone(), flow_weights(pre.layers, 'cuda').clone()
    seen = {}
    real = ops.train_force_grad

    def spy(xi, *a, **k):
        seen['xi'] = xi.clone()
        return real(xi, *a, **k)

    pre_xi = D(field(B, L, torch.Generator().manual_seed(33)))
    monkeypatch.setattr(pre.prior, 'sample_n', lambda n: pre_xi.clone())
    monkeypatch.setattr(ops, 'train_force_grad', spy)
    out = T.train_step(model, cfg, qed.BatchAction(beta), T.FlatAdam(model.layers, lr=1e-4), B, pre_model=pre, with_force=True)
    assert 'force' in out and seen['xi'].shape == pre_xi.shape
    x_model = ops.flow_forward(seen['xi'], w_model, nl)[0]
    x_pre = ops.flow_forward(pre_xi, w_pre, nl)[0]
    # the inverse's tolerance: the Newton loop stops at 1e-12 per plaquette, links are compared modulo 2 pi
    d = torch.remainder(x_model - x_pre + math.pi, 2 * math.pi) - math.pi
    assert float(d.abs().max()) < 1e-9, float(d.abs().max())
    assert not torch.equal(seen['xi'], pre_xi)


def test_operator_agrees_with_ops():
    import fthmc_amd.torch_ops as TO
    assert 'train_force_grad' in TO.__all__
    L, B, nl = 16, 2, 3
    gen = torch.Generator().manual_seed(41)
    w = ops.pack_weights(R.default_flow(nl, gen), device='cuda')
    x = D(field(B, L, gen))
    r = ops.train_force_grad(x, w, nl, 2.0, 'relu')
    F, fsq, gw = torch.ops.fthmc_hip.train_force_grad(x, w, nl, 2.0, 1)
    assert torch.equal(F, r['F']) and torch.equal(fsq, r['force_sq']) and torch.equal(gw, r['gw'])
    F0, fsq0, gw0 = torch.ops.fthmc_hip.train_force_grad(x, torch.zeros(0, dtype=torch.float64, device='cuda'), 0, 2.0, 0)
    assert torch.equal(F0, ops.wilson_force(x, 2.0)) and gw0.numel() == 0
    flow = R.default_flow(2, gen, hidden=(4, 6), k=5, n_mix=3)
    wa = ops.pack_weights(flow, device='cuda')
    ra = ops.train_force_grad(x, wa, 2, 2.0)
    Fa, _, gwa = torch.ops.fthmc_hip.train_force_grad(x, wa, 2, 2.0, 0, 3, [4, 6], 5)
    assert torch.equal(Fa, ra['F']) and torch.equal(gwa, ra['gw'])


# ---------------------------------------------------------------- 7. train() with config.with_force
def test_train_with_force_runs_both_steps():
    from fthmc_amd import train as T
    from fthmc_amd.config import TrainConfig
    from fthmc_amd.utils.layers import flow_weights

    def run(with_force):
        cfg = TrainConfig(L=8, beta=2.0, n_layers=2, batch_size=8, n_era=1, n_epoch=3, print_freq=0, base_lr=1e-3, with_force=with_force)
        torch.manual_seed(51)
        model = T.get_model(cfg)
        torch.manual_seed(52)
        out = T.train(cfg, model=model, verbose=False, use_graph=False)
        return out, flow_weights(model.layers, 'cuda').clone()

    out, w_force = run(True)
    assert len(out['history']['force']) == 3 and all(np.isfinite(float(f)) and float(f) > 0 for f in out['history']['force'])
    assert len(out['history']['loss_dkl']) == 3
    out0, w_plain = run(False)
    assert 'force' not in out0['history']
    assert not torch.equal(w_force, w_plain)
