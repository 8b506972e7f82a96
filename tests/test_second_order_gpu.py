"""GPU tests of the second-order path: fthmc_ft_action_vjp / fthmc_ft_force_vjp against the reference fixture and the oracle's
double backward, the differentiable public API (ft_force(create_graph=True), ft_action, FieldTransformation.action, the
ft_action_force operator), consistency with the first-order paths, and properties of the Hessian at full size."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from gpu_support import D, module_defaults

pytestmark = pytest.mark.gpu
_defaults = module_defaults()


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def field(B, L, gen, scale=math.pi):
    return (torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * scale


def oracle_vjps(x, flow, beta, act, g, gS, glogdet):
    """CPU double backward of oracle.ref_cpu.ft_action: (H g, d/dw <g, F>) and (d/dx, d/dw of sum gS S_eff + glogdet logdet)"""
    from oracle import ref_cpu as R
    fl = [tuple(t.detach().clone().requires_grad_(True) for t in layer) for layer in flow]
    params = [t for layer in fl for t in layer]
    xg = x.detach().clone().requires_grad_(True)
    F, = torch.autograd.grad(R.ft_action(xg, fl, beta, act).sum(), xg, create_graph=True)
    f = torch.autograd.grad((F * g).sum(), [xg] + params)
    y, logdet = R.flow_forward(xg, fl, act)
    S = R.action(y, beta) - logdet
    a = torch.autograd.grad((gS * S).sum() + (glogdet * logdet).sum(), [xg] + params)
    cat = lambda gs: torch.cat([t.reshape(-1) for t in gs]) if gs else torch.zeros(0, dtype=torch.float64)
    return (f[0], cat(f[1:])), (a[0], cat(a[1:]))


def _flow_module(L, nl, act='silu', seed=3):
    from fthmc_amd.utils import layers as Lyr
    torch.manual_seed(seed)
    flow = Lyr.make_u1_equiv_layers(n_layers=nl, n_mixture_comps=2, lattice_shape=(L, L), hidden_sizes=[8, 8], kernel_size=3,
                                    activation_fn=act)
    return flow.cuda()


def _oracle_flow(flow):
    from fthmc_amd.utils.layers import net_weights
    return [tuple(p.detach().cpu() for p in net_weights(layer.plaq_coupling.net)) for layer in flow]


# ---------------------------------------------------------------- parity
def test_vjps_match_the_reference_fixture():
    """tests/golden/second_order_L8.npz: the reference's own autograd through ft_force(create_graph=True) and ft_action"""
    from fthmc_amd import ops
    g = load_golden('second_order_L8')
    nl, beta = int(g['n_layers']), float(g['beta'])
    w = ops.pack_weights([[torch.as_tensor(g[f'w{li}_{pi}']) for pi in range(6)] for li in range(nl)], device='cuda')
    gw_ref = np.concatenate([g[f'gw{li}_{pi}'].reshape(-1) for li in range(nl) for pi in range(6)])
    ga_ref = np.concatenate([g[f'ga_w{li}_{pi}'].reshape(-1) for li in range(nl) for pi in range(6)])
    x = D(g['x'])
    hx, hw = ops.ft_force_vjp(x, w, nl, beta, D(g['g']))
    assert rel(hx, torch.as_tensor(g['Hg'])) < 1e-9 and rel(hw, torch.as_tensor(gw_ref)) < 1e-9
    ax, aw = ops.ft_action_vjp(x, w, nl, beta, D(g['gS']))
    assert rel(ax, torch.as_tensor(g['ga_x'])) < 1e-9 and rel(aw, torch.as_tensor(ga_ref)) < 1e-9
    assert rel(ops.ft_force(x, w, nl, beta), torch.as_tensor(g['F'])) < 1e-9


SHAPES = [  # (L, B, nl, act for the oracle, hidden, k, n_mix, final tanh)
    (8, 2, 2, 'silu', (8, 8), 3, 2, False),
    (12, 3, 2, 'relu', (8, 8), 3, 2, False),
    (16, 2, 3, 'leaky_relu', (8, 8), 3, 2, False),
    (16, 2, 4, 'leaky_relu', (8, 8), 3, 2, False),
    (8, 2, 2, 'silu', (4, 6), 5, 3, False),
    (8, 2, 2, 'silu', (8, 8), 3, 2, True),
]


@pytest.mark.parametrize('L,B,nl,act,hidden,k,n_mix,tanh', SHAPES)
def test_vjps_match_the_oracle_double_backward(L, B, nl, act, hidden, k, n_mix, tanh):
    from fthmc_amd import ops
    from oracle import ref_cpu as R
    gen = torch.Generator().manual_seed(100 * L + nl + k)
    beta = 2.5
    flow = R.default_flow(nl, gen, hidden=hidden, n_mix=n_mix, k=k)
    x, g = field(B, L, gen), torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64)
    gS, glogdet = torch.randn(B, generator=gen, dtype=torch.float64), torch.randn(B, generator=gen, dtype=torch.float64)
    (hx_r, hw_r), (ax_r, aw_r) = oracle_vjps(x, flow, beta, act + ('+tanh' if tanh else ''), g, gS, glogdet)
    w = ops.pack_weights(flow, device='cuda', final_tanh=tanh)
    hx, hw = ops.ft_force_vjp(D(x), w, nl, beta, D(g), act)
    ax, aw = ops.ft_action_vjp(D(x), w, nl, beta, D(gS), D(glogdet), act)
    errs = [rel(hx, hx_r), rel(hw, hw_r), rel(ax, ax_r), rel(aw, aw_r)]
    assert max(errs) < 1e-9, errs
    # the same bound for every layer's every parameter tensor and every chain on its own (tests/second_order_cases.py): the global
    # norm above lets a small tensor, a conv bias say, be wrong by its share of the largest
    import second_order_cases as C
    each = {}
    for what, got, ref in (('d/dw <g, F>', hw, hw_r), ('d/dw action', aw, aw_r)):
        each.update(C.per_tensor(C.split(got, flow), C.split(ref, flow), what))
    each.update(C.per_chain(hx, hx_r, 'H g'))
    each.update(C.per_chain(ax, ax_r, 'd/dx action'))
    assert C.hold(each, 1e-9, 'per tensor') < 1e-9


# ---------------------------------------------------------------- public API
def _oracle_force_loss_grads(x, oflow, beta):
    from oracle import ref_cpu as R
    fl = [tuple(t.clone().requires_grad_(True) for t in layer) for layer in oflow]
    xg = x.detach().cpu().clone().requires_grad_(True)
    F, = torch.autograd.grad(R.ft_action(xg, fl, beta).sum(), xg, create_graph=True)
    (F ** 2).mean().backward()
    return xg.grad, [t.grad for layer in fl for t in layer]


@pytest.mark.parametrize('flat', [False, True])
def test_force_loss_backward_fills_param_and_field_grads(flat):
    from fthmc_amd.config import Param, TrainConfig
    from fthmc_amd import train as T
    from fthmc_amd.utils import qed_helpers as qed
    from fthmc_amd.utils.layers import flatten_flow, net_weights
    L, B, nl, beta = 8, 3, 2, 2.0
    if flat:
        torch.manual_seed(5)
        flow = T.get_model(TrainConfig(L=L, beta=beta, n_layers=nl, batch_size=B, print_freq=0)).layers
        flatten_flow(flow)
    else:
        flow = _flow_module(L, nl)
    gen = torch.Generator().manual_seed(9)
    x = D(field(B, L, gen)).requires_grad_(True)
    param = Param(beta=beta, L=L)
    F = qed.ft_force(param, flow, x, create_graph=True)
    assert torch.equal(F.detach(), qed.ft_force(param, flow, x.detach()))
    (F ** 2).mean().backward()
    gx_r, gp_r = _oracle_force_loss_grads(x, _oracle_flow(flow), beta)
    params = [p for layer in flow for p in net_weights(layer.plaq_coupling.net)]
    assert rel(x.grad, gx_r) < 1e-9
    for p, r in zip(params, gp_r):
        assert p.grad is not None and p.grad.shape == p.shape and rel(p.grad, r) < 1e-9


def test_reference_pattern_through_ft_action_and_field_transformation():
    from fthmc_amd import ops
    from fthmc_amd.config import Param, TrainConfig, lfConfig
    from fthmc_amd import train as T
    from fthmc_amd.ft_hmc import FieldTransformation
    from fthmc_amd.utils import qed_helpers as qed
    from fthmc_amd.utils.layers import flow_weights, net_weights
    L, B, nl, beta = 8, 2, 2, 2.0
    cfg = TrainConfig(L=L, beta=beta, n_layers=nl, batch_size=B, print_freq=0)
    torch.manual_seed(12)
    flow = T.get_model(cfg).layers
    ft = FieldTransformation(flow=flow, config=cfg, lfconfig=lfConfig(tau=1.0, nstep=4))
    gen = torch.Generator().manual_seed(13)
    x0, g = D(field(B, L, gen)), D(torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64))
    params = [p for layer in flow for p in net_weights(layer.plaq_coupling.net)]
    w = flow_weights(flow, 'cuda')
    hx, hw = ops.ft_force_vjp(x0, w, nl, beta, g)
    hw = [t for row in ops.unpack_weight_grads(hw, nl) for t in row]
    for action in (lambda x: qed.ft_action(Param(beta=beta, L=L), flow, x), ft.action):
        x = x0.clone().requires_grad_(True)
        S = action(x)
        assert S.requires_grad and torch.equal(S.detach(), ops.ft_action(x0, w, nl, beta)[0])
        F, = torch.autograd.grad(S.sum(), x, create_graph=True)
        assert torch.equal(F.detach(), ops.ft_force(x0, w, nl, beta))
        gr = torch.autograd.grad((F * g).sum(), [x] + params)
        assert torch.equal(gr[0], hx) and all(torch.equal(a, b) for a, b in zip(gr[1:], hw))
        # first order in the weights: the action VJP
        gw = torch.autograd.grad(action(x).sum(), params)
        aw = ops.ft_action_vjp(x0, w, nl, beta, torch.ones(B, dtype=torch.float64, device='cuda'), need_gx=False)[1]
        assert all(torch.equal(a, b) for a, b in zip(gw, [t for row in ops.unpack_weight_grads(aw, nl) for t in row]))
    with torch.no_grad():
        assert not ft.action(x0.clone().requires_grad_(True)).requires_grad


def test_third_order_and_second_order_in_the_weights_raise():
    from fthmc_amd.config import Param
    from fthmc_amd.utils import qed_helpers as qed
    from fthmc_amd.utils.layers import net_weights
    L, B, nl, beta = 8, 2, 2, 2.0
    flow = _flow_module(L, nl)
    params = [p for layer in flow for p in net_weights(layer.plaq_coupling.net)]
    x = D(field(B, L, torch.Generator().manual_seed(4))).requires_grad_(True)
    F = qed.ft_force(Param(beta=beta, L=L), flow, x, create_graph=True)
    gx, = torch.autograd.grad((F ** 2).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(gx.sum(), x)
    S = qed.ft_action(Param(beta=beta, L=L), flow, x)
    gw = torch.autograd.grad(S.sum(), params, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(gw[0].sum(), x)


def test_ft_action_force_operator_backpropagates_through_every_output():
    import fthmc_amd.torch_ops  # noqa: F401
    from fthmc_amd import ops
    from oracle import ref_cpu as R
    L, B, nl, beta = 8, 2, 2, 2.0
    gen = torch.Generator().manual_seed(21)
    flow = R.default_flow(nl, gen)
    x, g = field(B, L, gen), torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64)
    gS, glogdet = torch.randn(B, generator=gen, dtype=torch.float64), torch.randn(B, generator=gen, dtype=torch.float64)
    w = ops.pack_weights(flow, device='cuda').requires_grad_(True)
    xg = D(x).requires_grad_(True)
    S, ld, F = torch.ops.fthmc_hip.ft_action_force(xg, w, nl, beta, 0)
    ((D(gS) * S).sum() + (D(glogdet) * ld).sum() + (D(g) * F).sum()).backward()
    (hx, hw), (ax, aw) = oracle_vjps(x, flow, beta, 'silu', g, gS, glogdet)
    assert rel(xg.grad, hx + ax) < 1e-9 and rel(w.grad, hw + aw) < 1e-9


def test_drivers_return_nothing_that_requires_grad():
    from fthmc_amd.config import Param, TrainConfig, lfConfig
    from fthmc_amd import train as T
    from fthmc_amd.ft_hmc import FieldTransformation
    from fthmc_amd.utils import qed_helpers as qed
    L, B, nl, beta = 8, 2, 2, 2.0
    cfg = TrainConfig(L=L, beta=beta, n_layers=nl, batch_size=B, print_freq=0)
    torch.manual_seed(31)
    model = T.get_model(cfg)
    assert any(p.requires_grad for p in model.layers.parameters())
    ft = FieldTransformation(flow=model.layers, config=cfg, lfconfig=lfConfig(tau=1.0, nstep=4))
    x = D(field(B, L, torch.Generator().manual_seed(32), 0.5))
    out = ft.hmc(x)
    flat = [out[0]] + [v for v in out[1].values() if torch.is_tensor(v)]
    v = torch.randn_like(x)
    flat += [ft.calc_energy(x, v)]
    param = Param(beta=beta, L=L, tau=1.0, nstep=4, ntraj=1, nrun=1)
    f1, hist = qed.ft_run(param, model.layers, x[0].clone())
    flat += [f1] + [t for t in qed.ft_hmc(param, model.layers, x[:1].clone())[2:] if torch.is_tensor(t)]
    assert not any(t.requires_grad for t in flat)


# ---------------------------------------------------------------- known answers
def _stencil(x):
    """plaquette P = x0 - x1 - x0(j+1) + x1(i+1) and its adjoint D^T on a plaquette field"""
    return x[:, 0] - x[:, 1] - torch.roll(x[:, 0], -1, 2) + torch.roll(x[:, 1], -1, 1)


def _stencil_t(p):
    return torch.stack([p - torch.roll(p, 1, 2), torch.roll(p, 1, 1) - p], 1)


def test_wilson_hessian_without_layers():
    from fthmc_amd import ops
    L, B, beta = 12, 3, 1.7
    gen = torch.Generator().manual_seed(41)
    x, g = D(field(B, L, gen)), D(torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64))
    hx, hw = ops.ft_force_vjp(x, None, 0, beta, g)
    ref = beta * _stencil_t(torch.cos(_stencil(x)) * _stencil(g))
    assert rel(hx, ref) < 1e-12 and hw.numel() == 0
    ax, _ = ops.ft_action_vjp(x, None, 0, beta, torch.full((B,), 0.5, dtype=torch.float64, device='cuda'))
    assert rel(ax, 0.5 * ops.wilson_force(x, beta)) < 1e-12
    # x = 0: the largest eigenvalue of H = beta D^T D is 8 beta (curl-curl at k = (pi, pi))
    z = torch.zeros(1, 2, 8, 8, dtype=torch.float64, device='cuda')
    v = D(torch.randn(1, 2, 8, 8, generator=gen, dtype=torch.float64))
    lam = 0.0
    for _ in range(200):
        v = v / v.norm()
        hv = ops.ft_force_vjp(z, None, 0, beta, v)[0]
        lam = float((v * hv).sum())
        v = hv
    assert abs(lam - 8 * beta) < 1e-9 * 8 * beta, lam


def test_a_few_adam_steps_on_the_force_lower_it():
    from fthmc_amd.config import Param
    from fthmc_amd.utils import qed_helpers as qed
    L, B, nl, beta = 8, 4, 2, 2.0
    flow = _flow_module(L, nl, seed=7)
    x = D(field(B, L, torch.Generator().manual_seed(8)))
    param = Param(beta=beta, L=L)
    opt = torch.optim.Adam(flow.parameters(), lr=3e-3)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = (qed.ft_force(param, flow, x, create_graph=True) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0], losses


# ---------------------------------------------------------------- full size: consistency and properties
BIG = {'config3': (128, 64, 8), 'config5_shard': (32, 256, 16)}


def _big(tag):
    from fthmc_amd import ops
    from oracle import ref_cpu as R
    B, L, nl = BIG[tag]
    gen = torch.Generator().manual_seed(B + L + nl)
    w = ops.pack_weights(R.default_flow(nl, gen), device='cuda')
    x = D(field(B, L, gen))
    return B, L, nl, 2.0, w, x, gen


@pytest.mark.parametrize('tag', list(BIG))
def test_first_order_consistency_at_full_size(tag):
    from fthmc_amd import ops
    B, L, nl, beta, w, x, gen = _big(tag)
    one = torch.ones(B, dtype=torch.float64, device='cuda')
    gx = ops.ft_action_vjp(x, w, nl, beta, one, need_gw=False)[0]
    assert rel(gx, ops.ft_force(x, w, nl, beta)) < 1e-11
    gw = ops.ft_action_vjp(x, w, nl, beta, one / B, need_gx=False)[1]
    assert rel(gw, ops.train_grad(x, w, nl, beta)['gw']) < 1e-11


@pytest.mark.parametrize('tag', list(BIG))
def test_hessian_properties_at_full_size(tag):
    from fthmc_amd import ops
    from fthmc_amd import graph_loop
    B, L, nl, beta, w, x, gen = _big(tag)
    a = D(torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64))
    b = D(torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64))
    Ha, gwa = ops.ft_force_vjp(x, w, nl, beta, a)
    Hb, _ = ops.ft_force_vjp(x, w, nl, beta, b)
    # symmetry of the Hessian
    ab, ba = float((a * Hb).sum()), float((b * Ha).sum())
    assert abs(ab - ba) < 1e-11 * max(abs(ab), float((a.abs() * Hb.abs()).sum())), (ab, ba)
    # determinism, and the workspace head (the weight expansions of the tuned calls) untouched
    ops.ft_force(x, w, nl, beta)
    key = (x.device.index, torch.cuda.current_stream().cuda_stream)
    head = int(ops._lib.load().fthmc_ws_head_bytes()) // 8
    h0 = ops._WS[key][:head].clone()
    Ha2, gwa2 = ops.ft_force_vjp(x, w, nl, beta, a)
    assert torch.equal(Ha, Ha2) and torch.equal(gwa, gwa2)
    assert torch.equal(h0, ops._WS[key][:head])
    # pure-gauge directions: S_eff is gauge invariant, H delta and d/dw <delta, F> vanish
    alpha = D(torch.randn(B, L, L, generator=gen, dtype=torch.float64))
    delta = torch.stack([alpha - torch.roll(alpha, -1, 1), alpha - torch.roll(alpha, -1, 2)], 1)
    Hd, gwd = ops.ft_force_vjp(x, w, nl, beta, delta)
    assert float(Hd.abs().max()) < 1e-10 * float(Ha.abs().max())
    assert float(gwd.abs().max()) < 1e-10 * float(gwa.abs().max())
    # central differences of the tuned first-order force
    eps = 1e-5
    fd = (ops.ft_force(x + eps * a, w, nl, beta) - ops.ft_force(x - eps * a, w, nl, beta)) / (2 * eps)
    assert rel(fd, Ha) < 1e-6
    d = D(torch.randn(w.numel(), generator=gen, dtype=torch.float64)) * 1e-1
    fw = (float((a * ops.ft_force(x, w + eps * d, nl, beta)).sum()) - float((a * ops.ft_force(x, w - eps * d, nl, beta)).sum())) / (2 * eps)
    assert abs(fw - float((gwa * d).sum())) < 1e-6 * float((gwa.abs() * d.abs()).sum())
    # chain independence: every chain's H g alone; the shards' weight terms add up
    h = B // 2
    Hs0, gws0 = ops.ft_force_vjp(x[:h].contiguous(), w, nl, beta, a[:h].contiguous())
    Hs1, gws1 = ops.ft_force_vjp(x[h:].contiguous(), w, nl, beta, a[h:].contiguous())
    assert torch.equal(torch.cat([Hs0, Hs1]), Ha)
    assert rel(gws0 + gws1, gwa) < 1e-12
    # a captured graph replays bit-equal to the eager call
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        ops.ft_force_vjp(x, w, nl, beta, a)                      # warm-up on the capturing stream (its workspace)
        gr = torch.cuda.CUDAGraph()
        with graph_loop.capture(gr, st):
            Hg_, gwg_ = ops.ft_force_vjp(x, w, nl, beta, a)
        gr.replay()
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    assert torch.equal(Hg_, Ha) and torch.equal(gwg_, gwa)
    del gr
