"""GPU: csrc/flow_generic.hip at the edges of the net shapes it accepts, on the cases of tests/net_shape_cases.py.

Every case goes through every entry point that the generic kernels serve, against the CPU oracle, on the hard inputs (weights
times 2, links pinned 1e-9 from +-pi), by the project's measure: max|got - ref| / max|ref| <= 1e-9 for every layer's every parameter
tensor and for every chain of every output (links as angle differences).  tests/test_net_shapes.py asserts on the CPU that the
oracle itself moves by at most 1e-12 per entry at these inputs, and pins the oracle's conv where its circular pad is at its limit.
Before its calls each test asserts that the packed weights carry the case's shape and that the call takes the generic kernels.
  sweeps        flow_forward, ft_action, ft_force, one ft_leapfrog step, train_grad       (first_order_cases.oracle_results)
  second order  ft_force_vjp, ft_action_vjp, train_force_grad: the Dual instances          (second_order_cases.oracle_results)
  one layer     at all eight (mu, off), a layer beyond the case's own with the weights of layer li % layers: flow_layer_fwd,
                flow_layer_bwd(need_gw=True), the stash route bit-equal to it; plaq_coupling_fwd / _bwd at (0, 0) and (1, 3)
  inverse       flow_layer_rev o flow_layer_fwd, flow_reverse o flow_forward, plaq_coupling_rev o plaq_coupling_fwd return the
                input (links 1e-9 / 1e-8, log J 1e-8 / 1e-7: those of tests/test_layer_calls_gpu.py
                test_generic_net_shapes_against_the_oracle); mix64 and uneven_mix1 are the Newton solve on 64 and on 1 component
  exact         chain b of the batch == the chain alone, a second call == the first, in place == out of place, bit for bit; for
                k9_L4 the field tiled 2 x 2 to L = 8 (there the k = 9 stencil is the un-aliased sum of the same taps) gives the
                L = 4 force and flowed field site for site, S_eff and log det times 4
  trajectory    one 4-step ft_trajectory against oracle.ref_cpu.ft_hmc(mode='md'): H0 1e-11, H1 1e-9, dH 1e-6, the same accepts

Observed on an MI355X (pytest -s prints them): per case the worst entry of the sweeps, of the second-order calls and of the
one-layer calls, beside the case's sensitivity (the oracle under a move of every input by one relative 2^-52, the worst of three
sets of signs and of all entries, first / second order: tests/test_net_shapes.py prints it).  l = layer, t = parameter tensor,
c = chain.
  case            net, L, B, layers         sweeps                 second order             one layer                sensitivity 1st / 2nd
  k9_L4           (4,) k9 m2 L4 B2 x8       1.2e-14  logp c1       4.4e-14  gw_vjp l0 t1    3.0e-15  plaq logJ c0    1.7e-14 / 1.1e-13
  k5_L4_nohidden  () k5 m2 L4 B2 x4         6.8e-14  logp c1       3.1e-15  gw_vjp l1 t0    1.7e-15  plaq logJ c1    1.1e-13 / 2.8e-14
  k15_L8          (3,) k15 m3 L8 B2 x2      2.9e-14  logdet c1     3.8e-15  gw_vjp l0 t3    3.0e-15  plaq logJ c1    8.4e-14 / 1.3e-14
  k1_L4           (8,8) k1 m2 L4 B2 x2      3.4e-15  logp c0       5.3e-15  gw_vjp l0 t0    6.7e-15  gw l6 t1        4.8e-14 / 9.0e-14
  wide256         (256,256) k3 m2 L4 B2 x1  2.8e-15  logdet c0     2.2e-15  aw l0 t5        2.8e-15  gw l3 t0        2.4e-14 / 4.3e-15
  mix64           (1,) k3 m64 L8 B2 x2      8.2e-15  logdet c1     2.3e-15  gw_vjp l1 t3    1.1e-14  gw l7 t3        4.3e-14 / 3.6e-14
  uneven_mix1     (3,17,2) k3 m1 L12 B3 x3  2.1e-15  logdet c1     9.7e-15  Hg c1           2.8e-15  gw l4 t1        1.1e-14 / 2.3e-14
  deep8           (2,)*8 k3 m2 L8 B2 x3     1.7e-14  gw l2 t5      1.6e-14  gw_force l0 t11 2.1e-14  gw l0 t7        4.7e-14 / 4.5e-14
  tanh_net        (5,) k5 m3 L8 B2 x4 tanh  1.1e-14  S_eff c1      2.0e-14  gw_force l2 t3  1.2e-15  gw l3 t3        9.8e-15 / 1.7e-14
  L20_k7          (6,) k7 m2 L20 B2 x2      1.6e-15  gw l1 t0      2.3e-14  Hg c1           3.1e-15  gw l3 t1        5.7e-15 / 9.8e-15
  L132_stride     (32,) k3 m2 L132 B2 x1    8.6e-15  gw l0 t0      1.7e-14  aw l0 t0        6.1e-14  gw l1 t0        1.2e-14 / 6.6e-14
(net: hidden widths, kernel size k, mixture components m; xN: layers.)  Every figure is four orders or more inside the bound and
at or below a few times the case's sensitivity.  The inverses returned the input to 3.2e-12 in the links (L132_stride, one layer) and
1.2e-10 in log J (L132_stride: a sum over 4356 active sites; 3.5e-12 on the others), Newton on 64 components (mix64) 6.9e-13 / 4.4e-13
and on one (uneven_mix1) 1.2e-12 / 8.8e-13; the trajectories' H0 and H1 agreed to 6e-16 relative, dH to 3.6e-12 (L132_stride).  The
tiled k9_L4 field gave the L = 4 results with no difference at all: the taps run in the same order over equal values.  No kernel
missed a bound, none was changed.  tests/test_limits_gpu.py: B = 65537 through the generic kernels and B = 2^20 through the tuned
ones ran, every chain bit-equal to the chain alone; the launches take a chain count past 65535 in gridDim.y / gridDim.z as they are.

That the bound bites, measured once on a copy of the tree that is not committed: k_gen_conv with its site loop replaced by a
single pass (`if (s < n)` in place of the `for`), so that with L^2 > 64 x 256 sites the planes' tails stay unwritten; it changes
no address.
5 of the 67 tests here fail on it, all of L132_stride, the one case whose site loop goes round twice: the sweeps (the force
off by 0.7 of its largest entry), the second-order calls (already their second, identical call differs: the tails hold what the
workspace held before), the one-layer calls (the stash route differs from the direct one), the chain alone, and the trajectory.  Its inverse test passes: forward and reverse read the same
stale planes.  tests/test_layer_calls_gpu.py test_generic_net_shapes_against_the_oracle (6 cases, L <= 20) and the hard-input suites
tests/test_first_order_hard_gpu.py and tests/test_second_order_hard_gpu.py (122 tests, generic cases at L = 8) pass it.
"""
import math

import pytest
import torch

import net_shape_cases as N
from first_order_cases import train_path
from gpu_support import D, R, module_defaults, ops

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

FC, C = N.FC, N.C
DT = FC.DT
# tests/test_net_shapes.py test_reference_is_well_conditioned_at_the_case, as printed: (first order, second order)
SENSITIVITY = {'k9_L4': (1.7e-14, 1.1e-13), 'k5_L4_nohidden': (1.1e-13, 2.8e-14), 'k15_L8': (8.4e-14, 1.3e-14),
               'k1_L4': (4.8e-14, 9.0e-14), 'wide256': (2.4e-14, 4.3e-15), 'mix64': (4.3e-14, 3.6e-14),
               'uneven_mix1': (1.1e-14, 2.3e-14), 'deep8': (4.7e-14, 4.5e-14), 'tanh_net': (9.8e-15, 1.7e-14),
               'L20_k7': (5.7e-15, 9.8e-15), 'L132_stride': (1.2e-14, 6.6e-14)}


def weights(case, layers=None):
    """the case's packed weights (of the listed layers), after asserting that they carry its shape and select the generic kernels"""
    inp = N.inputs(case)
    w = ops.pack_weights(inp.flow if layers is None else [inp.flow[li] for li in layers], device='cuda', final_tanh=case.tanh)
    assert ops.arch_of(w) == N.arch(case) != ops.DEFAULT_ARCH
    assert w.numel() == (case.nl if layers is None else len(layers)) * ops.arch_params(N.arch(case))
    assert train_path(case, 'mfma') == 'generic' and ops.train_force_path(case.B, case.L, N.arch(case)) == 0
    return w


def show(case, what, errs):
    s1, s2 = SENSITIVITY[case.name]
    print(f'{case.name} {what}: worst %.1e (%s)' % FC.worst(errs)[::-1], f'; sensitivity {s1:.1e} / {s2:.1e}')
    FC.hold(errs, N.BOUND, f'{case.name} {what}')


def angle_err(a, b):
    return float(R.wrap(a.detach().cpu() - b.detach().cpu()).abs().max())


@pytest.mark.parametrize('case', N.CASES, ids=N.IDS)
def test_sweeps_per_chain_and_per_tensor(case):
    """flow_forward, ft_action, ft_force, one ft_leapfrog step and train_grad; the force and the training gradient twice, the
    same bits; the input untouched"""
    inp, ref = N.inputs(case), N.first_order(case)
    w, x, nl, act = weights(case), D(inp.x), case.nl, case.act
    y, ld = ops.flow_forward(x, w, nl, act)
    S, ld2 = ops.ft_action(x, w, nl, N.BETA, act)[:2]
    F = ops.ft_force(x, w, nl, N.BETA, act)
    lf_x, lf_v = ops.ft_leapfrog(x, D(inp.g), w, nl, N.BETA, DT, 1, act)
    r = ops.train_grad(x, w, nl, N.BETA, act)
    r2 = ops.train_grad(x, w, nl, N.BETA, act)
    assert torch.equal(ops.ft_force(x, w, nl, N.BETA, act), F)
    assert all(torch.equal(r[k], r2[k]) for k in ('gw', 'logq', 'logp', 'x'))
    assert torch.equal(x, D(inp.x))
    errs = FC.compare({'y': y, 'logdet': ld, 'S_eff': S, 'F': F, 'lf_x': lf_x, 'lf_v': lf_v, 'gw': r['gw'], 'logq': r['logq'],
                       'logp': r['logp']}, ref, inp.flow)
    errs.update({f'{k} (ft_action)': v for k, v in FC.compare({'logdet': ld2}, ref, inp.flow).items()})
    errs.update({f'{k} (train_grad)': v for k, v in FC.compare({'y': r['x']}, ref, inp.flow).items()})
    assert len(errs) == 10 * case.B + 2 * (len(case.arch[0]) + 1) * nl
    show(case, 'sweeps', errs)


@pytest.mark.parametrize('case', N.CASES, ids=N.IDS)
def test_second_order_per_chain_and_per_tensor(case):
    """ft_force_vjp, ft_action_vjp and train_force_grad (the Dual instances of the generic kernels); twice, the same bits"""
    inp, ref = N.inputs(case), N.second_order(case)
    w, x, nl, act = weights(case), D(inp.x), case.nl, case.act
    assert ops.vjp_ws_bytes(case.B, case.L, nl, N.arch(case)) > 0

    def calls():
        hx, hw = ops.ft_force_vjp(x, w, nl, N.BETA, D(inp.g), act)
        ax, aw = ops.ft_action_vjp(x, w, nl, N.BETA, D(inp.gS), D(inp.glogdet), act)
        f = ops.train_force_grad(x, w, nl, N.BETA, act)
        return {'Hg': hx, 'gw_vjp': hw, 'ax': ax, 'aw': aw, 'F': f['F'], 'force_sq': f['force_sq'], 'gw_force': f['gw']}
    got, again = calls(), calls()
    assert all(torch.equal(got[k], again[k]) for k in got)
    errs = C.compare(got, ref, inp.flow)
    assert len(errs) == 4 * case.B + 3 * 2 * (len(case.arch[0]) + 1) * nl
    show(case, 'second order', errs)


@pytest.mark.parametrize('case', N.CASES, ids=N.IDS)
def test_one_layer_at_every_stripe(case):
    """every (mu, off): the layer's links and log J, its link gradient per chain and its weight gradient per tensor; the stash
    route and the in-place forward return the same bits; the plaquette-level map and its VJP at (0, 0) and (1, 3)"""
    from fthmc_amd import _lib
    inp, ref = N.inputs(case), N.layers_at_every_stripe(case)
    flow8 = N.eight_layers(inp).flow
    x, c, dlog, act = D(inp.x), D(inp.g), D(inp.gS), case.act
    got = {'layer_y': [], 'layer_logJ': [], 'layer_gx': [], 'layer_gw': []}
    for li, (mu, off) in enumerate(N.MU_OFF):
        wl = weights(case, [li % case.nl])
        y, logJ = ops.flow_layer_fwd(x, wl, mu, off, act)
        gx, gw = ops.flow_layer_bwd(x, wl, c, dlog, mu, off, act, need_gw=True)
        ys, logJs, stash = ops.flow_layer_fwd_stash(x, wl, mu, off, act)
        assert stash is not None and stash.numel() * 8 == _lib.load().fthmc_layer_stash_bytes(ops._arch(N.arch(case)), case.B, case.L)
        gxs, gws = ops.flow_layer_bwd_stash(stash, tuple(x.shape), wl, c, dlog, mu, off, act, need_gw=True)
        assert torch.equal(ys, y) and torch.equal(logJs, logJ) and torch.equal(gxs, gx) and torch.equal(gws, gw), (case.name, li)
        xi = x.clone()
        yi, logJi = ops.flow_layer_fwd(xi, wl, mu, off, act, inplace=True)
        assert yi.data_ptr() == xi.data_ptr() and torch.equal(xi, y) and torch.equal(logJi, logJ), (case.name, li)
        for k, v in zip(('layer_y', 'layer_logJ', 'layer_gx', 'layer_gw'), (y, logJ, gx, gw)):
            got[k].append(v)
    assert torch.equal(x, D(inp.x))
    errs = FC.compare(got, ref, flow8)
    assert len(errs) == 8 * 2 * (len(case.arch[0]) + 1) + 2 * 8 * case.B + case.B
    # the plaquette-level map on the plaquettes of the pinned links, gfP = g[:, 0], glogJ = gS
    P, gfP = R.plaq(inp.x), inp.g[:, 0].contiguous()
    pl = {'fP': [], 'logJ': [], 'gP': [], 'gw': []}
    pr = {'fP': [], 'logJ': [], 'gP': [], 'gw': []}
    for li in (0, 7):
        mu, off = N.MU_OFF[li]
        wl = weights(case, [li % case.nl])
        fP, lj = ops.plaq_coupling_fwd(D(P), wl, mu, off, act)
        gP, gw = ops.plaq_coupling_bwd(D(P), wl, D(gfP), dlog, mu, off, act, need_gw=True)
        Pg = P.clone().requires_grad_(True)
        wg = tuple(t.detach().clone().requires_grad_(True) for t in flow8[li])
        fPc, ljc = R.plaq_coupling_forward(Pg, wg, mu, off, inp.act)
        g = torch.autograd.grad((fPc * gfP).sum() + (ljc * inp.gS).sum(), [Pg] + list(wg))
        for k, a, b in zip(('fP', 'logJ', 'gP', 'gw'), (fP, lj, gP, gw), (fPc.detach(), ljc.detach(), g[0], tuple(g[1:]))):
            pl[k].append(a)
            pr[k].append(b)
    assert (N.MU_OFF[0], N.MU_OFF[7]) == ((0, 0), (1, 3))
    for i, li in enumerate((0, 7)):
        errs.update(FC.per_chain_angle(pl['fP'][i], pr['fP'][i], f'plaq fP {li}'))
        errs.update(FC.per_chain(pl['gP'][i], pr['gP'][i], f'plaq gP {li}'))
    errs.update(FC.per_chain(torch.stack([t.cpu() for t in pl['logJ']], 1), torch.stack(pr['logJ'], 1), 'plaq logJ'))
    errs.update(FC.per_tensor(C.split(torch.stack(pl['gw']), [flow8[0], flow8[7]]), pr['gw'], 'plaq gw'))
    show(case, 'one layer', errs)


@pytest.mark.parametrize('case', N.CASES, ids=N.IDS)
def test_inverses_return_the_input(case):
    """flow_layer_rev o flow_layer_fwd at every (mu, off), flow_reverse o flow_forward, plaq_coupling_rev o plaq_coupling_fwd"""
    inp = N.inputs(case)
    x, act, nl = D(inp.x), case.act, case.nl
    worst = {'layer x': 0.0, 'layer logJ': 0.0, 'plaq P': 0.0, 'plaq logJ': 0.0}
    for li, (mu, off) in enumerate(N.MU_OFF):
        wl = weights(case, [li % nl])
        y, lj = ops.flow_layer_fwd(x, wl, mu, off, act)
        xb, ljb = ops.flow_layer_rev(y, wl, mu, off, act)
        worst['layer x'] = max(worst['layer x'], angle_err(xb, x))
        worst['layer logJ'] = max(worst['layer logJ'], float((ljb + lj).abs().max()))
        if li in (0, 7):
            P = D(R.plaq(inp.x))
            fP, pj = ops.plaq_coupling_fwd(P, wl, mu, off, act)
            Pb, pjb = ops.plaq_coupling_rev(fP, wl, mu, off, act)
            worst['plaq P'] = max(worst['plaq P'], angle_err(Pb, P))
            worst['plaq logJ'] = max(worst['plaq logJ'], float((pjb + pj).abs().max()))
    w = weights(case)
    y, ld = ops.flow_forward(x, w, nl, act)
    xb, ldb = ops.flow_reverse(y, w, nl, act)
    worst['flow x'], worst['flow logdet'] = angle_err(xb, x), float((ldb + ld).abs().max())
    print(f'{case.name} inverse:', ', '.join(f'{k} {v:.1e}' for k, v in worst.items()))
    assert worst['layer x'] < 1e-9 and worst['layer logJ'] <= 1e-8, worst
    assert worst['plaq P'] < 1e-9 and worst['plaq logJ'] <= 1e-8, worst
    assert worst['flow x'] < 1e-8 and worst['flow logdet'] <= 1e-7, worst


@pytest.mark.parametrize('case', N.CASES, ids=N.IDS)
def test_a_chain_of_the_batch_is_the_chain_alone(case):
    """every chain's results do not depend on the chains beside it, bit for bit: the sweeps, a layer, the Hessian product"""
    inp = N.inputs(case)
    w, w0, x, g, nl, act = weights(case), weights(case, [0]), D(inp.x), D(inp.g), case.nl, case.act
    full = (*ops.flow_forward(x, w, nl, act), *ops.ft_action(x, w, nl, N.BETA, act), ops.ft_force(x, w, nl, N.BETA, act),
            *ops.flow_layer_fwd(x, w0, 1, 3, act), ops.ft_force_vjp(x, w, nl, N.BETA, g, act, need_gw=False)[0],
            ops.train_force_grad(x, w, nl, N.BETA, act, need_gw=False)['force_sq'])
    for b in range(case.B):
        xb, gb = x[b:b + 1].contiguous(), g[b:b + 1].contiguous()
        one = (*ops.flow_forward(xb, w, nl, act), *ops.ft_action(xb, w, nl, N.BETA, act), ops.ft_force(xb, w, nl, N.BETA, act),
               *ops.flow_layer_fwd(xb, w0, 1, 3, act), ops.ft_force_vjp(xb, w, nl, N.BETA, gb, act, need_gw=False)[0],
               ops.train_force_grad(xb, w, nl, N.BETA, act, need_gw=False)['force_sq'])
        assert len(one) == len(full) == 11
        for i, (a, f) in enumerate(zip(one, full)):
            assert torch.equal(a, f[b:b + 1]), (case.name, b, i)


def test_k9_on_L4_is_the_same_stencil_unaliased_on_L8():
    """k9_L4 tiled 2 x 2 to L = 8 with the same weights: on L = 8 the nine taps of a kernel row land on nine sites (one wraps),
    on L = 4 on four; the field has period 4, so every site sees the same sum in another order.  The flowed field and the force
    site for site to the bound, S_eff and log det times 4."""
    case = N.BY_NAME['k9_L4']
    inp = N.inputs(case)
    w, x, nl, act = weights(case), D(inp.x), case.nl, case.act
    x8 = x.repeat(1, 1, 2, 2)
    assert case.arch[1] // 2 == case.L and case.arch[1] // 2 < 8 < case.arch[1]
    y, ld = ops.flow_forward(x, w, nl, act)
    S = ops.ft_action(x, w, nl, N.BETA, act)[0]
    F = ops.ft_force(x, w, nl, N.BETA, act)
    y8, ld8 = ops.flow_forward(x8, w, nl, act)
    S8 = ops.ft_action(x8, w, nl, N.BETA, act)[0]
    F8 = ops.ft_force(x8, w, nl, N.BETA, act)
    errs = FC.per_chain_angle(y8, y.repeat(1, 1, 2, 2), 'y')
    errs.update(FC.per_chain(F8, F.repeat(1, 1, 2, 2), 'F'))
    errs.update(FC.per_chain(ld8, 4 * ld, 'logdet'))
    errs.update(FC.per_chain(S8, 4 * S, 'S_eff'))
    show(case, 'tiled to L = 8', errs)


@pytest.mark.parametrize('case', N.CASES, ids=N.IDS)
def test_trajectory_against_the_oracle(case):
    """one 4-step MD trajectory from the case's links with v = g"""
    inp = N.inputs(case)
    w, nl, act = weights(case), case.nl, case.act
    u = torch.rand(case.B, generator=torch.Generator().manual_seed(N.seed(case) + 1), dtype=torch.float64)
    r = ops.ft_trajectory(D(inp.x), D(inp.g), D(u), w, nl, N.BETA, DT, 4, act)
    dH, _, acc, newx, h0, h1 = R.ft_hmc(inp.x, inp.g, u, inp.flow, N.BETA, DT, 4, act=inp.act, mode='md')
    rel = lambda a, b: float(((a.cpu() - b).abs() / b.abs()).max())
    print(f'{case.name} trajectory: H0 {rel(r["H0"], h0):.1e}, H1 {rel(r["H1"], h1):.1e}, dH {float((r["dH"].cpu() - dH).abs().max()):.1e}')
    torch.testing.assert_close(r['H0'].cpu(), h0, rtol=1e-11, atol=1e-10)
    torch.testing.assert_close(r['H1'].cpu(), h1, rtol=1e-9, atol=1e-10)
    torch.testing.assert_close(r['dH'].cpu(), dH, rtol=1e-6, atol=1e-7)
    assert torch.equal(r['acc'].cpu() > 0.5, acc)
    assert angle_err(r['x_new'], newx) < 1e-8
    assert math.isfinite(float(r['dH'].abs().max()))
