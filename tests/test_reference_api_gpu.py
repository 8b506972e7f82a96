"""GPU tests of callers written against the reference's Python API: the physical-field ftHMC wrapper, the independence sampler
and the plaquette-level coupling layer on goldens of the reference, the `fthmc.*` import path, other net shapes through the
reference-shaped modules, FieldTransformation.run's carried state, the delta-Q^2 tooling on HIP-produced histories, and the sampler
at an operating point with a flow trained by the reference-shaped loop."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from gpu_support import D, H, R, angle_close, close, module_defaults, ops, switches

pytestmark = pytest.mark.gpu
_defaults = module_defaults()


def build_layers(g, L, act='silu'):
    from fthmc_amd.utils import layers as Lyr
    nl = int(g['n_layers'])
    flow = Lyr.make_u1_equiv_layers(n_layers=nl, n_mixture_comps=2, lattice_shape=(L, L), hidden_sizes=[8, 8],
                                    kernel_size=3, activation_fn=act)
    names = ['net.0.weight', 'net.0.bias', 'net.2.weight', 'net.2.bias', 'net.4.weight', 'net.4.bias']
    flow.load_state_dict({f'{li}.plaq_coupling.{n}': D(g[f'w{li}_{pi}']) for li in range(nl) for pi, n in enumerate(names)})
    return flow


# ---------------------------------------------------------------- f1: ft_hmc on the physical field
@pytest.mark.parametrize('L', [8, 16])
def test_physical_field_fthmc_golden(L):
    """qed_helpers.ft_hmc (ipynb/ft_hmc.py:420-435) against the reference run with captured v, u.
    'tight' golden (reference bisection down to fp resolution): the HIP inverse (Newton to 1e-12) agrees to
    rounding amplified by the trajectory; 'ref' golden (the reference's 1e-6 inverse tolerance): agreement
    within what that tolerance allows."""
    from fthmc_amd.config import Param
    from fthmc_amd.utils import qed_helpers as qed
    for tag, tol_dH, tol_f in (('tight', 1e-7, 1e-7), ('ref', 5e-3, 5e-5)):
        g = load_golden(f'fthmc_phys_L{L}_{tag}')
        flow = build_layers(g, L)
        param = Param(beta=float(g['beta']), L=L, tau=float(g['dt']) * int(g['nstep']), nstep=int(g['nstep']))
        field = D(g['field'])
        angle_close(qed.ft_flow_inv(flow, field), g['x_inv'], atol=1e-9 if tag == 'tight' else 2e-6)
        dH, e, acc, newfield = qed.ft_hmc(param, flow, field, v=D(g['v']), u=D(g['u']))
        g_dH, g_e, g_u = (float(np.asarray(g[k]).reshape(-1)[0]) for k in ('dH', 'exp_mdH', 'u'))
        assert abs(dH - g_dH) < tol_dH * max(1.0, abs(g_dH)), (tag, dH, g_dH)
        assert abs(e - g_e) < 10 * tol_dH * max(1.0, g_e)
        if abs(g_u - g_e) > 1e-2:
            assert bool(acc) == bool(g['acc'])
            angle_close(newfield, g['newfield'], atol=tol_f)
        assert newfield.shape == field.shape
    # a configuration [2, L, L] (what ft_run passes around) and the run loop
    param.nrun, param.ntraj = 1, 3
    f1, hist = qed.ft_run(param, flow, field[0])
    assert f1.shape == field[0].shape and len(hist['dH']) == 3 and all(np.isfinite(hist['plaq']))
    assert all(abs(q - round(q)) < 1e-8 for q in hist['topo'])
    big = qed.flow_resize(flow, (2 * L, 2 * L))
    assert len(big) == len(flow) and big[0].plaq_coupling.net is flow[0].plaq_coupling.net


# ---------------------------------------------------------------- f3: independence sampler
def test_independence_sampler_golden():
    """utils.samplers.make_mcmc_ensemble against the recorded reference chain (samplers.py:182-259): same
    proposals + same uniforms -> identical accept sequence and histories; and the GPU proposal generator
    reproduces the reference's proposals (flowed sample, logq, both logp flavours)."""
    from fthmc_amd.utils import qed_helpers as qed
    from fthmc_amd.utils import samplers as S
    from fthmc_amd.utils.distributions import MultivariateUniform
    g = load_golden('sampler_L8')
    L, beta, bs = 8, float(g['beta']), int(g['batch_size'])
    layers = build_layers(g, L)
    xi = D(g['xi'])
    n = xi.shape[0]
    action = qed.BatchAction(beta)

    class FixedPrior(MultivariateUniform):
        """the reference's prior, replaying the recorded draws"""
        def __init__(self):
            super().__init__(-math.pi * torch.ones(2, L, L, dtype=torch.float64, device='cuda'),
                             math.pi * torch.ones(L, L, dtype=torch.float64, device='cuda'))
            self.k = 0

        def sample_n(self, b):
            out = xi[self.k:self.k + b]
            self.k += b
            return out
    for literal, kx, kp in ((True, 'xi', 'logp_xi'), (False, 'xflow', 'logp_flow')):
        model = {'layers': layers, 'prior': FixedPrior()}
        props = list(S.serial_sample_generator(model, action, bs, n, reference_literal=literal))
        angle_close(torch.stack([p[0] for p in props]), g[kx], atol=1e-10)
        close(torch.stack([p[1] for p in props]), g['logq'], rtol=1e-11)
        close(torch.stack([p[2] for p in props]), g[kp], rtol=1e-11)
    model = {'layers': layers, 'prior': FixedPrior()}
    h = S.make_mcmc_ensemble(model, action, bs, n, uniforms=list(g['u']), reference_literal=True)
    assert np.array_equal(h['acc'], g['hist_acc'])
    for k in ('q', 'dqsq', 'logq', 'logp'):
        close(h[k], g['hist_' + k], rtol=2e-7, atol=1e-6)          # the reference's histories are float32


# ---------------------------------------------------------------- plaquette-level coupling map
@pytest.mark.parametrize('L,B', [(8, 2), (20, 3), (64, 4)])
def test_plaq_coupling_layer(L, B):
    """NCPPlaqCouplingLayer.forward / .reverse (layers.py:348-396) on plaquette fields vs the oracle."""
    from fthmc_amd.utils import layers as Lyr
    gen = torch.Generator().manual_seed(90 + L)
    flow = R.default_flow(8, gen)
    P = (torch.rand(B, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi
    for li, wts in enumerate(flow):
        mu, off = li % 2, (li // 2) % 4
        w = ops.pack_weights([wts], device='cuda')
        fP, lj = ops.plaq_coupling_fwd(P.cuda(), w, mu, off)
        fPc, ljc = R.plaq_coupling_forward(P, wts, mu, off)
        angle_close(fP, fPc, atol=1e-11); close(lj, ljc, rtol=1e-11, atol=1e-11)
        Pb, ljb = ops.plaq_coupling_rev(fP, w, mu, off, tol=1e-13)
        angle_close(Pb, P, atol=1e-9); close(ljb, -lj, atol=1e-8)
        Pc, ljc2 = R.plaq_coupling_reverse(fPc, wts, mu, off, tol=1e-13)
        close(ljb, ljc2, atol=1e-7)
    # through the layer classes
    layers = Lyr.make_u1_equiv_layers(n_layers=2, n_mixture_comps=2, lattice_shape=(L, L), hidden_sizes=[8, 8], kernel_size=3)
    pc = layers[1].plaq_coupling
    fx, lj = pc.forward(P.cuda())
    xb, ljb = pc.reverse(fx)
    angle_close(xb, P, atol=1e-9); close(ljb, -lj, atol=1e-8)
    with switches(variant=0):
        with pytest.raises(Exception, match='unsupported'):
            ops.plaq_coupling_fwd(P.cuda(), w, 0, 0)


# ---------------------------------------------------------------- the reference's import path
def test_reference_style_caller_through_fthmc_alias():
    """What a user of nftqcd/fthmc writes (fthmc/main.py:73-104, fthmc/train.py:162-228), imports unchanged."""
    from fthmc.config import FlowModel, TrainConfig, lfConfig
    from fthmc.ft_hmc import FieldTransformation
    from fthmc.train import train_step
    import fthmc.utils.layers as layers
    import fthmc.utils.qed_helpers as qed
    from fthmc.utils.distributions import MultivariateUniform

    def build(g, L):
        nl = int(g['n_layers'])
        flow = layers.make_u1_equiv_layers(n_layers=nl, n_mixture_comps=2, lattice_shape=(L, L), hidden_sizes=[8, 8],
                                           kernel_size=3, activation_fn='silu')
        names = ['net.0.weight', 'net.0.bias', 'net.2.weight', 'net.2.bias', 'net.4.weight', 'net.4.bias']
        flow.load_state_dict({f'{li}.plaq_coupling.{n}': D(g[f'w{li}_{pi}']) for li in range(nl) for pi, n in enumerate(names)})
        return flow
    # run_fthmc's body: FieldTransformation(flow=..., config=..., lfconfig=...) then trajectories
    g = load_golden('traj_md_L16')
    flow = build(g, 16)
    config = TrainConfig(L=16, beta=float(g['beta']), n_layers=len(flow))
    lfconfig = lfConfig(tau=float(g['dt']) * int(g['nstep']), nstep=int(g['nstep']))
    ft = FieldTransformation(flow=flow, config=config, lfconfig=lfconfig)
    xnew, m = ft._batch_hmc(D(g['x']), v=D(g['v']), u=D(g['u']))
    close(m['dh'], g['dH'], rtol=1e-6, atol=1e-6)
    assert np.array_equal(H(m['acc']) > 0.5, g['acc'])
    close(qed.ft_action(config, flow, D(g['x'])) + 0.5 * (D(g['v']) ** 2).flatten(1).sum(1), g['H0'], rtol=1e-10)
    # train_step on the golden prior draw
    g = load_golden('train_L8')
    flow = build(g, 8)
    B = g['xi'].shape[0]
    cfg = TrainConfig(L=8, beta=float(g['beta']), n_layers=len(flow), batch_size=B, base_lr=float(g['lr']))
    prior = MultivariateUniform(-math.pi * torch.ones(2, 8, 8, dtype=torch.float64, device='cuda'),
                                math.pi * torch.ones(8, 8, dtype=torch.float64, device='cuda'))
    model = FlowModel(prior=prior, layers=flow)
    opt = torch.optim.Adam(flow.parameters(), lr=cfg.base_lr)
    met = train_step(model, cfg, qed.BatchAction(float(g['beta'])), opt, B, xi=D(g['xi']))
    close(met['loss_dkl'], g['loss_dkl'], rtol=1e-10); close(met['ess'], g['ess'], rtol=1e-8)


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_net_shapes_golden_through_the_reference_api(tag):
    """The same through the reference-shaped Python API on goldens of the reference itself: make_u1_equiv_layers with
    other hidden_sizes / kernel_size / n_mixture_comps, qed.ft_flow / ft_action / ft_force, train_step."""
    from fthmc.config import FlowModel, Param, TrainConfig
    from fthmc.train import get_model, train_step
    import fthmc.utils.layers as layers
    import fthmc.utils.qed_helpers as qed
    g = load_golden(f'netshape_{tag}')
    hidden, k, n_mix, act, beta = [int(h) for h in g['hidden']], int(g['kernel_size']), int(g['n_mix']), str(g['act']), float(g['beta'])
    L, nl = g['x'].shape[-1], int(g['n_layers'])

    def load(flow, prefix):
        sd = {}
        for li in range(nl):
            for pi in range(2 * (len(hidden) + 1)):
                sd[f'{li}.plaq_coupling.net.{2 * (pi // 2)}.{"weight" if pi % 2 == 0 else "bias"}'] = D(g[f'{prefix}{li}_{pi}'])
        flow.load_state_dict(sd)                              # the reference's state_dict keys: Conv2d at even indices
    flow = layers.make_u1_equiv_layers(n_layers=nl, n_mixture_comps=n_mix, lattice_shape=(L, L), hidden_sizes=hidden,
                                       kernel_size=k, activation_fn=act)
    load(flow, 'w')
    param = Param(beta=beta, L=L)
    x = D(g['x'])
    angle_close(qed.ft_flow(flow, x), g['y'], atol=1e-10)
    close(qed.ft_action(param, flow, x), g['S_eff'], rtol=1e-11, atol=1e-10)
    close(qed.ft_force(param, flow, x), g['ft_force'], rtol=1e-8, atol=1e-10)
    xb = qed.ft_flow_inv(flow, D(g['y']))
    angle_close(xb, g['x'], atol=1e-8)
    B = g['xi'].shape[0]
    tc = TrainConfig(L=L, beta=beta, n_layers=nl, batch_size=B, base_lr=1e-3, hidden_sizes=hidden, kernel_size=k, n_s_nets=n_mix,
                     activation_fn=act)
    model = get_model(tc)
    load(model.layers, 'tw')
    for fused in (True, False):
        opt = torch.optim.SGD(model.layers.parameters(), lr=0.0)
        opt.zero_grad(set_to_none=True)
        met = train_step(model, tc, qed.BatchAction(beta), opt, B, xi=D(g['xi']), fused=fused)
        close(met['loss_dkl'], g['loss_dkl'], rtol=1e-10); close(met['ess'], g['ess'], rtol=1e-8)
        for li in range(nl):
            for pi, p in enumerate(model.layers[li].parameters()):
                close(p.grad, g[f'tgw{li}_{pi}'], rtol=1e-8, atol=1e-11)


# ---------------------------------------------------------------- the sampler at an operating point with a TRAINED flow
def test_sampler_is_exact_with_a_trained_flow():
    """bench.py times a random-init flow (the workload prescribes it).  Here the flow is trained with the reference-shaped
    loop (train -> train_step -> fthmc_train_grad) until the MD visibly changes, and ftHMC must still be an exact sampler:
    <exp(-dH)> = 1 and <cos P> of the flowed field = I1(beta) / I0(beta) (config.PLAQ_EXACT; finite-volume correction
    (I1/I0)^64 ~ 1e-10), errors from the 256 independent chains.  The trained weights (larger than any initialisation)
    also go through force and action against the oracle."""
    from fthmc_amd import parallel
    from fthmc_amd.config import PLAQ_EXACT, TrainConfig
    from fthmc_amd.train import get_model, train
    from fthmc_amd.utils.layers import net_weights
    L, beta, nl, B, nstep, therm, ntraj = 8, 2.0, 8, 256, 40, 60, 60
    torch.manual_seed(1331)
    cfg = TrainConfig(L=L, beta=beta, n_layers=nl, batch_size=512, n_era=1, n_epoch=600, base_lr=1e-3, print_freq=0)
    model = get_model(cfg)
    w0 = ops.pack_weights([net_weights(l.plaq_coupling.net) for l in model.layers], device='cuda')
    hist = train(cfg, model=model, verbose=False, save=False)['history']
    ess = [float(e) for e in hist['ess']]
    assert np.mean(ess[-30:]) > 2 * np.mean(ess[:30]), (np.mean(ess[:30]), np.mean(ess[-30:]))     # it did train
    layers = [net_weights(l.plaq_coupling.net) for l in model.layers]
    w = ops.pack_weights(layers, device='cuda')
    assert float((w - w0).abs().max()) > 0.05

    # trained weights against the oracle
    flow_cpu = [[p.detach().cpu() for p in lw] for lw in layers]
    xs = ((torch.rand(2, 2, L, L, generator=torch.Generator().manual_seed(4), dtype=torch.float64) * 2 - 1) * math.pi)
    S = ops.ft_action(xs.cuda(), w, nl, beta)[0]
    close(S, R.ft_action(xs, flow_cpu, beta), rtol=1e-10)
    close(ops.ft_force(xs.cuda(), w, nl, beta), R.ft_force(xs, flow_cpu, beta), rtol=1e-8, atol=1e-8)

    def run(w_, nst):
        g0, _ = ops.random_momenta(parallel.chain_seeds(7, 0, B, 0).cuda(), (B, 2, L, L), need_u=False)
        x = (0.1 * torch.erf(g0 / math.sqrt(2.0))).contiguous()
        acc = torch.zeros(B, dtype=torch.float64, device='cuda'); em = torch.zeros_like(acc); pl = torch.zeros_like(acc)
        for it in range(therm + ntraj):
            v, u = ops.random_momenta(parallel.chain_seeds(11, 0, B, it).cuda(), (B, 2, L, L))
            r = ops.ft_trajectory(x, v, u, w_, nl, beta, 1.0 / nst, nst)
            x = r['x_new']
            if it >= therm:
                acc += r['acc']; em += torch.exp(-r['dH']); pl += r['plaq']
        stat = lambda t: (float((t / ntraj).mean()), float((t / ntraj).std() / math.sqrt(B)))
        return stat(acc), stat(em), stat(pl)
    a0, _, _ = run(w0, 10)
    a1, _, _ = run(w, 10)
    assert a0[0] > 0.9 and a1[0] < 0.5, (a0, a1)          # the trained map stiffens the MD at the untrained step size ...
    acc, em, pl = run(w, nstep)
    assert acc[0] > 0.6, acc                               # ... and a finer step restores the acceptance
    assert abs(em[0] - 1.0) < 5 * em[1] and em[1] < 0.1, em
    assert abs(pl[0] - PLAQ_EXACT[beta]) < 5 * pl[1] and pl[1] < 2e-3, (pl, PLAQ_EXACT[beta])


@pytest.mark.parametrize('L,nl,B', [(8, 2, 6), (32, 2, 4)])
def test_reference_shaped_run_carries_state_and_observables(L, nl, B):
    """FieldTransformation.run(batch=True) (ft_hmc.py:272-346): the trajectory hands (S_eff, plaq, Q) of the accepted field to the
    next one and its plaq / Q to the history -- no H0 sweep, no extra flow sweep for the metrics -- and the history equals the one of
    the loop that recomputes both, as the reference does (ft_hmc.py:205, 266-270), on the same momenta and uniforms."""
    from fthmc_amd import train as T
    from fthmc_amd.config import TrainConfig, lfConfig
    from fthmc_amd.ft_hmc import FieldTransformation
    cfg = TrainConfig(L=L, beta=2.0, n_layers=nl, batch_size=B, print_freq=0)
    torch.manual_seed(11)
    model = T.get_model(cfg)
    x0 = (0.3 * (2 * torch.rand(B, 2, L, L, dtype=torch.float64) - 1)).cuda()
    n = 4
    ft = FieldTransformation(flow=model.layers, config=cfg, lfconfig=lfConfig(tau=1.0, nstep=8))
    torch.manual_seed(5); torch.cuda.manual_seed(5)
    h = ft.run(x0.clone(), nprint=0, num_trajs=n, batch=True)
    assert ft._carry is not None and ft._carry[0] is ft.x_last
    ft2 = FieldTransformation(flow=model.layers, config=cfg, lfconfig=lfConfig(tau=1.0, nstep=8))
    torch.manual_seed(5); torch.cuda.manual_seed(5)
    x = x0.clone()
    qold = ft2.lattice_metrics(ft2.flow_forward(x)[0], torch.zeros(B, dtype=torch.float64, device='cuda'))['q']
    for i in range(n):
        x, m = ft2._batch_hmc(x.clone(), step=i)                         # a copy: nothing is carried over
        lm = ft2.lattice_metrics(ft2.flow_forward(x)[0], qold)
        assert torch.equal(m['acc'], h['acc'][i])
        assert torch.allclose(m['dh'], h['dh'][i], rtol=0, atol=1e-9)
        assert torch.allclose(lm['plaq'], h['plaq'][i], rtol=1e-13, atol=0)
        assert torch.allclose(lm['q'], h['q'][i], rtol=0, atol=1e-11)
        assert torch.allclose(lm['dq'], h['dq'][i], rtol=0, atol=1e-11)
        qold = lm['q']
    assert torch.equal(x, ft.x_last)


def test_reference_shaped_single_chain_run_carries_state():
    """FieldTransformation.run() on the reference's [1, 2, L, L] field: same carry as the batch loop; the history equals the loop
    that recomputes H0 and flows the field again for its metrics."""
    from fthmc_amd import train as T
    from fthmc_amd.config import TrainConfig, lfConfig
    from fthmc_amd.ft_hmc import FieldTransformation
    L, nl, n = 8, 2, 5
    cfg = TrainConfig(L=L, beta=2.0, n_layers=nl, batch_size=1, print_freq=0)
    torch.manual_seed(13)
    model = T.get_model(cfg)
    x0 = (0.3 * (2 * torch.rand(1, 2, L, L, dtype=torch.float64) - 1)).cuda()
    ft = FieldTransformation(flow=model.layers, config=cfg, lfconfig=lfConfig(tau=1.0, nstep=8))
    torch.manual_seed(6); torch.cuda.manual_seed(6)
    h = ft.run(x0.clone(), nprint=0, num_trajs=n)
    ft2 = FieldTransformation(flow=model.layers, config=cfg, lfconfig=lfConfig(tau=1.0, nstep=8))
    torch.manual_seed(6); torch.cuda.manual_seed(6)
    x = x0.clone()
    for i in range(n):
        x, m = ft2.hmc(x.clone(), step=i)
        lm = ft2.lattice_metrics(ft2.flow_forward(x)[0], torch.zeros(1, dtype=torch.float64, device='cuda'))
        assert bool(m['acc']) == bool(h['acc'][i])
        assert torch.allclose(m['dh'], h['dh'][i], rtol=0, atol=1e-9)
        assert torch.allclose(lm['plaq'], h['plaq'][i], rtol=1e-13, atol=0) and torch.allclose(lm['q'], h['q'][i], rtol=0, atol=1e-11)
    assert torch.equal(x, ft.x_last)


# ---------------------------------------------------------------- f4: delta-Q^2 tooling on HIP-produced histories
def test_observables_tooling_on_hip_histories():
    """64 physical-field ftHMC trajectories of 8 chains at L = 8 through qed_helpers.ft_hmc (what ft_run loops over: inverse
    sweep -> trajectory -> forward sweep, ipynb/ft_hmc.py:420-435) on the HIP path, and the same chains through the oracle
    with the same momenta and accept draws: equal accept and charge histories, and equal rows out of the delta-Q^2-vs-lag /
    block-error tooling (ipynb/ft_hmc.py:16-53,168-176) in the reference's literal mode, chain by chain and for the ensemble."""
    from fthmc_amd.config import Param
    from fthmc_amd.utils import layers as LY, observables as OB, qed_helpers as qed
    gen = torch.Generator().manual_seed(64)
    B, L, nl, beta, tau, nstep, ntraj = 8, 8, 4, 2.0, 1.0, 10, 64
    wts = R.default_flow(nl, gen)
    flow = LY.make_u1_equiv_layers(n_layers=nl, n_mixture_comps=2, lattice_shape=(L, L), hidden_sizes=[8, 8], kernel_size=3)
    names = ('net.0.weight', 'net.0.bias', 'net.2.weight', 'net.2.bias', 'net.4.weight', 'net.4.bias')
    flow.load_state_dict({f'{li}.plaq_coupling.{n}': wts[li][pi].cuda() for li in range(nl) for pi, n in enumerate(names)})
    param = Param(beta=beta, L=L, tau=tau, nstep=nstep)
    x0 = (torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi
    vs = torch.randn(ntraj, B, 2, L, L, generator=gen, dtype=torch.float64)
    us = torch.rand(ntraj, B, generator=gen, dtype=torch.float64)
    # HIP: one configuration at a time, as the notebook runs it
    fields = [x0[b:b + 1].cuda() for b in range(B)]
    qh = np.zeros((ntraj + 1, B)); acc_h = np.zeros((ntraj, B), dtype=bool)
    qh[0] = np.asarray(ops.wilson_action_charge(x0.cuda(), beta)[1].cpu())
    for k in range(ntraj):
        vk, uk = vs[k].cuda(), us[k].cuda()
        for b in range(B):
            _, _, acc, fields[b] = qed.ft_hmc(param, flow, fields[b], v=vk[b:b + 1], u=uk[b])
            acc_h[k, b] = bool(acc)
        qh[k + 1] = np.asarray(ops.wilson_action_charge(torch.cat(fields), beta)[1].cpu())
    # oracle: the chains as a batch of independent systems, same draws, inverse by bisection down to fp resolution
    xc = x0.clone()
    qc = np.zeros((ntraj + 1, B)); acc_c = np.zeros((ntraj, B), dtype=bool)
    qc[0] = R.charge(xc).numpy()
    for k in range(ntraj):
        with torch.no_grad():
            xi = R.flow_reverse(xc, wts, tol=1e-13)[0]
        _, _, acc, newx, _, _ = R.ft_hmc(xi, vs[k], us[k], wts, beta, tau / nstep, nstep, mode='md')
        with torch.no_grad():
            xc = R.flow_forward(newx, wts)[0]
        acc_c[k] = acc.numpy(); qc[k + 1] = R.charge(xc).numpy()
    assert np.abs(qh - np.round(qh)).max() < 1e-8
    qh, qc = np.round(qh), np.round(qc)
    assert np.array_equal(acc_h, acc_c) and 0.2 < acc_h.mean() <= 1.0
    assert np.array_equal(qh, qc) and np.abs(np.diff(qh, axis=0)).max() > 0        # the charge does move
    for q_h, q_c in [(qh[:, b], qc[:, b]) for b in range(B)] + [(qh, qc)]:
        rows_h = OB.change_sqr_vs_dt(q_h, dt_range=8, reference_literal=True)
        rows_c = OB.change_sqr_vs_dt(q_c, dt_range=8, reference_literal=True)
        np.testing.assert_array_equal(np.asarray(rows_h), np.asarray(rows_c))
    assert np.isfinite(np.asarray(OB.change_sqr_vs_dt(qh, dt_range=8))[:, 1]).all()
