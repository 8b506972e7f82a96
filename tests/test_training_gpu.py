"""GPU tests of training: checkpoints and the scheduler, the device-bound loop (flat parameter buffer, captured step, metrics
kernel, Philox prior draw, FlatAdam) against the step-by-step route and the oracle, the one-launch training sweep of the small
lattices, the GradScaler option, and the training backward that computes its weight gradients itself (csrc/flow_bwd_train.hip)
on every stripe direction / offset, walks of one and of several items per workgroup, chains that do not fill a walk."""
import math
import os

import numpy as np
import pytest
import torch

from gpu_support import H, R, angle_close, close, module_defaults, ops, switches

pytestmark = pytest.mark.gpu
_defaults = module_defaults()


# ---------------------------------------------------------------- training loop: checkpoints, scheduler, transfer
def test_train_checkpoint_round_trip_and_scheduler(tmp_path):
    """train(save=True) writes one reference-format .tar per era (io.py:114-172) holding numpy histories;
    restore_model_from_checkpoint (train.py:77-92) reads it back exactly; ReduceLROnPlateau (train.py:314-317)
    steps on the loss; transfer_to_new_lattice reuses the nets on 2L with the same per-site results."""
    from fthmc_amd import train as T
    from fthmc_amd.config import SchedulerConfig, TrainConfig
    tc = TrainConfig(L=8, beta=2.0, n_layers=4, batch_size=16, base_lr=5e-3, n_era=2, n_epoch=3, print_freq=0)
    tc.update_logdirs(str(tmp_path / 'run'))
    torch.manual_seed(11)
    sc = SchedulerConfig(factor=0.5, patience=0, threshold=1e9, threshold_mode='abs', min_lr=1e-6)   # every step "plateaus"
    out = T.train(tc, scheduler_config=sc, save=True, verbose=False)
    assert len(out['ckpt_files']) == 2 and os.path.basename(out['ckpt_files'][-1]) == 'ckpt-era1-epoch3.tar'
    assert out['optimizer'].param_groups[0]['lr'] < tc.base_lr                    # the scheduler stepped
    assert len(out['history']['loss_dkl']) == 6 and isinstance(out['history']['logp'][0], np.ndarray)
    raw = torch.load(out['ckpt_files'][-1], weights_only=False)
    assert set(raw) == {'era', 'epoch', 'model_state_dict', 'optimizer_state_dict', 'history'}
    assert '0.plaq_coupling.net.0.weight' in raw['model_state_dict'] and len(raw['history']['ess']) == 6
    back = T.restore_model_from_checkpoint(out['ckpt_files'][-1], tc)
    for (k, a), (k2, b) in zip(out['model'].layers.state_dict().items(), back['model'].layers.state_dict().items()):
        assert k == k2 and torch.equal(a, b)
    # Adam state (restore builds AdamW like the reference does: same state tensors)
    sa, sb = out['optimizer'].state_dict()['state'], back['optimizer'].state_dict()['state']
    assert len(sa) == len(sb) == 24 and all(torch.equal(sa[i]['exp_avg'], sb[i]['exp_avg']) for i in sa)
    # transfer: on a 16 x 16 lattice made of four copies of an 8 x 8 field the (translation-equivariant, periodic)
    # flow gives four copies of the 8 x 8 result and four times the log-det
    from fthmc_amd.utils import qed_helpers as qed
    big = T.transfer_to_new_lattice(16, out['model'].layers)
    x8 = out['model'].prior.sample_n(3)
    y8, ld8 = ops.flow_forward(x8, qed.flow_weights(out['model'].layers, x8.device), 4)
    x16 = x8.repeat(1, 1, 2, 2)
    y16, ld16 = ops.flow_forward(x16, qed.flow_weights(big.layers, x8.device), 4)
    angle_close(y16, y8.repeat(1, 1, 2, 2), atol=1e-10); close(ld16, 4 * ld8, rtol=1e-10)
    assert big.prior.sample_n(2).shape == (2, 2, 16, 16)


# ---------------------------------------------------------------- flat parameter buffer
def test_flat_parameter_buffer_keeps_the_reference_module_layout():
    """flatten_flow re-homes the conv parameters as views of one buffer in ABI order: state_dict keys and values,
    load_state_dict, optimizers and transfer_to_new_lattice keep working, flow_weights hands the buffer out without a copy."""
    from fthmc_amd import train as T
    from fthmc_amd.config import TrainConfig
    from fthmc_amd.utils import layers as LY
    tc = TrainConfig(L=8, beta=2.0, n_layers=4, batch_size=8)
    torch.manual_seed(5)
    model = T.get_model(tc)
    before = {k: v.clone() for k, v in model.layers.state_dict().items()}
    packed = LY.flow_weights(model.layers)                       # not flattened yet: a packed copy
    flat = LY.flatten_flow(model.layers)
    assert torch.equal(flat, packed) and flat.numel() == 4 * 955
    assert LY.flatten_flow(model.layers) is flat                 # idempotent
    assert LY.flow_weights(model.layers).data_ptr() == flat.data_ptr()          # no copy any more
    after = model.layers.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert '0.plaq_coupling.net.0.weight' in after and after['3.plaq_coupling.net.4.bias'].shape == (3,)
    # in-place updates through the parameters are updates of the buffer, and the other way round
    p = model.layers[1].plaq_coupling.net[2].weight
    with torch.no_grad():
        p.mul_(2.0)
    assert torch.equal(LY.flow_weights(model.layers)[955 + 152:955 + 152 + 576].view(8, 8, 3, 3), p)
    model.layers.load_state_dict(before)                         # copies in place: still views
    assert LY.flatten_flow(model.layers) is flat and torch.equal(flat, packed)
    # gradient buffer: every .grad is a view of it
    g = LY.flow_grad_buffer(model.layers)
    LY.attach_grads(model.layers)
    g.fill_(3.0)
    assert all(float(q.grad.min()) == 3.0 for q in model.layers.parameters())
    # a second ModuleList over the same nets (transfer) shares the buffer
    big = T.transfer_to_new_lattice(16, model.layers)
    assert LY.flow_weights(big.layers).data_ptr() == flat.data_ptr()
    # .to() re-creates the parameters: the next call flattens again
    model.layers.to(torch.float64)
    assert LY.flow_weights(model.layers).numel() == flat.numel()


# ---------------------------------------------------------------- device pieces of a training step
def test_prior_draw_and_metrics_kernels():
    from fthmc_amd import parallel
    B, L, beta = 37, 12, 3.0
    seeds = parallel.chain_seeds(7, 100, 100 + B, 3).cuda()
    xi = ops.random_uniform(seeds, (B, 2, L, L), -math.pi, math.pi)
    assert xi.shape == (B, 2, L, L) and float(xi.min()) >= -math.pi and float(xi.max()) < math.pi
    assert abs(float(xi.mean())) < 0.1 and abs(float(xi.var()) - math.pi ** 2 / 3) < 0.2
    # a chain's draw depends on its seed only: any sub-batch reproduces its chains bit for bit
    assert torch.equal(ops.random_uniform(seeds[5:9], (4, 2, L, L), -math.pi, math.pi), xi[5:9])
    assert not torch.equal(xi[0], xi[1])
    gen = torch.Generator().manual_seed(3)
    x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).cuda()
    logq = torch.randn(B, generator=gen, dtype=torch.float64).cuda() * 3 - 500
    logp = torch.randn(B, generator=gen, dtype=torch.float64).cuda() * 3 + 200
    row = ops.train_metrics(xi, x, logq, logp, beta, dkl_factor=0.7)
    m = ops.split_metrics(row, B)
    logw = logp - logq
    ess = torch.exp(2 * torch.logsumexp(logw, 0) - torch.logsumexp(2 * logw, 0)) / B     # calc_ess, distributions.py:27-37
    close(m['loss_dkl'], 0.7 * (logq - logp).mean(), rtol=1e-13)
    close(m['ess'], ess, rtol=1e-11)
    q, qi = ops.wilson_action_charge(x, beta)[1], ops.wilson_action_charge(xi, beta)[1]
    assert torch.equal(m['logp'], logp) and torch.equal(m['logq'], logq) and torch.equal(m['q'], q)
    close(m['dq'], (q - qi).abs(), atol=0); close(m['plaq'], logp / (beta * L * L), rtol=1e-15)


@pytest.mark.parametrize('decoupled,wd', [(False, 0.0), (False, 1e-2), (True, 1e-2)])
def test_flat_adam_equals_torch_adam(decoupled, wd):
    """FlatAdam (ONE launch on the flat buffers, step count and rate on the device) against torch.optim.Adam / AdamW on the
    same gradients, with a learning-rate change on the way, and its state_dict loaded into the torch optimizer and back."""
    from fthmc_amd import train as T
    from fthmc_amd.config import TrainConfig
    from fthmc_amd.utils import layers as LY
    tc = TrainConfig(L=8, beta=2.0, n_layers=3, batch_size=4)
    torch.manual_seed(2)
    a, b = T.get_model(tc), T.get_model(tc)
    b.layers.load_state_dict(a.layers.state_dict())
    oa = T.FlatAdam(a.layers, lr=3e-3, weight_decay=wd, decoupled=decoupled)
    ob = (torch.optim.AdamW if decoupled else torch.optim.Adam)(b.layers.parameters(), lr=3e-3, weight_decay=wd, foreach=False)
    ga = LY.flow_grad_buffer(a.layers)
    gen = torch.Generator().manual_seed(9)
    for k in range(7):
        g = torch.randn(ga.numel(), generator=gen, dtype=torch.float64).cuda() * (1.0 + k)
        ga.copy_(g)
        o = 0
        for p in b.layers.parameters():
            p.grad = g[o:o + p.numel()].view(p.shape).clone(); o += p.numel()
        if k == 4:
            for opt in (oa, ob):
                opt.param_groups[0]['lr'] = 1e-3             # what a scheduler does
        oa.step(); ob.step()
        close(LY.flow_weights(a.layers), LY.flow_weights(b.layers), rtol=1e-13, atol=1e-15)
    import copy
    sa, sb = copy.deepcopy(oa.state_dict()), copy.deepcopy(ob.state_dict())      # state_dict() hands out references, not copies
    assert sa['param_groups'][0]['lr'] == 1e-3 and len(sa['state']) == len(sb['state']) == 18
    for i in sa['state']:
        close(sa['state'][i]['exp_avg'], sb['state'][i]['exp_avg'], rtol=1e-13, atol=1e-18)
        close(sa['state'][i]['exp_avg_sq'], sb['state'][i]['exp_avg_sq'], rtol=1e-13, atol=1e-18)
        assert float(sa['state'][i]['step']) == float(sb['state'][i]['step']) == 7.0
    # either state loads into the other kind and the two keep walking together
    oa.load_state_dict(sb); ob.load_state_dict(sa)
    g = torch.randn(ga.numel(), generator=gen, dtype=torch.float64).cuda()
    ga.copy_(g); o = 0
    for p in b.layers.parameters():
        p.grad = g[o:o + p.numel()].view(p.shape).clone(); o += p.numel()
    oa.step(); ob.step()
    close(LY.flow_weights(a.layers), LY.flow_weights(b.layers), rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize('L,B,nl', [(8, 16, 4), (16, 8, 2), (20, 4, 3)])
def test_graph_trainer_equals_step_by_step(L, B, nl):
    """GraphTrainer (captured step, Philox prior, flat gradient buffer, FlatAdam: one launch per step) walks through the same
    weights and metrics as train_step called step by step on the same draws with the reference's optimizer
    (optim.Adam, train.py:297), and its eager mode equals its captured mode bit for bit."""
    from fthmc_amd import parallel, train as T
    from fthmc_amd.config import TrainConfig
    from fthmc_amd.utils import layers as LY
    from fthmc_amd.utils import qed_helpers as qed
    tc = TrainConfig(L=L, beta=2.5, n_layers=nl, batch_size=B, base_lr=2e-3, print_freq=0)
    torch.manual_seed(21)
    m0 = T.get_model(tc)
    init = {k: v.clone() for k, v in m0.layers.state_dict().items()}
    nsteps, seed = 5, 99
    runs = {}
    for mode in ('graph', 'eager'):
        model = T.get_model(tc); model.layers.load_state_dict(init)
        tr = T.GraphTrainer(model, tc, T.make_optimizer(model, tc), B, seed=seed, use_graph=(mode == 'graph'))
        for _ in range(nsteps):
            tr.step()
        hist_ = tr.history()                                     # synchronises the trainer's stream
        runs[mode] = (LY.flow_weights(model.layers).clone(), hist_)
    assert torch.equal(runs['graph'][0], runs['eager'][0])
    for k in T.METRIC_KEYS:
        assert all(np.array_equal(a, b) for a, b in zip(runs['graph'][1][k], runs['eager'][1][k])), k
    # step by step through the reference-shaped API with a plain Adam on the same draws
    model = T.get_model(tc); model.layers.load_state_dict(init)
    opt = torch.optim.Adam(model.layers.parameters(), lr=tc.base_lr)
    act = qed.BatchAction(tc.beta)
    hist = []
    for k in range(nsteps):
        xi = ops.random_uniform(parallel.chain_seeds(seed, 0, B, k).cuda(), (B, 2, L, L), -math.pi, math.pi)
        hist.append(T.train_step(model, tc, act, opt, B, xi=xi))
    close(LY.flow_weights(model.layers), runs['graph'][0], rtol=1e-9, atol=1e-12)
    gh = runs['graph'][1]
    assert len(gh['loss_dkl']) == nsteps and gh['logp'][0].shape == (B,) and gh['ess'][0].shape == ()
    for k in range(nsteps):
        for key in ('loss_dkl', 'ess', 'logp', 'logq', 'plaq'):
            close(hist[k][key], gh[key][k], rtol=1e-8, atol=1e-9)
        close(hist[k]['q'], gh['q'][k], atol=1e-8); close(hist[k]['dq'], gh['dq'][k], atol=1e-8)


def test_train_step_metrics_match_the_autograd_route():
    """train_step(fused=True) (flat gradient buffer, metrics kernel) against train_step(fused=False) (layer-wise autograd,
    torch formulas) on one draw: loss, ESS, per-chain arrays and every parameter gradient."""
    from fthmc_amd import train as T
    from fthmc_amd.config import TrainConfig
    from fthmc_amd.utils import qed_helpers as qed
    tc = TrainConfig(L=12, beta=3.0, n_layers=3, batch_size=6, base_lr=0.0, print_freq=0)
    torch.manual_seed(8)
    model = T.get_model(tc)
    xi = model.prior.sample_n(6)
    act = qed.BatchAction(tc.beta)
    outs, grads = [], []
    for fused in (True, False):
        opt = torch.optim.SGD(model.layers.parameters(), lr=0.0)
        outs.append(T.train_step(model, tc, act, opt, 6, xi=xi, fused=fused, dkl_factor=1.3))
        grads.append([p.grad.clone() for p in model.layers.parameters()])
    for k in T.METRIC_KEYS:
        close(outs[0][k], outs[1][k], rtol=1e-9, atol=1e-9)
    gmax = max(float(g.abs().max()) for g in grads[1])
    for a, b in zip(*grads):
        close(a, b, rtol=1e-8, atol=1e-11 * max(gmax, 1.0))


# ---------------------------------------------------------------- small lattices: the training sweep in one launch
@pytest.mark.parametrize('L,nl,B,beta,act', [(8, 4, 5, 2.0, 'silu'), (12, 3, 3, 3.0, 'silu'), (16, 8, 9, 4.0, 'silu'), (16, 2, 2, 2.0, 'relu'),
                                             (8, 1, 1, 1.0, 'leaky_relu')])
def test_small_lattice_training_sweep(L, nl, B, beta, act):
    """fthmc_train_grad at L = 8, 12, 16: ONE launch runs the forward sweep (stash, h1, h2, log J), the loss pieces and the
    backward sweep of every chain (flow_small.hip, training sweep), k_flow_wgrad turns the pre-activation gradients it leaves
    into weight gradients.  Against the tiled path (small path off) and against the oracle's autograd."""
    gen = torch.Generator().manual_seed(900 + L + nl)
    flow = R.default_flow(nl, gen)
    w = ops.pack_weights(flow, device='cuda')
    xi = (torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi
    assert ops.get_small_path()
    r = ops.train_grad(xi.cuda(), w, nl, beta, act)
    with switches(small=False):
        rt = ops.train_grad(xi.cuda(), w, nl, beta, act)
    d = (H(r['x']) - H(rt['x']) + np.pi) % (2 * np.pi) - np.pi
    assert np.abs(d).max() < 1e-11
    close(r['logq'], rt['logq'], rtol=1e-12); close(r['logp'], rt['logp'], rtol=1e-12)
    gmax = float(rt['gw'].abs().max())
    close(r['gw'], rt['gw'], rtol=1e-9, atol=1e-12 * max(gmax, 1.0))
    out, grads = R.train_grads(xi, flow, beta, act)
    close(r['logq'], out['logq'], rtol=1e-11); close(r['logp'], out['logp'], rtol=1e-11)
    gws = ops.unpack_weight_grads(r['gw'], nl)
    for li in range(nl):
        for pi in range(6):
            close(gws[li][pi], grads[li][pi], rtol=1e-8, atol=1e-11 * max(gmax, 1.0))
    assert torch.equal(ops.train_grad(xi.cuda(), w, nl, beta, act)['gw'], r['gw'])          # deterministic
    # the chains of a batch do not see each other: chain 0 alone
    r1 = ops.train_grad(xi[:1].cuda(), w, nl, beta, act, need_gw=False)
    close(r1['logq'], r['logq'][:1], rtol=1e-13); close(r1['logp'], r['logp'][:1], rtol=1e-13)


# ---------------------------------------------------------------- the reference's GradScaler option
def test_train_step_with_a_grad_scaler_equals_the_plain_step():
    """train_step(scaler=GradScaler()) (train.py:206-209, 321-324): scale(loss).backward(), scaler.step, scaler.update on the
    autograd route leave the weights of the plain step (fp64: the scale is a power of two, scaling and unscaling are exact) and
    the same metrics; train(use_scaler=True) runs."""
    from fthmc_amd import train as T
    from fthmc_amd.config import TrainConfig
    from fthmc_amd.utils import layers as LY
    from fthmc_amd.utils import qed_helpers as qed
    tc = TrainConfig(L=8, beta=2.0, n_layers=2, batch_size=6, base_lr=1e-3, print_freq=0, n_era=1, n_epoch=3)
    torch.manual_seed(4)
    m0 = T.get_model(tc)
    init = {k: v.clone() for k, v in m0.layers.state_dict().items()}
    xi = m0.prior.sample_n(6)
    act = qed.BatchAction(tc.beta)
    res = {}
    for tag in ('plain', 'scaler'):
        model = T.get_model(tc); model.layers.load_state_dict(init)
        opt = torch.optim.Adam(model.layers.parameters(), lr=tc.base_lr)
        sc = torch.amp.GradScaler('cuda') if tag == 'scaler' else None
        met = [T.train_step(model, tc, act, opt, 6, xi=xi, scaler=sc, fused=False) for _ in range(3)]
        res[tag] = (LY.flow_weights(model.layers).clone(), met)
    assert torch.equal(res['plain'][0], res['scaler'][0])
    for a, b in zip(res['plain'][1], res['scaler'][1]):
        for k in T.METRIC_KEYS:
            np.testing.assert_array_equal(a[k], b[k])
    out = T.train(tc, use_scaler=True, verbose=False)
    assert len(out['history']['loss_dkl']) == 3 and np.isfinite(out['history']['loss_dkl'][-1])


@pytest.mark.parametrize('B,L,nl,beta', [(1, 32, 8, 2.0),      # 4 items: every workgroup walks one tile; all eight (mu, off)
                                         (3, 64, 8, 6.0),      # 48 items
                                         (20, 64, 2, 4.0),     # 320 items > 256 workgroups: every workgroup walks two items
                                         (2, 128, 3, 3.0)])    # 128 items, tiles far from the lattice edge
def test_fused_training_backward_vs_oracle(B, L, nl, beta):
    """fthmc_train_grad on the tiled-exactly shapes (L a power of two >= 32: csrc/flow_bwd_train.hip) = loss.backward() of
    train_step (fthmc/train.py:191-210) through the oracle's autograd: loss pieces to 1e-11, every weight gradient to 1e-8
    relative (fp64; sums over up to 3e5 sites in another order); bit-identical on repetition (fixed summation order)."""
    gen = torch.Generator().manual_seed(600 + L + B)
    flow = R.default_flow(nl, gen)
    xi = (torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi
    nref = min(B, 3)                                            # the oracle's autograd is slow: the first chains, each on its own
    w = ops.pack_weights(flow, device='cuda')
    r = ops.train_grad(xi.cuda(), w, nl, beta, groups=1)
    r2 = ops.train_grad(xi.cuda(), w, nl, beta, groups=1)
    assert torch.equal(r['gw'], r2['gw']) and torch.equal(r['logq'], r2['logq'])
    per_chain = []
    for c in range(nref):
        out, grads = R.train_grads(xi[c:c + 1], flow, beta)
        close(r['logq'][c:c + 1], out['logq'], rtol=1e-11, atol=0.0); close(r['logp'][c:c + 1], out['logp'], rtol=1e-11, atol=0.0)
        rc =ops.train_grad(xi[c:c + 1].cuda(), w, nl, beta, groups=1)
        gws = ops.unpack_weight_grads(rc['gw'], nl)
        for li in range(nl):
            for pi in range(6):
                scale = float(grads[li][pi].abs().max())
                close(gws[li][pi], grads[li][pi], rtol=1e-8, atol=1e-10 * max(scale, 1.0))
        per_chain.append(rc['gw'])
    # the batch's gradient is the mean of its chains' (each chain's own call is checked above or is one more walk of the same kernel)
    for c in range(nref, B):
        per_chain.append(ops.train_grad(xi[c:c + 1].cuda(), w, nl, beta, groups=1)['gw'])
    close(r['gw'], sum(per_chain) / B, rtol=1e-9, atol=1e-10)


def test_fused_training_backward_leaves_the_force_path_alone():
    """the plaquette-gradient field the fused kernel hands down the sweep is the force path's: ft_force (k_flow_bwd_gather, no
    weight gradients) and the x-gradient implied by train_grad agree through the loss pieces; chain groups give the same gradient"""
    gen = torch.Generator().manual_seed(66)
    B, L, nl, beta = 4, 64, 4, 5.0
    flow = R.default_flow(nl, gen)
    w = ops.pack_weights(flow, device='cuda')
    xi = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).cuda()
    r1 = ops.train_grad(xi, w, nl, beta, groups=1)
    r2 = ops.train_grad(xi, w, nl, beta, groups=2)
    assert torch.equal(r1['logq'], r2['logq']) and torch.equal(r1['logp'], r2['logp'])
    close(r1['gw'], r2['gw'], rtol=1e-10, atol=1e-12)
    # directional derivative of the loss in weight space
    dw = torch.randn(w.numel(), generator=gen, dtype=torch.float64).cuda()
    dw = dw / dw.norm()

    def loss(wv):
        t = ops.train_grad(xi, wv, nl, beta, need_gw=False)
        return float((t['logq'] - t['logp']).mean())
    eps = 1e-6
    fd = (loss(w + eps * dw) - loss(w - eps * dw)) / (2 * eps)
    an = float((r1['gw'] * dw).sum())
    assert abs(an - fd) < 1e-5 * max(1.0, abs(an)), (an, fd)
