"""GPU tests of graph capture and of what a captured loop carries: workspaces under capture, the reference-shaped drivers
(FieldTransformation.run, qed_helpers.ft_run) as captured loops against their eager loops, the carried state keyed by the weights'
content, the weight versions of the C ABI checked on the device, and graph_loop.capture itself."""
import math

import pytest
import torch

from gpu_support import R, capture, close, module_defaults, ops

pytestmark = pytest.mark.gpu
_defaults = module_defaults()


# ---------------------------------------------------------------- workspace vs captured graphs
def test_workspace_survives_growth_after_capture():
    """A graph captured on a stream keeps replaying correctly after a larger call on the same stream replaced
    that stream's workspace; and growing a workspace during capture is refused."""
    from fthmc_amd._lib import FthmcError
    gen = torch.Generator().manual_seed(3)
    nl, beta = 2, 2.0
    flow = R.default_flow(nl, gen)
    w = ops.pack_weights(flow, device='cuda')
    xs = ((torch.rand(2, 2, 16, 16, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).cuda()
    xl = ((torch.rand(8, 2, 32, 32, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).cuda()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        want = ops.ft_force(xs, w, nl, beta).clone()            # warm-up: allocates this stream's workspace
        st.synchronize()
        out = torch.empty_like(xs)
        graph = torch.cuda.CUDAGraph()
        with capture(graph, st):
            out.copy_(ops.ft_force(xs, w, nl, beta))
        with pytest.raises(FthmcError, match='graph capture'):
            g2 = torch.cuda.CUDAGraph()
            with capture(g2, st):
                ops.ft_force(xl, w, nl, beta)                     # would have to grow the workspace while capturing
        big = ops.ft_force(xl, w, nl, beta)                       # eager: the workspace is replaced, the old one retired
        big2 = ops.ft_force(xl, w, nl, beta)
        out.zero_()
        graph.replay()
        st.synchronize()
        assert torch.equal(out, want)
        assert torch.equal(big, big2)
    close(big, R.ft_force(xl.cpu(), flow, beta), rtol=1e-8, atol=1e-9)


def _model(L, nl, B, beta=2.0, seed=11):
    from fthmc_amd import train as T
    from fthmc_amd.config import TrainConfig
    cfg = TrainConfig(L=L, beta=beta, n_layers=nl, batch_size=B, print_freq=0)
    torch.manual_seed(seed)
    return cfg, T.get_model(cfg)


# ---------------------------------------------------------------- the captured run loop
@pytest.mark.parametrize('L,nl,B', [(8, 2, 4), (16, 4, 8), (32, 2, 16)])
def test_captured_run_equals_the_eager_loop(L, nl, B):
    """FieldTransformation.run(batch=True): the captured loop (one graph launch per trajectory, momenta and uniforms from
    torch's generator inside the graph, state carried in place, history read back lazily) returns the history and the
    final field of the eager loop, bit for bit (fthmc/ft_hmc.py:272-346)."""
    from fthmc_amd.config import lfConfig
    from fthmc_amd.ft_hmc import FieldTransformation, LazyHistory
    cfg, model = _model(L, nl, B)
    x0 = (0.3 * (2 * torch.rand(B, 2, L, L, dtype=torch.float64) - 1)).cuda()
    n = 6
    out = {}
    for mode in ('graph', 'eager'):
        ft = FieldTransformation(flow=model.layers, config=cfg, lfconfig=lfConfig(tau=1.0, nstep=6))
        torch.manual_seed(5); torch.cuda.manual_seed(5)
        h = ft.run(x0.clone(), nprint=0, num_trajs=n, batch=True, use_graph=(mode == 'graph'))
        assert isinstance(h, LazyHistory) == (mode == 'graph')
        assert ft.captured == (mode == 'graph')
        # a second run from the field the first one returned: the carried state is taken over (no H0 sweep) in both modes
        h2 = ft.run(ft.x_last, nprint=0, num_trajs=3, batch=True, use_graph=(mode == 'graph'))
        out[mode] = (h, h2, ft.x_last.clone())
    for a, b in zip(out['graph'][:2], out['eager'][:2]):
        assert set(a.keys()) == set(b.keys()) == {'traj', 'dt', 'acc', 'dh', 'exp_mdh', 'plaq', 'q', 'dq'}
        for k in ('acc', 'dh', 'exp_mdh', 'plaq', 'q', 'dq'):
            assert len(a[k]) == len(b[k])
            for i, (ta, tb) in enumerate(zip(a[k], b[k])):
                assert torch.equal(ta, tb), (k, i)
        assert a['traj'] == b['traj']
    assert torch.equal(out['graph'][2], out['eager'][2])


def test_captured_single_chain_run_equals_the_eager_loop():
    """the reference's own shape: one [1, 2, L, L] system, one accept (ft_hmc.py:190-224)"""
    from fthmc_amd.config import lfConfig
    from fthmc_amd.ft_hmc import FieldTransformation
    L, nl, n = 8, 2, 7
    cfg, model = _model(L, nl, 1, seed=13)
    x0 = (0.3 * (2 * torch.rand(1, 2, L, L, dtype=torch.float64) - 1)).cuda()
    out = {}
    for mode in ('graph', 'eager'):
        ft = FieldTransformation(flow=model.layers, config=cfg, lfconfig=lfConfig(tau=1.0, nstep=8))
        torch.manual_seed(6); torch.cuda.manual_seed(6)
        out[mode] = (ft.run(x0.clone(), nprint=0, num_trajs=n, use_graph=(mode == 'graph')), ft.x_last.clone())
    a, b = out['graph'][0], out['eager'][0]
    for k in ('dh', 'plaq', 'q', 'dq'):
        for ta, tb in zip(a[k], b[k]):
            assert torch.equal(ta, tb), k
    assert [bool(t) for t in a['acc']] == [bool(t) for t in b['acc']]
    assert torch.equal(out['graph'][1], out['eager'][1])


def test_literal_reference_modes_stay_on_the_eager_loop():
    """energy_mode='reference_literal' (calc_energy's batch-wide kinetic term) has no fused trajectory: run() keeps
    the step-by-step loop and returns a plain dict"""
    from fthmc_amd.config import lfConfig
    from fthmc_amd.ft_hmc import FieldTransformation, LazyHistory
    cfg, model = _model(8, 2, 3)
    ft = FieldTransformation(flow=model.layers, config=cfg, lfconfig=lfConfig(tau=0.5, nstep=4), energy_mode='reference_literal')
    x0 = (0.3 * (2 * torch.rand(3, 2, 8, 8, dtype=torch.float64) - 1)).cuda()
    h = ft.run(x0, nprint=0, num_trajs=2, batch=True)
    assert not isinstance(h, LazyHistory) and len(h['acc']) == 2 and '_plaq' not in h and '_q' not in h


# ---------------------------------------------------------------- carry keyed by the weights' content
@pytest.mark.parametrize('use_graph', [True, False])
def test_carried_state_is_dropped_when_the_weights_change(use_graph):
    """run, a FlatAdam step (the kernel writes the flat buffer through raw pointers: no tensor version moves and
    flow_weights() hands out the same object), run(ft.x_last): the second run must take H0 from the NEW weights -- equal to the
    loop that recomputes everything -- and the same after load_state_dict and after a change of beta."""
    from fthmc_amd import train as T
    from fthmc_amd.config import lfConfig
    from fthmc_amd.ft_hmc import FieldTransformation
    from fthmc_amd.utils import layers as LY
    L, nl, B = 8, 2, 6
    cfg, model = _model(L, nl, B)
    opt = T.make_optimizer(model, cfg)                                   # FlatAdam: flattens the flow
    assert isinstance(opt, T.FlatAdam)
    ft = FieldTransformation(flow=model.layers, config=cfg, lfconfig=lfConfig(tau=1.0, nstep=6))
    x0 = (0.3 * (2 * torch.rand(B, 2, L, L, dtype=torch.float64) - 1)).cuda()
    torch.manual_seed(3); torch.cuda.manual_seed(3)
    ft.run(x0.clone(), nprint=0, num_trajs=3, batch=True, use_graph=use_graph)
    saved = {k: v.clone() for k, v in model.layers.state_dict().items()}

    def change_by_optimizer():
        w_before = LY.flow_weights(model.layers)
        LY.flow_grad_buffer(model.layers).normal_()
        opt.param_groups[0]['lr'] = 0.05
        opt.step()
        assert LY.flow_weights(model.layers) is w_before                 # the same object: identity says nothing

    def change_by_load():
        model.layers.load_state_dict(saved)

    def change_beta():
        cfg.beta = 2.7
        ft._denom = cfg.beta * cfg.volume

    for change in (change_by_optimizer, change_by_load, change_beta):
        x = ft.x_last
        change()
        torch.manual_seed(4); torch.cuda.manual_seed(4)
        h = ft.run(x, nprint=0, num_trajs=2, batch=True, use_graph=use_graph)
        # the stateless loop under the new weights on the same draws
        ft2 = FieldTransformation(flow=model.layers, config=cfg, lfconfig=lfConfig(tau=1.0, nstep=6))
        torch.manual_seed(4); torch.cuda.manual_seed(4)
        xx = x.clone()
        for i in range(2):
            xx, m = ft2._batch_hmc(xx.clone(), step=i)
            assert torch.equal(m['acc'], h['acc'][i]), change.__name__
            assert torch.equal(m['dh'], h['dh'][i]), change.__name__
        assert torch.equal(xx, ft.x_last), change.__name__


def test_weights_cache_follows_a_replaced_net():
    """FieldTransformation.weights() keeps the parameter list of the flow it saw; a conv net swapped inside the same
    ModuleList (transfer-style reuse) must be picked up"""
    from fthmc_amd.config import lfConfig
    from fthmc_amd.ft_hmc import FieldTransformation
    cfg, model = _model(8, 2, 2)
    _, other = _model(8, 2, 2, seed=99)
    ft = FieldTransformation(flow=model.layers, config=cfg, lfconfig=lfConfig(tau=1.0, nstep=4))
    x = (0.3 * (2 * torch.rand(2, 2, 8, 8, dtype=torch.float64) - 1)).cuda()
    s0 = ft.action(x).clone()
    model.layers[1].plaq_coupling.net = other.layers[1].plaq_coupling.net
    s1 = ft.action(x)
    ft_fresh = FieldTransformation(flow=model.layers, config=cfg, lfconfig=lfConfig(tau=1.0, nstep=4))
    assert torch.equal(s1, ft_fresh.action(x)) and not torch.equal(s0, s1)


# ---------------------------------------------------------------- weight versions (C ABI `_v` entry points)
def test_weight_versions_are_checked_on_the_device():
    """ops with a caller-stated weight version (`wkey` -> the `_v` entry points of the C ABI) expand the weights once per version
    into the stream's workspace; the library compares the version with the stamps its last expansion left there ON THE DEVICE:
    a wrong or stale version, other weights under the same version, a call without a version in between all end in an
    expansion and in the numbers of calls that state nothing.  That an equal version really skips the expansion is shown by
    wiping the expansion behind its stamps."""
    gen = torch.Generator().manual_seed(3)
    L, nl, B, beta = 16, 4, 5, 3.0
    wa = ops.pack_weights(R.default_flow(nl, gen), device='cuda')
    wb = ops.pack_weights(R.default_flow(nl, gen), device='cuda')
    x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).cuda()
    ref_a = ops.ft_action(x, wa, nl, beta)[0].clone()
    ref_b = ops.ft_action(x, wb, nl, beta)[0].clone()
    Fa = ops.ft_force(x, wa, nl, beta).clone()
    assert torch.equal(ops.ft_action(x, wa, nl, beta, wkey='v1')[0], ref_a)      # expands, stamps
    assert torch.equal(ops.ft_action(x, wa, nl, beta, wkey='v1')[0], ref_a)      # stamps found
    assert torch.equal(ops.ft_force(x, wa, nl, beta, wkey='v1'), Fa)
    # the expansion of layer 1 wiped behind its stamps (the head = 64 layer regions, the last 8 doubles of a region are its stamps: csrc/kernels.h)
    ws = ops._WS[(x.device.index, torch.cuda.current_stream().cuda_stream)]
    from fthmc_amd import _lib
    W = int(_lib.load().fthmc_ws_head_bytes()) // (64 * 8)
    assert W >= 8768 and int(_lib.load().fthmc_ws_head_bytes()) == 64 * W * 8
    ws[W:2 * W - 8].zero_()
    assert not torch.equal(ops.ft_action(x, wa, nl, beta, wkey='v1')[0], ref_a)  # same version: nothing was expanded (the proof)
    assert torch.equal(ops.ft_action(x, wa, nl, beta, wkey='other')[0], ref_a)   # a WRONG version: expanded, same numbers
    assert torch.equal(ops.ft_action(x, wa, nl, beta, wkey='other')[0], ref_a)
    assert torch.equal(ops.ft_action(x, wb, nl, beta, wkey='other')[0], ref_b)   # other weights under the same version: expanded
    assert torch.equal(ops.ft_action(x, wa, nl, beta, wkey='other')[0], ref_a)
    ops.flow_layer_fwd(x, wb[:955].contiguous(), 0, 0)                           # a call without a version overwrites layer 0 and clears its stamps
    assert torch.equal(ops.ft_action(x, wa, nl, beta, wkey='other')[0], ref_a)
    with pytest.raises(ops.FthmcError):                                          # a call that fails early leaves nothing behind (there is no state to leave)
        ops.ft_force(x[:, :, :6, :6].contiguous(), wb, nl, beta, wkey='other')
    assert torch.equal(ops.ft_action(x, wb, nl, beta, wkey='other')[0], ref_b)
    wa.mul_(1.01)                                                                # new content, new version
    ref_a2 = ops.ft_action(x, wa, nl, beta)[0].clone()
    assert torch.equal(ops.ft_action(x, wa, nl, beta, wkey='v2')[0], ref_a2) and not torch.equal(ref_a2, ref_a)
    # a graph captured under one version keeps producing the right numbers when other weights passed through its workspace
    # in between (the advisor's sequence: eager w1 -> replay with w2 -> eager w1)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        out_b = ops.ft_action(x, wb, nl, beta, wkey='g')[0]                      # warm-up: workspace of this stream
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with capture(g, st):
            out_b = ops.ft_action(x, wb, nl, beta, wkey='g')[0]
        assert torch.equal(ops.ft_action(x, wa, nl, beta, wkey='v2')[0], ref_a2)
        g.replay()
        assert torch.equal(out_b, ref_b)
        assert torch.equal(ops.ft_action(x, wa, nl, beta, wkey='v2')[0], ref_a2)
        g.replay()
        assert torch.equal(out_b, ref_b)
    torch.cuda.current_stream().wait_stream(st)


# ---------------------------------------------------------------- physical-field driver
def test_captured_ft_run_equals_the_eager_loop(tmp_path):
    """qed_helpers.ft_run (ipynb/ft_hmc.py:437-487: inverse flow, trajectory, forward flow, observables per trajectory of ONE
    configuration) as a captured loop against its eager loop: same histories, same final field, same log lines."""
    from fthmc_amd.config import Param
    from fthmc_amd.utils import qed_helpers as qed
    L, nl = 8, 2
    _, model = _model(L, nl, 1, seed=21)
    param = Param(beta=2.0, L=L, tau=1.0, nstep=6, ntraj=5, nrun=2)
    f0 = (0.4 * (2 * torch.rand(2, L, L, dtype=torch.float64) - 1)).cuda()
    res = {}
    for mode in ('graph', 'eager'):
        torch.manual_seed(8); torch.cuda.manual_seed(8)
        log = tmp_path / f'{mode}.log'
        field, hist = qed.ft_run(param, model.layers, f0.clone(), logfile=str(log), use_graph=(mode == 'graph'))
        res[mode] = (field.clone(), {k: list(v) for k, v in hist.items()}, log.read_text())
    assert torch.equal(res['graph'][0], res['eager'][0])
    for k in ('dH', 'exp_mdH', 'acc', 'plaq', 'topo'):
        assert res['graph'][1][k] == res['eager'][1][k], k
    assert res['graph'][2] == res['eager'][2]


def test_two_captured_loops_with_different_flows_do_not_disturb_each_other():
    """Two FieldTransformations over different flows, their captured runs interleaved (and an eager batch call in between on
    the shared stream pool): every run equals the eager loop of its own flow -- the replays carry no weight expansion, so each
    loop owns the streams (and with them the workspaces) it replays into, and re-establishes them at every run."""
    import pickle
    from fthmc_amd.config import lfConfig
    from fthmc_amd.ft_hmc import FieldTransformation
    L, nl, B = 32, 2, 16                                                  # two chain groups: the side-stream path
    cfg, ma = _model(L, nl, B, seed=31)
    _, mb = _model(L, nl, B, seed=32)
    x0 = (0.3 * (2 * torch.rand(B, 2, L, L, dtype=torch.float64) - 1)).cuda()
    lf = lfConfig(tau=1.0, nstep=5)
    want = {}
    for tag, m in (('a', ma), ('b', mb)):
        ft = FieldTransformation(flow=m.layers, config=cfg, lfconfig=lf)
        torch.manual_seed(7); torch.cuda.manual_seed(7)
        h1 = ft.run(x0.clone(), nprint=0, num_trajs=3, batch=True, use_graph=False)
        h2 = ft.run(ft.x_last, nprint=0, num_trajs=3, batch=True, use_graph=False)
        want[tag] = (torch.stack(h1['dh'] + h2['dh']), ft.x_last.clone())
    fa = FieldTransformation(flow=ma.layers, config=cfg, lfconfig=lf)
    fb = FieldTransformation(flow=mb.layers, config=cfg, lfconfig=lf)
    torch.manual_seed(7); torch.cuda.manual_seed(7)
    ga = torch.cuda.get_rng_state()
    ha1 = fa.run(x0.clone(), nprint=0, num_trajs=3, batch=True)
    sa = torch.cuda.get_rng_state()
    torch.cuda.set_rng_state(ga)
    hb1 = fb.run(x0.clone(), nprint=0, num_trajs=3, batch=True)
    sb = torch.cuda.get_rng_state()
    fb._batch_hmc(x0.clone())                                             # an eager two-group call on the shared side-stream pool
    torch.cuda.set_rng_state(sa)
    ha2 = fa.run(fa.x_last, nprint=0, num_trajs=3, batch=True)
    torch.cuda.set_rng_state(sb)
    hb2 = fb.run(fb.x_last, nprint=0, num_trajs=3, batch=True)
    assert torch.equal(torch.stack(ha1['dh'] + ha2['dh']), want['a'][0]) and torch.equal(fa.x_last, want['a'][1])
    assert torch.equal(torch.stack(hb1['dh'] + hb2['dh']), want['b'][0]) and torch.equal(fb.x_last, want['b'][1])
    plain = pickle.loads(pickle.dumps(ha1))                               # a LazyHistory travels as the dict it stands for
    assert type(plain) is dict and torch.equal(torch.stack(plain['dh']), torch.stack(ha1['dh']))


def test_capture_holds_the_garbage_collector_off():
    """graph_loop.capture: no automatic collection starts in the capturing thread (a finaliser that calls into the HIP runtime --
    an older graph's, a stream's -- would end the process there); the collector's state comes back, also after an error"""
    import gc
    from fthmc_amd.graph_loop import capture
    st, t = torch.cuda.Stream(), torch.zeros(4, dtype=torch.float64, device='cuda')
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        t.add_(1.0)
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        assert gc.isenabled()
        with capture(g, st):
            assert not gc.isenabled()
            t.add_(1.0)
        assert gc.isenabled()
        g.replay(); g.replay()
        st.synchronize()
        assert float(t[0]) == 3.0
        with pytest.raises(ZeroDivisionError):
            with capture(torch.cuda.CUDAGraph(), st):
                1 / 0
        assert gc.isenabled() and not torch.cuda.is_current_stream_capturing()
