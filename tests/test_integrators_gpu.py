"""GPU tests of the MD integrators (integrator='omelyan' | 'force_gradient' beside the leapfrog): plain HMC and ftHMC on every kernel
path against the CPU oracle run through the schedules of tests/integrator_cases.py, the bit equalities the sampler relies on,
reversibility, the Python drivers and the refusals.

Inputs: seeded uniform links in +-pi, normal momenta, tau = 0.5, Omelyan with nstep 3 and force-gradient with nstep 2.  Every
comparison of accept flags is made on inputs whose decisions are decided on the oracle's numbers: |u - exp(-dH)| > 1e-3 for every
chain (integrator_cases.decided_case redraws the seed by a fixed rule otherwise, at most 3 times)."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401

import integrator_cases as IC

from gpu_support import H, angle_close, close, module_defaults, ops, switches

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

TAU = 0.5
INTEGRATORS = (('omelyan', 3), ('force_gradient', 2))
BETA_PLAIN, BETA_FT = 3.0, 2.0


def flow_of(seed, nl, arch=None):
    from oracle import ref_cpu as R_
    gen = torch.Generator().manual_seed(seed)
    if arch is None:
        return R_.default_flow(nl, gen)
    return R_.default_flow(nl, gen, hidden=arch[0], k=arch[1], n_mix=arch[2])


# ---------------------------------------------------------------- the oracle's cases, computed once and shared
@functools.lru_cache(maxsize=None)
def plain_case(seed, B, L, name, nstep):
    dt = TAU / nstep
    return IC.decided_case(seed, B, L, lambda x, v, u: IC.plain_hmc(x, v, u, BETA_PLAIN, name, dt, nstep))


@functools.lru_cache(maxsize=None)
def ft_case(seed, B, L, nl, name, nstep, arch=None):
    dt = TAU / nstep
    flow = flow_of(seed, nl, arch)
    s, x, v, u, res = IC.decided_case(seed, B, L, lambda x, v, u: IC.ft_hmc(x, v, u, flow, BETA_FT, name, dt, nstep))
    return flow, s, x, v, u, res


# ---------------------------------------------------------------- plain HMC
# (id, seed, B, L): L = 8, 24 the one-launch kernel; L = 72 the tile kernels; L = 128 the row-strip kernels
PLAIN = [('L8', 11, 3, 8), ('L24', 12, 3, 24), ('L72', 13, 2, 72), ('L128', 14, 2, 128)]


def check_plain(r, res):
    close(r['dH'], res['dH'], rtol=1e-8, atol=1e-9)
    assert np.array_equal(H(r['acc']) > 0.5, res['acc'].numpy())
    close(r['x_new'], res['newx'], atol=1e-9)


@pytest.mark.parametrize('name,nstep', INTEGRATORS)
@pytest.mark.parametrize('case', PLAIN, ids=[c[0] for c in PLAIN])
def test_plain_hmc_vs_oracle(case, name, nstep):
    _, seed, B, L = case
    s, x, v, u, res = plain_case(seed, B, L, name, nstep)
    r = ops.hmc_trajectory(x.cuda(), v.cuda(), u.cuda(), BETA_PLAIN, TAU / nstep, nstep, integrator=name)
    close(r['H0'], res['H0'], rtol=1e-10); close(r['H1'], res['H1'], rtol=1e-8)
    check_plain(r, res)


@pytest.mark.parametrize('name,nstep', INTEGRATORS)
def test_plain_hmc_in_place_takes_the_multi_launch_path(name, nstep):
    """x_new aliasing x at L = 8: the one-launch kernel is not taken (C ABI directly: ops.hmc_trajectory refuses the alias)"""
    from fthmc_amd import _lib
    s, x, v, u, res = plain_case(11, 3, 8, name, nstep)
    B, L = 3, 8
    xd, vd, ud = x.cuda(), v.cuda(), u.cuda()
    dH, acc = torch.empty(B, dtype=torch.float64, device='cuda'), torch.empty(B, dtype=torch.float64, device='cuda')
    ws, nb = ops._ws(xd, B, L, 0)
    rc = _lib.load().fthmc_hmc_trajectory_int(ops._p(xd), ops._p(vd), ops._p(ud), B, L, BETA_PLAIN, TAU / nstep, nstep,
                                              _lib.INTEGRATORS[name], ops._p(xd), ops._p(dH), ops._p(acc), None, None, ws, nb,
                                              ops._stream(xd))
    assert rc == 0
    check_plain({'dH': dH, 'acc': acc, 'x_new': xd}, res)


@pytest.mark.parametrize('entry', ['hmc_trajectory', 'hmc_trajectory_pb'])
def test_plain_leapfrog_in_place_takes_the_multi_launch_path(entry):
    """the same with the leapfrog: fthmc_hmc_trajectory and fthmc_hmc_trajectory_pb (a constant beta_b) with x_new aliasing x at
    L = 8 run the fused leap steps, the regularizing pass and the separate energies, and are held to the oracle as above"""
    from fthmc_amd import _lib
    nstep = 3
    s, x, v, u, res = plain_case(11, 3, 8, 'leapfrog', nstep)
    B, L = 3, 8
    xd, vd, ud = x.cuda(), v.cuda(), u.cuda()
    dH, acc = torch.empty(B, dtype=torch.float64, device='cuda'), torch.empty(B, dtype=torch.float64, device='cuda')
    ws, nb = ops._ws(xd, B, L, 0)
    p = ops._p
    if entry == 'hmc_trajectory':
        rc = _lib.load().fthmc_hmc_trajectory(p(xd), p(vd), p(ud), B, L, BETA_PLAIN, TAU / nstep, nstep, p(xd), p(dH), p(acc), None, None,
                                              ws, nb, ops._stream(xd))
    else:
        bb = torch.full((B,), BETA_PLAIN, dtype=torch.float64, device='cuda')
        rc = _lib.load().fthmc_hmc_trajectory_pb(p(xd), p(vd), p(ud), B, L, p(bb), TAU / nstep, nstep, _lib.INTEGRATORS['leapfrog'],
                                                 p(xd), p(dH), p(acc), None, None, ws, nb, ops._stream(xd))
    assert rc == 0
    check_plain({'dH': dH, 'acc': acc, 'x_new': xd}, res)


@pytest.mark.parametrize('name,nstep', INTEGRATORS)
def test_plain_md_vs_oracle(name, nstep):
    x, p, _ = IC.draw(21, 3, 8)
    xo, po = ops.leapfrog(x.cuda(), p.cuda(), BETA_PLAIN, TAU / nstep, nstep, integrator=name)
    xr, pr = IC.plain_md(x, p, BETA_PLAIN, name, TAU / nstep, nstep)
    close(xo, xr, rtol=0, atol=1e-11); close(po, pr, rtol=0, atol=1e-11)


# ---------------------------------------------------------------- ftHMC
# (id, seed, B, L, layers, net shape, variant, small path)
FT = [('small-L8', 31, 3, 8, 2, None, 1, True), ('small-L12', 32, 3, 12, 3, None, 1, True), ('small-L16', 33, 3, 16, 4, None, 1, True),
      ('tiled-L16', 33, 3, 16, 4, None, 1, False),
      ('L32-3layers', 34, 2, 32, 3, None, 1, True), ('L32-4layers', 35, 2, 32, 4, None, 1, True),
      ('ragged-L20', 36, 2, 20, 2, None, 1, True),
      ('net-4-3-1-L8', 37, 3, 8, 2, ((4,), 3, 1), 1, True),
      ('valu-L16', 33, 3, 16, 4, None, 0, False)]


@pytest.mark.parametrize('name,nstep', INTEGRATORS)
@pytest.mark.parametrize('case', FT, ids=[c[0] for c in FT])
def test_ft_trajectory_vs_oracle(case, name, nstep):
    _, seed, B, L, nl, arch, variant, small = case
    flow, s, x, v, u, res = ft_case(seed, B, L, nl, name, nstep, arch)
    dt = TAU / nstep
    with switches(variant=variant, small=small):
        w = ops.pack_weights(flow, device='cuda')
        r = ops.ft_trajectory(x.cuda(), v.cuda(), u.cuda(), w, nl, BETA_FT, dt, nstep, mode='md', integrator=name)
        xo, vo = ops.ft_leapfrog(x.cuda(), v.cuda(), w, nl, BETA_FT, dt, nstep, integrator=name)
        torch.cuda.synchronize()
    close(r['H0'], res['H0'], rtol=1e-10); close(r['H1'], res['H1'], rtol=1e-7)
    close(r['dH'], res['dH'], rtol=1e-6, atol=1e-6)
    assert np.array_equal(H(r['acc']) > 0.5, res['acc'].numpy())
    angle_close(r['x_new'], res['newx'], atol=1e-6)
    close(r['plaq'], res['plaq'], rtol=1e-6); close(r['Q'], res['Q'], atol=1e-6)
    close(xo, res['md_x'], rtol=1e-7, atol=1e-7); close(vo, res['md_v'], rtol=1e-7, atol=1e-7)


# ---------------------------------------------------------------- bit equalities
KEYS = ('x_new', 'dH', 'acc', 'H0', 'H1', 'plaq', 'Q', 'state')


def _inputs(seed, B, L, nl):
    flow = flow_of(seed, nl)
    x, v, u = IC.draw(seed, B, L)
    return ops.pack_weights(flow, device='cuda'), x.cuda(), v.cuda(), u.cuda()


def _same(a, b, keys=KEYS):
    for k in keys:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('L,nl', [(16, 4), (32, 3)])
def test_leapfrog_through_the_new_entry_points_is_the_leapfrog(L, nl):
    """FTHMC_INT_LEAPFROG through fthmc_ft_trajectory_int_v / fthmc_ft_md_v / fthmc_hmc_trajectory_int / fthmc_md (C ABI: the
    Python wrappers route 'leapfrog' to the old entry points themselves) = the existing entry points, bit for bit"""
    from fthmc_amd import _lib
    lib = _lib.load()
    B, dt, nstep = 3, 0.1, 3
    w, x, v, u = _inputs(41, B, L, nl)
    ref = ops.ft_trajectory(x, v, u, w, nl, BETA_FT, dt, nstep)
    out = {k: torch.empty_like(t) for k, t in ref.items()}
    ws, nb = ops._ws(x, B, L, nl)
    p = ops._p
    rc = lib.fthmc_ft_trajectory_int_v(p(x), p(v), p(u), p(w), None, nl, B, L, 0, BETA_FT, dt, nstep, 0, p(out['x_new']), p(out['dH']),
                                       p(out['acc']), p(out['H0']), p(out['H1']), p(out['plaq']), p(out['Q']), None, p(out['state']),
                                       ws, nb, ops._stream(x), 0, 0)
    assert rc == 0
    _same(out, ref)
    xo, vo = ops.ft_leapfrog(x, v, w, nl, BETA_FT, dt, nstep)
    x2, v2 = torch.empty_like(x), torch.empty_like(v)
    assert lib.fthmc_ft_md_v(p(x), p(v), p(w), None, nl, B, L, 0, BETA_FT, dt, nstep, p(x2), p(v2), ws, nb, ops._stream(x), 0, 0) == 0
    assert torch.equal(x2, xo) and torch.equal(v2, vo)
    # the plain twins
    rp = ops.hmc_trajectory(x, v, u, BETA_PLAIN, dt, nstep)
    xn, dH, acc = torch.empty_like(x), torch.empty(B, dtype=torch.float64, device='cuda'), torch.empty(B, dtype=torch.float64, device='cuda')
    ws0, nb0 = ops._ws(x, B, L, 0)
    assert lib.fthmc_hmc_trajectory_int(p(x), p(v), p(u), B, L, BETA_PLAIN, dt, nstep, 0, p(xn), p(dH), p(acc), None, None, ws0, nb0,
                                        ops._stream(x)) == 0
    assert torch.equal(xn, rp['x_new']) and torch.equal(dH, rp['dH']) and torch.equal(acc, rp['acc'])
    xl, pl = ops.leapfrog(x, v, BETA_PLAIN, dt, nstep)
    assert lib.fthmc_md(p(x), p(v), B, L, BETA_PLAIN, dt, nstep, 0, p(x2), p(v2), ws0, nb0, ops._stream(x)) == 0
    assert torch.equal(x2, xl) and torch.equal(v2, pl)


@pytest.mark.parametrize('name,nstep', INTEGRATORS)
@pytest.mark.parametrize('L,nl', [(16, 4), (32, 3)])
def test_two_identical_calls_give_the_same_bits(L, nl, name, nstep):
    w, x, v, u = _inputs(42, 3, L, nl)
    a = ops.ft_trajectory(x, v, u, w, nl, BETA_FT, TAU / nstep, nstep, integrator=name)
    b = ops.ft_trajectory(x, v, u, w, nl, BETA_FT, TAU / nstep, nstep, integrator=name)
    _same(a, b)


@pytest.mark.parametrize('name,nstep', INTEGRATORS)
def test_chain_groups_and_batch_size_do_not_change_a_chain(name, nstep):
    """groups=2 equals groups=1 at B = 4, L = 32; chains 0..1 of the B = 4 call equal a B = 2 call"""
    L, nl = 32, 3
    w, x, v, u = _inputs(43, 4, L, nl)
    dt = TAU / nstep
    one = ops.ft_trajectory(x, v, u, w, nl, BETA_FT, dt, nstep, integrator=name, groups=1)
    two = ops.ft_trajectory(x, v, u, w, nl, BETA_FT, dt, nstep, integrator=name, groups=2)
    torch.cuda.synchronize()
    _same(one, two)
    half = ops.ft_trajectory(x[:2].contiguous(), v[:2].contiguous(), u[:2].contiguous(), w, nl, BETA_FT, dt, nstep, integrator=name)
    for k in KEYS:
        full = one[k][:, :2] if k == 'state' else one[k][:2]
        assert torch.equal(full, half[k]), k


@pytest.mark.parametrize('name,nstep', INTEGRATORS)
@pytest.mark.parametrize('L,nl', [(16, 4), (32, 3)])
def test_chained_state_equals_stateless(L, nl, name, nstep):
    """state_out -> state_in over 3 trajectories changes nothing"""
    B = 3
    flow = flow_of(44, nl)
    w = ops.pack_weights(flow, device='cuda')
    gen = torch.Generator().manual_seed(44)
    x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).cuda()
    xa, xb, state = x.clone(), x.clone(), None
    for t in range(3):
        v = torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64).cuda()
        u = torch.rand(B, generator=gen, dtype=torch.float64).cuda()
        ra = ops.ft_trajectory(xa, v, u, w, nl, BETA_FT, TAU / nstep, nstep, integrator=name)
        rb = ops.ft_trajectory(xb, v, u, w, nl, BETA_FT, TAU / nstep, nstep, integrator=name, state_in=state)
        _same(ra, rb)
        xa, xb, state = ra['x_new'].clone(), rb['x_new'].clone(), rb['state'].clone()


# (id, integrator, nstep, per-chain beta)
GENERAL_SETTINGS = [('leapfrog', 'leapfrog', 3, False), ('omelyan', 'omelyan', 3, False), ('force_gradient-ladder', 'force_gradient', 2, True)]


@pytest.mark.parametrize('setting', GENERAL_SETTINGS, ids=[c[0] for c in GENERAL_SETTINGS])
@pytest.mark.parametrize('nl,arch', [(2, ((4,), 3, 1)), (0, None)], ids=['net-4-3-1', 'no-layers'])
def test_chained_state_equals_stateless_on_the_general_branch(nl, arch, setting):
    """Another net shape and a flow without layers take the general branch of the sequencer (energies, MD and Metropolis as
    separate launches) at L = 8: state_out -> state_in over 2 trajectories changes nothing, with a number as beta (the state is
    copied into the old triple) and with a per-chain ladder (the beta-free state: pb_eval copies it)"""
    _, name, nstep, ladder = setting
    B, L = 3, 8
    w = ops.pack_weights(flow_of(46, nl, arch), device='cuda') if nl else None
    beta = torch.tensor([1.5, 2.0, 3.0], dtype=torch.float64, device='cuda') if ladder else BETA_FT
    gen = torch.Generator().manual_seed(46)
    x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).cuda()
    xa, xb, state = x.clone(), x.clone(), None
    for t in range(2):
        v = torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64).cuda()
        u = torch.rand(B, generator=gen, dtype=torch.float64).cuda()
        ra = ops.ft_trajectory(xa, v, u, w, nl, beta, TAU / nstep, nstep, integrator=name)
        rb = ops.ft_trajectory(xb, v, u, w, nl, beta, TAU / nstep, nstep, integrator=name, state_in=state)
        _same(ra, rb)
        xa, xb, state = ra['x_new'].clone(), rb['x_new'].clone(), rb['state'].clone()


# ---------------------------------------------------------------- reversibility
@pytest.mark.parametrize('name,nstep', INTEGRATORS)
@pytest.mark.parametrize('L,nl', [(16, 4), (32, 3)])
def test_md_is_reversible(L, nl, name, nstep):
    w, x, v, _ = _inputs(45, 3, L, nl)
    dt = TAU / nstep
    x1, v1 = ops.ft_leapfrog(x, v, w, nl, BETA_FT, dt, nstep, integrator=name)
    x2, v2 = ops.ft_leapfrog(x1, -v1, w, nl, BETA_FT, dt, nstep, integrator=name)
    close(x2, x, rtol=0, atol=1e-8); close(-v2, v, rtol=0, atol=1e-8)


# ---------------------------------------------------------------- the Python drivers
def _ft(L, nl, integrator, B=1, seed=11):
    from fthmc_amd import train as T
    from fthmc_amd.config import TrainConfig, lfConfig
    from fthmc_amd.ft_hmc import FieldTransformation
    cfg = TrainConfig(L=L, beta=BETA_FT, n_layers=nl, batch_size=B, print_freq=0)
    torch.manual_seed(seed)
    model = T.get_model(cfg)
    return FieldTransformation(flow=model.layers, config=cfg, lfconfig=lfConfig(tau=TAU, nstep=2), integrator=integrator)


def test_field_transformation_hmc_is_ft_trajectory():
    L, nl = 8, 2
    ft = _ft(L, nl, 'force_gradient')
    x, v, u = (t.cuda() for t in IC.draw(51, 1, L))
    xnew, m = ft.hmc(x, v=v, u=u[0])
    r = ops.ft_trajectory(x, v, u, ft.weights(x.device), nl, BETA_FT, ft.dt, ft.nstep, ft._act, integrator='force_gradient')
    assert torch.equal(xnew, r['x_new']) and torch.equal(m['dh'], r['dH'][0]) and bool(m['acc']) == bool(r['acc'][0] > 0.5)
    # and it is not the leapfrog's trajectory
    r0 = ops.ft_trajectory(x, v, u, ft.weights(x.device), nl, BETA_FT, ft.dt, ft.nstep, ft._act)
    assert not torch.equal(r0['dH'], r['dH'])
    x1, v1 = ft.leapfrog(x, v)
    x2, v2 = ops.ft_leapfrog(x, v, ft.weights(x.device), nl, BETA_FT, ft.dt, ft.nstep, ft._act, integrator='force_gradient')
    assert torch.equal(x1, x2) and torch.equal(v1, v2)


def test_captured_run_equals_the_eager_loop():
    L, nl, B, n = 8, 2, 4, 4
    x0 = (0.3 * (2 * torch.rand(B, 2, L, L, dtype=torch.float64, generator=torch.Generator().manual_seed(52)) - 1)).cuda()
    out = {}
    for mode in ('graph', 'eager'):
        ft = _ft(L, nl, 'force_gradient', B=B)
        torch.manual_seed(5); torch.cuda.manual_seed(5)
        h = ft.run(x0.clone(), nprint=0, num_trajs=n, batch=True, use_graph=(mode == 'graph'))
        assert ft.captured == (mode == 'graph')
        out[mode] = ({k: [t.clone() for t in h[k]] for k in ('acc', 'dh', 'exp_mdh', 'plaq', 'q', 'dq')}, ft.x_last.clone())
    for k, a in out['graph'][0].items():
        b = out['eager'][0][k]
        assert len(a) == len(b) == n
        for i, (ta, tb) in enumerate(zip(a, b)):
            assert torch.equal(ta, tb), (k, i)
    assert torch.equal(out['graph'][1], out['eager'][1])
    # the same draws under the leapfrog give another history: the keyword reached the captured loop
    ft = _ft(L, nl, 'leapfrog', B=B)
    torch.manual_seed(5); torch.cuda.manual_seed(5)
    h = ft.run(x0.clone(), nprint=0, num_trajs=n, batch=True, use_graph=True)
    assert not torch.equal(h['dh'][0], out['graph'][0]['dh'][0])


# ---------------------------------------------------------------- refusals
def test_refusals():
    from fthmc_amd._lib import FthmcError
    from fthmc_amd.config import TrainConfig, lfConfig
    from fthmc_amd.ft_hmc import FieldTransformation
    L, nl = 8, 2
    w, x, v, u = _inputs(61, 2, L, nl)
    with pytest.raises(ValueError):
        ops.ft_trajectory(x, v, u, w, nl, BETA_FT, 0.1, 2, integrator='verlet')
    with pytest.raises(ValueError):
        ops.hmc_trajectory(x, v, u, BETA_PLAIN, 0.1, 2, integrator='verlet')
    for mode in ('literal', 'reference_literal'):
        with pytest.raises(ValueError):
            ops.ft_trajectory(x, v, u, w, nl, BETA_FT, 0.1, 2, mode=mode, integrator='omelyan')
    for name in ('omelyan', 'force_gradient'):
        with pytest.raises(FthmcError):
            ops.ft_trajectory(x, v, u, w, nl, BETA_FT, 0.1, 0, integrator=name)
        with pytest.raises(FthmcError):
            ops.ft_leapfrog(x, v, w, nl, BETA_FT, 0.1, 0, integrator=name)
        with pytest.raises(FthmcError):
            ops.hmc_trajectory(x, v, u, BETA_PLAIN, 0.1, 0, integrator=name)
        with pytest.raises(FthmcError):
            ops.leapfrog(x, v, BETA_PLAIN, 0.1, 0, integrator=name)
    # the C ABI itself: an unknown integrator and the literal mode with another integrator are FTHMC_ERR_UNSUPPORTED
    from fthmc_amd import _lib
    lib = _lib.load()
    p = ops._p
    out = {k: torch.empty(2, dtype=torch.float64, device='cuda') for k in ('dH', 'acc')}
    xn = torch.empty_like(x)
    ws, nb = ops._ws(x, 2, L, nl)
    for integ, mode in ((5, 0), (1, 1)):
        rc = lib.fthmc_ft_trajectory_int_v(p(x), p(v), p(u), p(w), None, nl, 2, L, 0, BETA_FT, 0.1, 2, mode, p(xn), p(out['dH']),
                                           p(out['acc']), None, None, None, None, None, None, ws, nb, ops._stream(x), integ, 0)
        assert rc == -2, (integ, mode, rc)
    assert lib.fthmc_md(p(x), p(v), 2, L, BETA_PLAIN, 0.1, 2, 5, p(xn), p(xn), ws, nb, ops._stream(x)) == -2
    cfg = TrainConfig(L=L, beta=BETA_FT, n_layers=nl)
    with pytest.raises(ValueError):
        FieldTransformation(torch.nn.ModuleList(), cfg, lfConfig(tau=0.5, nstep=2), leapfrog_mode='reference_literal', integrator='omelyan')
    with pytest.raises(ValueError):
        FieldTransformation(torch.nn.ModuleList(), cfg, lfConfig(tau=0.5, nstep=2), integrator='verlet')
