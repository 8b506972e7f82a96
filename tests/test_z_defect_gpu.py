"""GPU tests of boundary-condition tempering (csrc/defect.hip) against the numpy twin of tests/defect_cases.py.  (Named to be
collected behind every other GPU test file; nothing here or there depends on the order: the module sets the library's default variant
and small path, as the other GPU modules do, and keeps its scratch in a cache family of its own.)

Cases (defect_cases.CASES): (B, L) in {(3, 4), (2, 8), (5, 12), (2, 20), (3, 32), (2, 36), (2, 64)} on the one-launch and the sequenced
path, (2, 68) and (1, 128) on the sequenced path; field amplitudes pi and 0.3, beta 2 and 6, nstep 1 and 3, the three integrators; the
defects Ld = 0, 1 and L, a row that wraps at j0 = L - 1 and one at j0 = 0; g_b per chain mixed out of {0, beta / 3, beta}.

Bounds: the project's figures for the plain kernels (tests/test_integrators_gpu.py: H0 rtol 1e-10, forces 1e-11 of their scale,
x_new atol 1e-9, dH rtol 1e-8 / atol 1e-9, H1 rtol 1e-8).  The float64 twin against the long double twin on these cases
(tests/test_defect.py, measured): force 1.0e-15 of its scale, S_d 8.6e-13 relative, H0 5.4e-16 relative, x_new 2.1e-15, H1 3.1e-15
relative, dH 3.9e-12 -- 8 x each is far inside the figures above, so no case widens a bound.  Accept flags are compared on every chain:
the twin leaves none out on these inputs (|u - exp(-dH)| >= 1e-6 exp(-dH))."""
import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401

import defect_cases as DC

import gpu_support
from gpu_support import D, H, module_defaults, ops

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

LD = np.longdouble
Q2_EXACT_L16_B6 = 1.1947014482


class _Twin(dict):
    """the float64 twin against the long double twin, worst over the cases: computed from defect_cases when first read (what
    tests/test_defect.py prints), so that the figures beside the bounds follow the cases"""

    def _fill(self):
        if not len(self):
            w = dict.fromkeys(('force', 'S', 'H0', 'x_new', 'dH', 'H1'), 0.0)
            for c in DC.CASES:
                B, L, amp, beta, nstep, integ, dk = c
                x, v, u, g, df, ref = DC.case(c)
                r = DC.trajectory(x, v, u, beta, g, df, DC.DT, nstep, integ, dt=np.float64)
                S64, SLD = DC.action(x, beta, g, df, np.float64)[0], DC.action(x, beta, g, df, LD)[0]
                fig = {'force': DC.rel_err(DC.force(x, beta, g, df, np.float64), DC.force(x, beta, g, df, LD)),
                       'S': float(np.abs((S64.astype(LD) - SLD) / SLD).max()),
                       'H0': float(np.abs((r['H0'].astype(LD) - ref['H0']) / ref['H0']).max()),
                       'x_new': float(np.abs(r['x_new'].astype(LD) - ref['x_new']).max()),
                       'dH': float(np.abs(r['dH'].astype(LD) - ref['dH']).max()),
                       'H1': float(np.abs((r['H1'].astype(LD) - ref['H1']) / ref['H1']).max())}
                for k, val in fig.items():
                    w[k] = max(w[k], val)
            self.update(w)
        return self

    def __getitem__(self, k):
        return dict.__getitem__(self._fill(), k)

    def __repr__(self):
        return repr({k: f'{val:.2e}' for k, val in self._fill().items()})


TWIN = _Twin()
KEYS = ('x_new', 'dH', 'acc', 'H0', 'H1', 'csum', 'dsum', 'Q')


def close(a, b, rtol=1e-10, atol=1e-10):
    """against the twin's longdouble figures, rounded to fp64 first"""
    gpu_support.close(a, DC.f64(b), rtol=rtol, atol=atol)


def bits(a, b):
    a, b = H(a), H(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def paths_of(L):
    return (1, 2) if L <= 64 else (2,)


def dev_case(c):
    x, v, u, g, df, ref = DC.case(c)
    return D(x), D(v), D(u), D(g), df, ref


def run(c, path, out=None, g=None, sl=slice(None)):
    B, L, amp, beta, nstep, integ, dk = c
    x, v, u, gd, df, ref = dev_case(c)
    return ops.defect_trajectory(x[sl].clone(), v[sl].clone(), u[sl].clone(), beta, (gd if g is None else g)[sl].clone(), df, DC.DT, nstep,
                                 integrator=integ, path=path, out=out)


def parent_in_place(x, v, u, beta_b, dt, nstep, integ):
    """the parent's sequenced per-chain-beta trajectory at any L: fthmc_hmc_trajectory_pb with x_new aliasing x (C ABI directly:
    ops.hmc_trajectory refuses the alias) -> dict as ops.hmc_trajectory"""
    from fthmc_amd import _lib
    B, _, L, _ = x.shape
    xd = x.clone()
    o = {k: torch.empty(B, dtype=torch.float64, device='cuda') for k in ('dH', 'acc', 'H0', 'H1')}
    ws, nb = ops._ws(xd, B, L, 0)
    rc = _lib.load().fthmc_hmc_trajectory_pb(ops._p(xd), ops._p(v), ops._p(u), B, L, ops._p(beta_b), dt, nstep, _lib.INTEGRATORS[integ], ops._p(xd),
                                             ops._p(o['dH']), ops._p(o['acc']), ops._p(o['H0']), ops._p(o['H1']), ws, nb, ops._stream(xd))
    assert rc == 0
    o['x_new'] = xd
    return o


def test_the_twin_figures_do_not_widen_a_bound():
    print('float64 twin vs long double twin on these cases:', TWIN, '-- bounds: force 1e-11, S 1e-10, H0 1e-10, x_new 1e-9, dH 1e-9 + 1e-8 |dH|, H1 1e-8')
    assert 8 * TWIN['force'] <= 1e-11 and 8 * TWIN['S'] <= 1e-10 and 8 * TWIN['H0'] <= 1e-10 and 8 * TWIN['x_new'] <= 1e-9
    assert 8 * TWIN['dH'] <= 1e-9 and 8 * TWIN['H1'] <= 1e-8


# ---------------------------------------------------------------- g_b = beta: the per-chain-beta kernels' bits
@pytest.mark.parametrize('c', DC.CASES, ids=DC.case_id)
def test_periodic_coupling_gives_the_per_chain_beta_trajectory_bit_for_bit(c):
    B, L, amp, beta, nstep, integ, dk = c
    x, v, u, g, df, ref = dev_case(c)
    bb = torch.full((B,), beta, dtype=torch.float64, device='cuda')
    C, Dsum, Q = DC.sums(DC.case(c)[0], df, LD)
    for path in paths_of(L):
        r = run(c, path, g=bb)
        if path == 1:
            p = ops.hmc_trajectory(x, v, u, bb, DC.DT, nstep, integrator=integ)            # L <= 64: the one-launch kernel
        else:
            p = parent_in_place(x, v, u, bb, DC.DT, nstep, integ)                           # the sequenced form
        for k in ('x_new', 'dH', 'acc', 'H0', 'H1'):
            assert bits(r[k], p[k]), (path, k, float(np.abs(H(r[k]) - H(p[k])).max()))
        tw = DC.sums(H(r['x_new']), df, LD)                                                 # of the field x_new holds
        close(r['csum'], tw[0], rtol=1e-11, atol=0.0)
        close(r['dsum'], tw[1], rtol=1e-11, atol=0.0)
        assert np.array_equal(H(r['Q']), tw[2])
    if L > 64:                                                                              # there ops.hmc_trajectory is the sequenced form too
        p = ops.hmc_trajectory(x, v, u, bb, DC.DT, nstep, integrator=integ)
        assert all(bits(r[k], p[k]) for k in ('x_new', 'dH', 'acc', 'H0', 'H1'))


# ---------------------------------------------------------------- the pieces on their own
@pytest.mark.parametrize('c', DC.CASES, ids=DC.case_id)
def test_force_and_action_against_the_long_double_twin(c):
    B, L, amp, beta, nstep, integ, dk = c
    x, v, u, g, df, ref = dev_case(c)
    xh, gh = DC.case(c)[0], DC.case(c)[3]
    F = DC.force(xh, beta, gh, df, LD)
    scale = float(np.abs(F).max())
    Fd = H(ops.defect_force(x, beta, g, df))
    err = float(np.abs(Fd.astype(LD) - F).max())
    S, C, Dsum, Q = DC.action(xh, beta, gh, df, LD)
    Sd, Cd, Dd, Qd = ops.defect_action(x, beta, g, df)
    print(f'force {err / scale:.2e} of its scale (bound 1e-11), S {float(np.abs((H(Sd).astype(LD) - S) / S).max()):.2e} relative (bound 1e-10)')
    assert err <= 1e-11 * scale
    close(Sd, S, rtol=1e-10, atol=0.0)
    close(Cd, C, rtol=1e-11, atol=0.0)
    close(Dd, Dsum, rtol=1e-11, atol=1e-13)
    assert np.array_equal(H(Qd), Q)
    # each output optional: the same bits into a caller's tensors, one at a time
    for k, full in zip(('S', 'csum', 'dsum', 'Q'), (Sd, Cd, Dd, Qd)):
        o = {k: torch.full((B,), float('nan'), dtype=torch.float64, device='cuda')}
        ops.defect_action(x, beta, g, df, out=o)
        assert bits(o[k], full)
    from fthmc_amd import _lib
    only = torch.full((B,), float('nan'), dtype=torch.float64, device='cuda')
    assert _lib.load().fthmc_defect_action(ops._p(x), B, L, beta, ops._p(g), *df, None, None, ops._p(only), None, ops._stream(x)) == 0
    assert bits(only, Dd)
    assert bits(ops.defect_force(x[B - 1:].clone(), beta, g[B - 1:].clone(), df), Fd[B - 1:])   # a chain alone


# ---------------------------------------------------------------- whole trajectories
@pytest.mark.parametrize('c', DC.CASES, ids=DC.case_id)
def test_trajectory_against_the_twin_on_every_path(c):
    B, L, amp, beta, nstep, integ, dk = c
    x, v, u, g, df, ref = dev_case(c)
    res = {}
    for path in paths_of(L):
        r = res[path] = run(c, path)
        print(f'path {path}: H0 {float(np.abs((H(r["H0"]).astype(LD) - ref["H0"]) / ref["H0"]).max()):.2e} (1e-10), x_new '
              f'{float(np.abs(H(r["x_new"]).astype(LD) - ref["x_new"]).max()):.2e} (1e-9), dH {float(np.abs(H(r["dH"]).astype(LD) - ref["dH"]).max()):.2e} '
              f'(1e-9 + 1e-8 |dH|), H1 {float(np.abs((H(r["H1"]).astype(LD) - ref["H1"]) / ref["H1"]).max()):.2e} (1e-8); twin float64: {TWIN}')
        assert np.array_equal(H(r['acc']) > 0.5, ref['acc'])                                # every chain: none is left out
        close(r['H0'], ref['H0'], rtol=1e-10, atol=0.0)
        close(r['x_new'], ref['x_new'], rtol=0.0, atol=1e-9)
        close(r['dH'], ref['dH'], rtol=1e-8, atol=1e-9)
        close(r['H1'], ref['H1'], rtol=1e-8, atol=0.0)
        close(r['csum'], ref['csum'], rtol=1e-10, atol=0.0)
        close(r['dsum'], ref['dsum'], rtol=1e-10, atol=1e-12)
        assert np.array_equal(H(r['Q']), ref['Q'])
        assert all(bits(run(c, path)[k], r[k]) for k in r)                                  # two calls, the same bits
    if len(res) == 2:                                                                       # path against path: within the same bounds
        a, b = res[1], res[2]
        assert bits(a['acc'], b['acc']) and bits(a['Q'], b['Q'])
        gpu_support.close(a['x_new'], b['x_new'], rtol=0.0, atol=1e-9)
        gpu_support.close(a['H0'], b['H0'], rtol=1e-10, atol=0.0)
        gpu_support.close(a['dH'], b['dH'], rtol=1e-8, atol=1e-9)
        gpu_support.close(a['H1'], b['H1'], rtol=1e-8, atol=0.0)
        assert all(bits(run(c, 0)[k], a[k]) for k in a)                                     # path 0 is path 1 where it is served
    else:
        assert all(bits(run(c, 0)[k], res[2][k]) for k in res[2])
    # aliased output on the sequenced path equals separate output, and path 0 takes it there
    xa = x.clone()
    ra = ops.defect_trajectory(xa, v, u, beta, g, df, DC.DT, nstep, integrator=integ, path=2, out={'x_new': xa})
    assert ra['x_new'].data_ptr() == xa.data_ptr() and all(bits(ra[k], res[2][k]) for k in ra)
    ra0 = ops.defect_trajectory(xa.copy_(x), v, u, beta, g, df, DC.DT, nstep, integrator=integ, path=0, out={'x_new': xa})
    assert all(bits(ra0[k], res[2][k]) for k in ra0)


@pytest.mark.parametrize('c', [c for c in DC.CASES if c[6] in ('wrap', 'full')], ids=DC.case_id)
def test_a_chain_of_a_batch_is_the_chain_alone_and_null_outputs_change_nothing(c):
    from fthmc_amd import _lib
    B, L, amp, beta, nstep, integ, dk = c
    x, v, u, g, df, ref = dev_case(c)
    for path in paths_of(L):
        r = run(c, path)
        for b in {0, B - 1}:
            one = run(c, path, sl=slice(b, b + 1))
            assert all(bits(one[k], r[k][b:b + 1]) for k in r), (path, b)
        # every optional output null: the same x_new
        xn = torch.empty_like(x)
        need = ops.defect_ws_bytes(B, L, path)
        ws, nb = ops._stream_buffer(x, need, 'defect') if need else (None, 0)
        rc = _lib.load().fthmc_defect_trajectory(ops._p(x), ops._p(v), ops._p(u), B, L, beta, ops._p(g), *df, DC.DT, nstep, _lib.INTEGRATORS[integ],
                                                 path, ops._p(xn), None, None, None, None, None, None, None, ws, nb, ops._stream(x))
        assert rc == 0 and bits(xn, r['x_new'])


def test_scratch_is_asked_for_only_on_the_sequenced_path():
    c = DC.CASES[1]
    B, L, amp, beta, nstep, integ, dk = c

    def keys():
        return [k for k in ops._WS if len(k) == 3 and k[2] == 'defect']
    ops.release_workspaces()
    run(c, 1); run(c, 0)
    assert keys() == []
    run(c, 2)
    assert len(keys()) == 1
    assert ops.defect_ws_bytes(B, L, 1) == 0 and ops.defect_ws_bytes(B, L, 2) == ops.defect_ws_bytes(B, L, 0) > ops.ws_bytes(B, L, 0)
    x, v, u, g, df, ref = dev_case(c)
    with pytest.raises(ValueError):
        ops.defect_trajectory(x, v, u, beta, g, df, 0.1, 1, path=1, out={'x_new': x})
    with pytest.raises(ValueError):
        ops.defect_trajectory(x, v, u, beta, g, (0, L, 1), 0.1, 1)
    with pytest.raises(ValueError):
        ops.defect_trajectory(x, v, u, beta, g, (0, 0, L + 1), 0.1, 1)


# ---------------------------------------------------------------- the translation
@pytest.mark.parametrize('B,L', [(5, 4), (6, 12), (4, 36), (3, 68)])
def test_translate_is_torch_roll_on_the_top_rung_and_a_copy_elsewhere(B, L):
    x = D(DC.links(B, L, 40 + L, np.pi))
    rng = np.random.default_rng(L)
    rung = torch.tensor([b % 3 for b in range(B)], dtype=torch.int32, device='cuda')
    sh = rng.integers(0, L, size=(B, 2))
    sh[0] = (0, L - 1); sh[min(3, B - 1)] = (L - 1, 0)                                     # shifts 0 and L - 1 on top-rung chains (b % 3 == 0)
    shift = torch.tensor(sh, dtype=torch.int32, device='cuda')
    out = ops.defect_translate(x, rung, 0, shift)
    tw = DC.translate(H(x), H(rung), 0, sh)
    assert bits(out, tw)
    for b in range(B):
        want = torch.roll(x[b], (int(sh[b][0]), int(sh[b][1])), dims=(1, 2)) if b % 3 == 0 else x[b]
        assert bits(out[b], want), b
    S0, Q0, p0 = ops.wilson_action_charge(x, 3.0)
    S1, Q1, p1 = ops.wilson_action_charge(out, 3.0)
    gpu_support.close(S1, S0, rtol=1e-12, atol=0.0)
    gpu_support.close(Q1, Q0, rtol=0.0, atol=1e-12)
    # into a caller's field; shifts beyond [0, L) are reduced; a rung nobody sits on copies everything; x itself is refused
    o2 = torch.empty_like(x)
    assert ops.defect_translate(x, rung, 0, shift + L, out=o2).data_ptr() == o2.data_ptr() and bits(o2, out)
    assert bits(ops.defect_translate(x, rung, 0, shift - 2 * L), out)
    assert bits(ops.defect_translate(x, rung, 7, shift), x)
    with pytest.raises(gpu_support.ops.FthmcError):
        ops.defect_translate(x, rung, 0, shift, out=x)


# ---------------------------------------------------------------- the driver
def _param(**kw):
    from fthmc_amd.config import Param
    return Param(**kw)


def _series(h):
    return {k: np.asarray(h[k]) for k in ('plaq', 'Q', 'acc', 'dH', 'dsum', 'swap_rounds', 'rung', 'round_trips')}


def test_run_ptbc_captured_equals_eager_and_a_hand_sequenced_iteration():
    from fthmc_amd.defect import run_ptbc, shift_seed
    from fthmc_amd.tempering import swap_seed
    L, K, M, ntraj = 8, 4, 2, 8
    par = _param(beta=3.0, L=L, tau=0.6, nstep=3, seed=5)
    cs = [0.0, 0.4, 0.75, 1.0]
    df = (6, 7, 4)
    x0 = D(DC.links(K * M, L, 79, 1.0))
    ha, hb = (run_ptbc(par, cs, M, ntraj, defect=df, integrator='omelyan', x=x0, captured=cap) for cap in (True, False))
    a, b = _series(ha), _series(hb)
    for k in a:
        assert a[k].shape == b[k].shape and bits(a[k].astype(np.float64), b[k].astype(np.float64)), k
    assert bits(ha['x'], hb['x']) and bits(ha['g_b'], hb['g_b']) and bits(ha['rung_last'], hb['rung_last'])
    assert a['plaq'].shape == (ntraj, K, M) and a['rung'].shape == (ntraj, K * M) and ha['swap_acc'].shape == (K - 1,)
    assert list(ha['cs']) == cs and tuple(ha['defect']) == df and (a['swap_rounds'] >= 0).any()
    # rung bookkeeping: every ladder holds every rung once at every trajectory, g_b follows the rung
    assert (np.sort(a['rung'].reshape(ntraj, M, K), axis=2) == np.arange(K)).all()
    assert np.array_equal(H(ha['g_b']), par.beta * np.array(cs)[H(ha['rung_last'])])
    # one hand-sequenced iteration: the first history rows, bit for bit
    B = K * M
    lad = ops.ladder_init([par.beta * c for c in cs], M, device='cuda')
    g_b, rung, chain_of = lad['beta_b'], lad['rung'], lad['chain_of']
    x = x0.clone()
    for t in range(2):
        seeds = ops.chain_seeds(par.seed, 0, B, t, device='cuda')
        v, u = ops.random_momenta(seeds, x.shape)
        r = ops.defect_trajectory(x, v, u, par.beta, g_b, df, par.tau / par.nstep, par.nstep, integrator='omelyan', path=0)
        rg = H(rung).astype(np.int64)
        order = (np.argsort(rg.reshape(M, K), axis=1) + (np.arange(M) * K)[:, None]).T      # [K, M] -> chain index
        assert np.array_equal(a['rung'][t], rg)
        assert bits(a['plaq'][t], H(r['csum'])[order] / float(L * L)) and bits(a['dsum'][t], H(r['dsum'])[order])
        assert bits(a['Q'][t], H(r['Q'])[order]) and bits(a['dH'][t], H(r['dH'])[order]) and bits(a['acc'][t], H(r['acc'])[order])
        us = ops.random_uniform(ops.chain_seeds(swap_seed(par.seed), 0, M, t, device='cuda'), (M, K - 1), 0.0, 1.0)
        sw = ops.replica_swap(lad['betas'], r['dsum'], us, g_b, rung, chain_of, t % 2)
        assert bits(a['swap_rounds'][t], sw['swap_acc'])
        co, rn = H(chain_of).reshape(M, K), H(rung).reshape(M, K)
        assert all(rn[m][co[m][k]] == k for m in range(M) for k in range(K))                # chain_of is the inverse of rung
        ush = ops.random_uniform(ops.chain_seeds(shift_seed(par.seed), 0, B, t, device='cuda'), (B, 2), 0.0, 1.0)
        shift = torch.floor(ush * float(L)).to(torch.int32)
        x = ops.defect_translate(r['x_new'], rung, K - 1, shift)
    # translate = False leaves the fields where the trajectories put them; the driver refuses what it documents
    hn = run_ptbc(par, cs, M, 2, defect=df, integrator='omelyan', x=x0, translate=False)
    assert bits(np.asarray(hn['plaq'])[0], a['plaq'][0]) and bits(np.asarray(hn['swap_rounds'])[0], a['swap_rounds'][0])
    for bad in ([0.0, 0.5], [0.5, 0.4, 1.0], [-0.1, 1.0], [1.0]):
        with pytest.raises(ValueError):
            run_ptbc(par, bad, M, 2)
    with pytest.raises(ValueError):
        run_ptbc(par, cs, M, 2, defect=(0, 0, L + 1))


# ---------------------------------------------------------------- physics: what the feature is for
def _jackknife(per_ladder):
    M = len(per_ladder)
    jk = (per_ladder.sum() - per_ladder) / (M - 1)
    return float(per_ladder.mean()), float(np.sqrt((M - 1) * np.mean((jk - jk.mean()) ** 2)))


def test_ptbc_unfreezes_the_charge_and_samples_the_periodic_rung():
    """L = 16, beta = 6 (plain HMC is frozen there), 32 ladders of K = 8 rungs linear in c (256 chains), a defect of 4 plaquettes, 600
    leapfrog trajectories (tau = 1, 10 steps) from a cold start, one captured run.  The averages leave out the first 100 trajectories, as
    the twin's sampler test does (tests/test_defect.py): a cold start has Q = 0 and cos P = 1 everywhere, and what it takes to forget that is
    a bias of the mean, not noise the error bar knows of (with all 600 the twin's <Q^2> sits 2.5 sigma low).  Of the other 500: <Q^2> of rung K - 1 within |z| <= 4
    of the exact 1.1947014482 (jackknife over the ladders), every rung's defect <cos P> within |z| <= 4 of exact_defect_plaquette, and
    more |dQ| per trajectory on the top rung than the top rung of tempered HMC over a ladder of beta that is as flat as a ladder may be."""
    from fthmc_amd.defect import run_ptbc
    from fthmc_amd.tempering import run_tempered
    from fthmc_amd.utils.observables import exact_defect_plaquette
    M, K, ntraj, therm, Ld = 32, 8, 600, 100, 4
    cs = [k / (K - 1) for k in range(K - 1)] + [1.0]
    par = _param(beta=6.0, L=16, tau=1.0, nstep=10, seed=29)
    h = run_ptbc(par, cs, M, ntraj, defect=(0, 0, Ld))
    Q = np.rint(np.asarray(h['Q'])[:, K - 1, :])                                            # [ntraj, M]
    q2, err = _jackknife((Q[therm:] ** 2).mean(axis=0))
    z = (q2 - Q2_EXACT_L16_B6) / err
    dq = float(np.abs(np.diff(Q, axis=0)).mean())
    ht = run_tempered(par, None, [6.0 - 1e-6 * (K - 1 - k) for k in range(K)], M, ntraj)
    Qt = np.rint(np.asarray(ht['Q'])[:, K - 1, :])
    dqt = float(np.abs(np.diff(Qt, axis=0)).mean())
    print(f'<Q^2> {q2:.4f} +- {err:.4f}, exact {Q2_EXACT_L16_B6:.4f}, z {z:+.2f}; |dQ| per trajectory {dq:.4f} against {dqt:.4f} tempered flat; '
          f'acceptance {float(np.asarray(h["acc"]).mean()):.3f}, swaps {np.round(h["swap_acc"], 3)}, round trips {int(h["round_trips"].sum())}')
    assert abs(z) <= 4.0
    assert dq > dqt and dq > 0.1
    dp = np.asarray(h['dsum'])[therm:] / Ld                                                 # [n, K, M]
    for k in range(K):
        m, e = _jackknife(dp[:, k, :].mean(axis=0))
        ex = exact_defect_plaquette(6.0, 16, cs[k], Ld)
        print(f'rung {k} c {cs[k]:.3f}: defect <cos P> {m:.4f} +- {e:.4f}, exact {ex:.4f}, z {(m - ex) / e:+.2f}')
        assert abs(m - ex) <= 4.0 * e, k
