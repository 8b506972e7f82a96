"""GPU tests that hold the kernels of boundary-condition tempering (csrc/defect.hip, defect_trajectory_call in csrc/api.hip) per site and
per chain at their launch edges, on hard inputs, inside bounds derived from the inputs (tests/defect_hard_cases.py;
tests/test_defect_hard.py shows on the CPU that the float64 twin meets every bound with no chain left out, and that twelve named defects
do not).

Shapes: batch (B 258, L 4: k_defect_energy's second workgroup and its guard), L36 and L60 (ragged passes of the 512-thread sums and of
the one-launch kernel's 1024 threads), L132 (the second pass of k_defect_gp, k_defect_force and k_defect_translate; sequenced path),
slice (B 65537, L 4: the second slice of chains of launch_defect_force and launch_defect_translate; force, action and translate only).
Defects: one, full, wrap, col0, end (a line that starts on the last row) and, at L = 132, a line across the pass edge at site 16384 and
one that starts behind it and wraps to the front.  Inputs: pinned links on chain 0, the last chain never regularized (|x| about 30),
momenta x 3; couplings mixed out of {0, beta / 3, beta}.  Every tolerance is an array from defect_hard_cases; nothing here is a bare
number.  Q and the accept flags are compared exactly on every chain.

Observed on an MI355X (worst |device - reference| / bound per case, and where it sits):
  force and action (F per site; S, csum, dsum per chain; Q equal on every chain)
  field batch-one             0.362 F[3,0,1,2]         (F 0.362 S 0.036 csum 0.029 dsum 0.185)
  field batch-full            0.335 F[191,0,1,2]       (F 0.335 S 0.025 csum 0.029 dsum 0.059)
  field batch-wrap            0.438 F[81,1,0,3]        (F 0.438 S 0.033 csum 0.033 dsum 0.105)
  field batch-col0            0.507 F[85,0,0,1]        (F 0.507 S 0.024 csum 0.024 dsum 0.084)
  field batch-end             0.395 F[107,0,1,3]       (F 0.395 S 0.027 csum 0.033 dsum 0.083)
  field L36-wrap              0.330 F[1,0,9,25]        (F 0.330 S 0.000 csum 0.000 dsum 0.009)
  field L36-col0              0.275 F[0,0,16,15]       (F 0.275 S 0.001 csum 0.001 dsum 0.027)
  field L36-end               0.330 F[0,1,16,18]       (F 0.330 S 0.001 csum 0.001 dsum 0.006)
  field L60-one               0.290 F[0,1,47,32]       (F 0.290 S 0.002 csum 0.002 dsum 0.101)
  field L60-full              0.366 F[0,0,57,58]       (F 0.366 S 0.000 csum 0.000 dsum 0.010)
  field L60-end               0.292 F[1,1,55,1]        (F 0.292 S 0.001 csum 0.001 dsum 0.019)
  field L132-full             0.360 F[0,0,27,49]       (F 0.360 S 0.000 csum 0.000 dsum 0.005)
  field L132-end              0.396 F[0,0,108,124]     (F 0.396 S 0.000 csum 0.000 dsum 0.006)
  field L132-straddle         0.382 F[0,1,44,55]       (F 0.382 S 0.000 csum 0.000 dsum 0.025)
  field L132-wrapback         0.383 F[1,1,70,106]      (F 0.383 S 0.001 csum 0.001 dsum 0.017)
  field slice-wrap            0.622 F[7675,0,3,0]      (F 0.622 S 0.053 csum 0.055 dsum 0.116)
  field slice-end             0.625 F[44573,0,3,0]     (F 0.625 S 0.045 csum 0.042 dsum 0.126)
  trajectories (the worst of x_new per link and H0, H1, dH, csum, dsum per chain)
  batch-one-n1-leapfrog             path 1 0.448 x_new[58,0,3,3]       path 2 0.448 x_new[58,0,3,3]
  batch-one-n2-omelyan              path 1 0.427 x_new[210,1,0,3]      path 2 0.427 x_new[210,1,0,3]
  batch-full-n1-force_gradient      path 1 0.434 x_new[115,1,3,3]      path 2 0.434 x_new[115,1,3,3]
  batch-full-n2-leapfrog            path 1 0.484 x_new[115,1,3,3]      path 2 0.484 x_new[115,1,3,3]
  batch-wrap-n1-omelyan             path 1 0.510 x_new[183,0,3,0]      path 2 0.510 x_new[183,0,3,0]
  batch-wrap-n2-force_gradient      path 1 0.373 x_new[227,1,3,3]      path 2 0.373 x_new[227,1,3,3]
  batch-col0-n1-leapfrog            path 1 0.478 x_new[217,0,0,0]      path 2 0.478 x_new[217,0,0,0]
  batch-col0-n2-omelyan             path 1 0.435 x_new[224,0,0,2]      path 2 0.435 x_new[224,0,0,2]
  batch-end-n1-force_gradient       path 1 0.429 x_new[106,0,1,0]      path 2 0.429 x_new[106,0,1,0]
  batch-end-n2-leapfrog             path 1 0.424 x_new[179,1,1,3]      path 2 0.424 x_new[179,1,1,3]
  L36-wrap-n1-omelyan               path 1 0.432 x_new[0,1,3,24]       path 2 0.432 x_new[0,1,3,24]
  L36-wrap-n2-force_gradient        path 1 0.417 x_new[0,0,21,18]      path 2 0.417 x_new[0,0,21,18]
  L36-col0-n1-leapfrog              path 1 0.487 x_new[1,0,11,30]      path 2 0.487 x_new[1,0,11,30]
  L36-col0-n2-omelyan               path 1 0.398 x_new[0,0,17,11]      path 2 0.398 x_new[0,0,17,11]
  L36-end-n1-force_gradient         path 1 0.446 x_new[0,1,27,9]       path 2 0.446 x_new[0,1,27,9]
  L36-end-n2-leapfrog               path 1 0.430 x_new[0,1,8,19]       path 2 0.430 x_new[0,1,8,19]
  L60-one-n1-omelyan                path 1 0.463 x_new[1,1,25,1]       path 2 0.463 x_new[1,1,25,1]
  L60-one-n2-force_gradient         path 1 0.434 x_new[0,1,12,52]      path 2 0.434 x_new[0,1,12,52]
  L60-full-n1-leapfrog              path 1 0.470 x_new[0,0,52,18]      path 2 0.470 x_new[0,0,52,18]
  L60-full-n2-omelyan               path 1 0.439 x_new[0,0,12,50]      path 2 0.439 x_new[0,0,12,50]
  L60-end-n1-force_gradient         path 1 0.308 x_new[1,0,13,55]      path 2 0.308 x_new[1,0,13,55]
  L60-end-n2-leapfrog               path 1 0.450 x_new[1,1,32,55]      path 2 0.450 x_new[1,1,32,55]
  L132-full-n1-leapfrog             path 2 0.486 x_new[0,1,7,24]
  L132-full-n1-force_gradient       path 2 0.446 x_new[0,0,125,31]
  L132-end-n1-leapfrog              path 2 0.467 x_new[0,0,93,83]
  L132-end-n1-force_gradient        path 2 0.485 x_new[0,0,112,125]
  L132-straddle-n1-leapfrog         path 2 0.517 x_new[1,0,72,106]
  L132-straddle-n1-force_gradient   path 2 0.466 x_new[0,0,87,2]
  L132-wrapback-n1-leapfrog         path 2 0.459 x_new[0,1,12,44]
  L132-wrapback-n1-force_gradient   path 2 0.479 x_new[0,0,64,121]
  the largest of all: 0.625; accept flags and Q equal the reference's on every chain of every case
"""
import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401

import defect_hard_cases as DH

from gpu_support import D, H, module_defaults, ops

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

BETA, DT = DH.BETA, DH.DT
TRAJ_KEYS = ('x_new', 'dH', 'acc', 'H0', 'H1', 'csum', 'dsum', 'Q')


def bits(a, b):
    a, b = H(a), H(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def same(r, s, keys=TRAJ_KEYS):
    return [k for k in keys if not bits(r[k], s[k])]


def show(tag, f):
    w, k, at = DH.worst_of(f)
    print(f'OBSERVED {tag}: {w:.4f} at {k}{list(at)}  ' + ' '.join(f'{k} {v[0]:.3f}' for k, v in f.items()))
    return w


def dev_field(x, g, df):
    xd, gd = D(x), D(g)
    S, C, Dm, Q = ops.defect_action(xd, BETA, gd, df)
    return {'F': H(ops.defect_force(xd, BETA, gd, df)), 'S': H(S), 'csum': H(C), 'dsum': H(Dm), 'Q': H(Q)}


def traj(T, c, path, sl=None, g=None, out=None):
    """the case's trajectory on `path`; sl: a slice of chains run alone; g: other couplings"""
    sl = slice(None) if sl is None else sl
    x, v, u = (D(a[sl]) for a in (T.x, T.v, T.u))
    gd = D(T.g[sl]) if g is None else g
    return ops.defect_trajectory(x, v, u, BETA, gd, T.df, DT, c.nstep, integrator=c.integrator, path=path, out=out)


def parent_in_place(x, v, u, beta_b, dt, nstep, integ):
    """the parent's sequenced per-chain-beta trajectory: fthmc_hmc_trajectory_pb with x_new aliasing x (tests/test_z_defect_gpu.py)"""
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


# ---------------------------------------------------------------- force and action: per site, per chain
@pytest.mark.parametrize('c', DH.FIELD_CASES, ids=DH.field_id)
def test_force_per_site_and_action_per_chain(c):
    ref = DH.field_reference(c)
    assert ref['decided'].all()
    f, ok = DH.field_fracs(dev_field(ref['x'], ref['g'], ref['df']), ref)
    assert show(f'field {DH.field_id(c)}', f) <= 1.0 and ok, f


# ---------------------------------------------------------------- trajectories
@pytest.mark.parametrize('c', DH.CASES, ids=DH.case_id)
def test_trajectory_inside_the_propagated_bounds_on_every_path(c):
    T = DH.traj_reference(c)
    res = {}
    for path in c.paths:
        r = res[path] = traj(T, c, path)
        f, ok = DH.traj_fracs({k: H(r[k]) for k in TRAJ_KEYS}, T)
        w = show(f'trajectory {DH.case_id(c)} path {path}', f)
        assert ok and w <= 1.0, (path, f)                                    # accept flags and Q: the reference's on every chain
        assert not same(traj(T, c, path), r), path                           # two calls, the same bits
    served = res[c.paths[0]]                                                 # path 0: the one-launch kernel where it serves the shape
    assert not same(traj(T, c, 0), served)
    xa = D(T.x)
    ra = ops.defect_trajectory(xa, D(T.v), D(T.u), BETA, D(T.g), T.df, DT, c.nstep, integrator=c.integrator, path=2, out={'x_new': xa})
    assert ra['x_new'].data_ptr() == xa.data_ptr() and not same(ra, res[2])  # aliased output on the sequenced path


BATCH = [c for c in DH.CASES if c.shape == 'batch']


@pytest.mark.parametrize('c', BATCH, ids=DH.case_id)
def test_a_chain_of_the_batch_equals_the_chain_alone(c):
    """chains 0, 255, 256, 257 of 258 (either side of k_defect_energy's workgroup edge), on both paths; force and action as well"""
    T = DH.traj_reference(c)
    chains = (0, 255, 256, 257)
    for path in c.paths:
        r = traj(T, c, path)
        for b in chains:
            one = traj(T, c, path, sl=slice(b, b + 1))
            assert not same(one, {k: r[k][b:b + 1] for k in TRAJ_KEYS}), (path, b)
    xd, gd = D(T.x), D(T.g)
    F = ops.defect_force(xd, BETA, gd, T.df)
    A = ops.defect_action(xd, BETA, gd, T.df)
    for b in chains:
        assert bits(ops.defect_force(xd[b:b + 1].clone(), BETA, gd[b:b + 1].clone(), T.df), F[b:b + 1])
        one = ops.defect_action(xd[b:b + 1].clone(), BETA, gd[b:b + 1].clone(), T.df)
        assert all(bits(one[k], A[k][b:b + 1]) for k in range(4)), b


@pytest.mark.parametrize('c', BATCH, ids=DH.case_id)
def test_periodic_coupling_on_the_batch_gives_the_per_chain_beta_trajectory_bit_for_bit(c):
    """g_b = beta on all 258 chains: ops.hmc_trajectory with a beta tensor on path 1 (the one-launch kernel), the parent's sequenced
    per-chain-beta trajectory on path 2, as tests/test_z_defect_gpu.py checks at B <= 5"""
    T = DH.traj_reference(c)
    bb = torch.full((c.B,), BETA, dtype=torch.float64, device='cuda')
    x, v, u = D(T.x), D(T.v), D(T.u)
    for path in c.paths:
        r = traj(T, c, path, g=bb)
        p = ops.hmc_trajectory(x, v, u, bb, DT, c.nstep, integrator=c.integrator) if path == 1 else parent_in_place(x, v, u, bb, DT, c.nstep, c.integrator)
        assert not same(r, p, ('x_new', 'dH', 'acc', 'H0', 'H1')), path


# ---------------------------------------------------------------- the translation
def rolled(x, b, s):
    return torch.roll(x[b], (int(s[0]), int(s[1])), dims=(1, 2))


def test_translate_past_one_pass_is_torch_roll_and_the_twin_bit_for_bit():
    """L = 132: 1040 output sites of every plane in k_defect_translate's second pass; shifts 0, L - 1, negative, >= L"""
    t = DH.translate_case('L132')
    x, rung = D(t.x), torch.tensor(t.rung, dtype=torch.int32, device='cuda')
    for s in DH.L132_SHIFTS:
        sh = np.array([s, (3, 3)], dtype=np.int32)
        out = ops.defect_translate(x, rung, t.top, torch.tensor(sh, dtype=torch.int32, device='cuda'))
        assert bits(out, DH.t_translate(t.x, t.rung, t.top, sh)), s
        assert bits(out[0], rolled(x, 0, s)) and bits(out[1], x[1]), s
    assert bits(ops.defect_translate(x, rung, 9, torch.tensor(sh, dtype=torch.int32, device='cuda')), x)       # a rung nobody sits on


def test_translate_past_one_slice_of_chains_is_torch_roll_and_the_twin_bit_for_bit():
    """B = 65537: chains 65535 and 65536 in launch_defect_translate's second slice; 65534 and 65535 on the top rung with different
    non-zero shifts, 65533 and 65536 not"""
    t = DH.translate_case('slice')
    x, rung = D(t.x), torch.tensor(t.rung, dtype=torch.int32, device='cuda')
    shift = torch.tensor(t.shift, dtype=torch.int32, device='cuda')
    out = ops.defect_translate(x, rung, t.top, shift)
    assert bits(out, DH.t_translate(t.x, t.rung, t.top, t.shift))
    on = np.flatnonzero(t.rung == t.top)
    for b in np.concatenate([on[:8], on[-8:], [DH.SLICE - 1, DH.SLICE]]):
        assert bits(out[b], rolled(x, b, t.shift[b])), b
    for b in (1, DH.SLICE - 2, DH.SLICE + 1):
        assert t.rung[b] != t.top and bits(out[b], x[b]), b
    assert bits(ops.defect_translate(x, rung, 9, shift), x)                                                     # a rung nobody sits on
