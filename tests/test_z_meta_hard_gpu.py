"""GPU tests that hold the metadynamics kernels (csrc/meta.hip, the biased hmc_trajectory_call in csrc/api.hip) per site and per chain at their
launch edges, on hard inputs, inside bounds derived from the inputs (tests/meta_hard_cases.py; tests/test_meta_hard.py shows on the
CPU that the float64 twin meets every bound with no chain and no lookup left out, and that twelve named defects do not).

Shapes: rows (B 6, L 8, G 2 and 3: the row map at 1 < G < B), batch (B 258, L 4, G 1, 3, 258: k_meta_energy's second workgroup and its
guard), L36 and L60 (ragged passes of the 512-thread sums and of the one-launch kernel's 1024 threads), L132 (the second pass of
k_meta_gp's grid-stride loop, sequenced path).  Inputs: pinned links on chain 0, the last chain never regularized (|x| about 30),
momenta x 3.  Placement: chains on either wall, in the first and the last interval, 1e-6 either side of a node, against nb = 41 and
nb = 2; the zero field on a node.  Every tolerance is an array from meta_hard_cases; nothing here is a bare number.

Observed on an MI355X (worst |device - reference| / bound per case, and where it sits):
  force and action (F per site; S, qm, vbias per chain)
  field rows-G2-rough                       0.181 F[0,1,7,1]          (F 0.181 S 0.009 qm 0.008 vbias 0.009)
  field rows-G2-quad                        0.281 F[3,1,7,3]          (F 0.281 S 0.014 qm 0.008 vbias 0.009)
  field rows-G3-rough                       0.144 F[5,1,3,3]          (F 0.144 S 0.009 qm 0.017 vbias 0.019)
  field rows-G3-quad                        0.189 F[5,0,6,5]          (F 0.189 S 0.020 qm 0.017 vbias 0.009)
  field batch-G1-rough                      0.265 F[13,0,2,0]         (F 0.265 S 0.029 qm 0.042 vbias 0.117)
  field batch-G3-rough                      0.244 F[177,1,1,1]        (F 0.244 S 0.025 qm 0.037 vbias 0.078)
  field batch-G258-rough                    0.376 vbias[190]          (F 0.229 S 0.029 qm 0.042 vbias 0.376)
  field L36-G2-rough                        0.024 F[1,0,20,31]        (F 0.024 S 0.001 qm 0.002 vbias 0.002)
  field L60-G1-rough                        0.023 F[1,1,28,41]        (F 0.023 S 0.001 qm 0.001 vbias 0.001)
  field L60-G1-quad                         0.250 F[0,1,25,1]         (F 0.250 S 0.001 qm 0.001 vbias 0.001)
  field L132-G2-rough                       0.056 F[1,0,64,56]        (F 0.056 S 0.000 qm 0.000 vbias 0.000)
  placement nb=41                           0.175 F[2,0,4,3]          (F 0.175 S 0.006 qm 0.009 vbias 0.008)
  placement nb=2                            0.777 vbias[5]            (F 0.143 S 0.003 qm 0.002 vbias 0.777)
  trajectories (the worst of x_new per link and H0, H1, dH, qm, vbias per chain)
  rows-G2-rough-n1-leapfrog                 path 1 0.459 x_new[5,0,4,2]        path 2 0.459 x_new[5,0,4,2]
  rows-G2-rough-n2-omelyan                  path 1 0.276 x_new[4,0,3,3]        path 2 0.276 x_new[4,0,3,3]
  rows-G2-quad-n1-force_gradient            path 1 0.369 x_new[0,1,4,7]        path 2 0.369 x_new[0,1,4,7]
  rows-G2-quad-n2-leapfrog                  path 1 0.340 x_new[2,1,7,1]        path 2 0.340 x_new[2,1,7,1]
  rows-G3-rough-n1-omelyan                  path 1 0.455 x_new[5,1,0,4]        path 2 0.455 x_new[5,1,0,4]
  rows-G3-rough-n2-force_gradient           path 1 0.278 x_new[3,1,1,4]        path 2 0.278 x_new[3,1,1,4]
  rows-G3-quad-n1-leapfrog                  path 1 0.433 x_new[4,0,1,2]        path 2 0.433 x_new[4,0,1,2]
  rows-G3-quad-n2-omelyan                   path 1 0.383 x_new[4,1,6,6]        path 2 0.383 x_new[4,1,6,6]
  batch-G1-rough-n1-force_gradient          path 1 0.443 x_new[74,0,2,3]       path 2 0.443 x_new[74,0,2,3]
  batch-G1-rough-n2-leapfrog                path 1 0.428 x_new[96,0,3,0]       path 2 0.428 x_new[96,0,3,0]
  batch-G3-rough-n1-omelyan                 path 1 0.435 x_new[213,0,1,2]      path 2 0.435 x_new[213,0,1,2]
  batch-G3-rough-n2-force_gradient          path 1 0.374 x_new[226,1,3,2]      path 2 0.374 x_new[226,1,3,2]
  batch-G258-rough-n1-leapfrog              path 1 0.450 x_new[205,1,3,3]      path 2 0.450 x_new[205,1,3,3]
  batch-G258-rough-n2-omelyan               path 1 0.376 vbias[190]            path 2 0.376 vbias[190]
  L36-G2-rough-n1-force_gradient            path 1 0.172 x_new[0,1,13,1]       path 2 0.172 x_new[0,1,13,1]
  L36-G2-rough-n2-leapfrog                  path 1 0.161 x_new[0,0,3,31]       path 2 0.161 x_new[0,0,3,31]
  L60-G1-rough-n1-omelyan                   path 1 0.180 x_new[0,1,7,59]       path 2 0.180 x_new[0,1,7,59]
  L60-G1-rough-n2-force_gradient            path 1 0.019 x_new[0,0,47,57]      path 2 0.019 x_new[0,0,47,57]
  L60-G1-quad-n1-leapfrog                   path 1 0.225 x_new[0,0,18,4]       path 2 0.225 x_new[0,0,18,4]
  L60-G1-quad-n2-omelyan                    path 1 0.025 H0[0]                 path 2 0.025 H0[0]
  L132-G2-rough-n1-leapfrog                 path 2 0.004 H0[0]
  L132-G2-rough-n1-force_gradient           path 2 0.072 x_new[0,1,50,22]
  the largest of all: 0.777; accept flags equal the reference's on every chain of every case
"""
import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401

import meta_cases as MC
import meta_hard_cases as MH
import stencil_cases as SC

from gpu_support import D, H, module_defaults, ops

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

BETA, DT = MH.BETA, MH.DT
TRAJ_KEYS = ('x_new', 'dH', 'acc', 'H0', 'H1', 'qm', 'vbias')


def bits(a, b):
    a, b = H(a), H(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def same(r, s, keys=TRAJ_KEYS):
    return [k for k in keys if not bits(r[k], s[k])]


def show(tag, f):
    w, k, at = MH.worst_of(f)
    print(f'OBSERVED {tag}: {w:.4f} at {k}{list(at)}  ' + ' '.join(f'{k} {v[0]:.3f}' for k, v in f.items()))
    return w


def dev_field(x, tab):
    xd, V = D(x), D(tab.V)
    S, qm, vb = ops.meta_action(xd, BETA, V, tab.qmax, tab.wall)
    return {'F': H(ops.meta_force(xd, BETA, V, tab.qmax, tab.wall)), 'S': H(S), 'qm': H(qm), 'vbias': H(vb)}


def traj(T, c, path, sl=None, V=None, out=None):
    """the case's trajectory on `path`; sl: a slice of chains run alone against the table rows V"""
    sl = slice(None) if sl is None else sl
    x, v, u = (D(a[sl]) for a in (T.x, T.v, T.u))
    V = D(T.tab.V) if V is None else V
    return ops.meta_trajectory(x, v, u, BETA, DT, c.nstep, V, T.tab.qmax, T.tab.wall, integrator=c.integrator, path=path, out=out)


# ---------------------------------------------------------------- force and action: per site, per chain
@pytest.mark.parametrize('c', MH.FIELD_CASES, ids=MH.field_id)
def test_force_per_site_and_action_per_chain(c):
    ref = MH.field_reference(c)
    assert ref['decided'].all()
    f = MH.field_fracs(dev_field(ref['x'], ref['tab']), ref)
    assert show(f'field {MH.field_id(c)}', f) <= 1.0, f


@pytest.mark.parametrize('nb', MH.PLACEMENTS)
def test_placed_chains_walls_end_intervals_and_either_side_of_a_node(nb):
    p, ref = MH.placement(nb), MH.placement_reference(nb)
    assert ref['decided'].all()
    f = MH.field_fracs(dev_field(p.x, p.tab), ref)
    assert show(f'placement nb={nb}', f) <= 1.0, f


def test_zero_field_returns_the_nodes_height_and_a_zero_force_in_every_bit():
    x, tab, node = MH.zero_field()
    got = dev_field(x, tab)
    assert bits(got['vbias'], tab.V[np.arange(len(x)), node]) and not SC.bits(got['qm']).any()
    assert not SC.bits(got['F']).any()
    assert bits(got['S'], MH.field_twin(x, tab)['S'])


# ---------------------------------------------------------------- trajectories
@pytest.mark.parametrize('c', MH.CASES, ids=MH.case_id)
def test_trajectory_inside_the_propagated_bounds_on_every_path(c):
    T = MH.traj_reference(c)
    res = {}
    for path in c.paths:
        r = res[path] = traj(T, c, path)
        f, ok = MH.traj_fracs({k: H(r[k]) for k in TRAJ_KEYS}, T)
        w = show(f'trajectory {MH.case_id(c)} path {path}', f)
        assert ok and w <= 1.0, (path, f)
        assert not same(traj(T, c, path), r), path                           # two calls, the same bits
    served = res[c.paths[0]]                                                 # path 0: the one-launch kernel where it serves the shape
    assert not same(traj(T, c, 0), served)
    xa = D(T.x)
    ra = ops.meta_trajectory(xa, D(T.v), D(T.u), BETA, DT, c.nstep, D(T.tab.V), T.tab.qmax, T.tab.wall, integrator=c.integrator, path=2,
                             out={'x_new': xa})
    assert ra['x_new'].data_ptr() == xa.data_ptr() and not same(ra, res[2])  # aliased output on the sequenced path


BATCH_ALONE = [c for c in MH.CASES if c.shape == 'batch']        # G = 1, 3 (chains 256, 257 read row 2) and 258; alone: B = G = 1
ROWS = [c for c in MH.CASES if c.shape == 'rows']


@pytest.mark.parametrize('c', BATCH_ALONE + ROWS, ids=MH.case_id)
def test_a_chain_of_the_batch_equals_the_chain_alone_with_its_row(c):
    """batch: chains 0, 255, 256, 257 of 258 (either side of k_meta_energy's workgroup edge); rows: every chain, with the row the map
    b / (B / G) gives it"""
    T = MH.traj_reference(c)
    rows = T.tab.rows(c.B)
    chains = (0, 255, 256, 257) if c.shape == 'batch' else range(c.B)
    for path in c.paths:
        r = traj(T, c, path)
        for b in chains:
            one = traj(T, c, path, sl=slice(b, b + 1), V=D(T.tab.V[rows[b]:rows[b] + 1]))
            assert not same(one, {k: r[k][b:b + 1] for k in TRAJ_KEYS}), (path, b)
    xd, V = D(T.x), D(T.tab.V)
    F = ops.meta_force(xd, BETA, V, T.tab.qmax, T.tab.wall)
    S, qm, vb = ops.meta_action(xd, BETA, V, T.tab.qmax, T.tab.wall)
    for b in chains:
        Vb = D(T.tab.V[rows[b]:rows[b] + 1])
        assert bits(ops.meta_force(xd[b:b + 1].clone(), BETA, Vb, T.tab.qmax, T.tab.wall), F[b:b + 1])
        one = ops.meta_action(xd[b:b + 1].clone(), BETA, Vb, T.tab.qmax, T.tab.wall)
        assert bits(one[0], S[b:b + 1]) and bits(one[1], qm[b:b + 1]) and bits(one[2], vb[b:b + 1]), b


NULL_CASES = [next(c for c in MH.CASES if c.shape == s) for s in ('rows', 'batch', 'L36', 'L132')]


@pytest.mark.parametrize('c', NULL_CASES, ids=MH.case_id)
def test_every_optional_output_null_gives_the_same_x_new(c):
    """through the C ABI (ops.meta_trajectory always passes dH .. vb_out): all six null, on every path that serves the shape"""
    from fthmc_amd import _lib
    T = MH.traj_reference(c)
    x, v, u, V = D(T.x), D(T.v), D(T.u), D(T.tab.V)
    for path in c.paths:
        full = traj(T, c, path)
        xn = torch.full_like(x, float('nan'))
        ws, nbytes = ops._meta_ws(x, ops.meta_ws_bytes(c.B, c.L, 2)) if path == 2 else (None, 0)
        rc = _lib.load().fthmc_meta_trajectory(ops._p(x), ops._p(v), ops._p(u), c.B, c.L, BETA, DT, c.nstep, _lib.INTEGRATORS[c.integrator],
                                               ops._p(V), c.G, T.tab.nb, T.tab.qmax, T.tab.wall, path, ops._p(xn), None, None, None, None,
                                               None, None, ws, nbytes, ops._stream(x))
        assert rc == 0
        torch.cuda.synchronize()
        assert bits(xn, full['x_new']), path


# ---------------------------------------------------------------- deposit where the launch shape changes
@pytest.mark.parametrize('cpr', (300, 257))
def test_deposit_over_two_node_blocks_and_a_short_last_chunk(cpr):
    """G = 3 rows of cpr walkers into nb = 300 nodes: two workgroups on grid y (256 + 44 nodes), two chunks of walkers (256 + 44, or
    256 + 1).  A NaN walker and walkers outside on either side in each chunk; row 1's walkers are all outside or NaN: it keeps its
    bits.  The one walker of the 256 + 1 tail is NaN in row 0 and, in row 2, sits where walker 3 of the first chunk sits: its hill
    lands on two nodes that chunk already raised, and the table must differ there -- and only there -- from what the first 256
    walkers alone leave.  Bit for bit meta_cases.Table.deposit (chain order)."""
    G, nb, qmax, w = 3, 300, 2.0, 0.0625 + 2.0 ** -30
    nchunk = -(-cpr // 256)
    assert -(-nb // 256) == 2 and nchunk == 2 and cpr - 256 == {300: 44, 257: 1}[cpr]
    rng = np.random.default_rng(44000 + cpr)
    q = rng.uniform(-qmax, qmax, (G, cpr))
    q[:, 1], q[:, 5], q[:, 9] = np.nan, 2.5, -2.5                              # the first chunk
    if cpr == 300:
        q[:, 256 + 1], q[:, 256 + 5], q[:, 256 + 9] = np.nan, 2.5, -2.5        # the second chunk
        q[:, 256 + 20] = q[:, 3]                                               # a node met from both chunks
    else:
        q[0, 256], q[2, 256] = np.nan, q[2, 3]                                 # the one walker of the last chunk
    q[1] = np.where(np.arange(cpr) % 3 == 0, np.nan, np.where(np.arange(cpr) % 3 == 1, qmax, -qmax - 1e-9))
    q[0, 20], q[0, 21] = -qmax, np.nextafter(qmax, 0)                          # the first node, the last interval
    V0 = rng.normal(size=(G, nb))
    tab = MC.Table(V0, qmax, 0.0).deposit(q.reshape(-1), w)
    Vd = D(V0)
    ops.meta_deposit(D(q.reshape(-1)), Vd, qmax, w)
    assert bits(Vd, tab.V)
    assert bits(Vd[1], V0[1]) and not bits(Vd[0], V0[0]) and not bits(Vd[2], V0[2])
    assert (H(Vd)[0, 256:] != V0[0, 256:]).any() and (H(Vd)[0, :256] != V0[0, :256]).any()      # both node blocks were written
    # what the last chunk adds: the table of the first 256 walkers of every row alone differs from the device's where its hills land
    head = q.copy()
    head[:, 256:] = np.nan
    diff = H(Vd) != MC.Table(V0, qmax, 0.0).deposit(head.reshape(-1), w).V
    if cpr == 257:
        inside, i, f, _, _ = MC.Table(V0, qmax, 0.0).locate(q[2, 256:], np.float64)
        assert inside[0] and 0.0 < f[0] < 1.0 and np.flatnonzero(diff[2]).tolist() == [i[0], i[0] + 1] and not diff[:2].any()
    else:
        assert diff[0].sum() > 40 and diff[2].sum() > 40 and not diff[1].any()
    ops.meta_deposit(D(q.reshape(-1)), Vd, qmax, w)                            # on top of itself: the table is read in place
    assert bits(Vd, tab.deposit(q.reshape(-1), w).V)
