"""CPU checks behind tests/test_z_meta_hard_gpu.py (tests/meta_hard_cases.py): the float64 twin of the metadynamics kernels, in their
operation and summation order, stays inside every derived bound against the long double reference on every committed case with no
chain and no lookup left out -- the proof that the inputs can meet the bounds without the device --; every named mutant of the twin
leaves a bound on the case named for it here; the shapes reach the launch edges they claim, computed from the launchers' arithmetic;
the placement tables put each chain where they say, by margin; the reference here and meta_cases' long double twin state the same
operations."""
import math

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401

import batch_kernel_cases as BC
import integrator_cases as IC
import meta_cases as MC
import meta_hard_cases as MH
import stencil_cases as SC

LD = MH.LD


def show(tag, f):
    w, k, at = MH.worst_of(f)
    print(f'{tag}: worst {w:.4f} of the bound at {k}{list(at)}  ' + ' '.join(f'{k} {v[0]:.3f}' for k, v in f.items()))
    return w


def test_reference_is_extended_precision():
    assert np.finfo(np.longdouble).nmant == 63


# ---------------------------------------------------------------- the twin inside the bounds, nothing left out
@pytest.mark.parametrize('c', MH.FIELD_CASES, ids=MH.field_id)
def test_twin_force_and_action_inside_the_bounds(c):
    ref = MH.field_reference(c)
    assert ref['decided'].all(), np.flatnonzero(~ref['decided'])
    w = show(f'TWIN field {MH.field_id(c)}', MH.field_fracs(MH.field_twin(ref['x'], ref['tab']), ref))
    assert w <= 1.0


@pytest.mark.parametrize('c', MH.CASES, ids=MH.case_id)
def test_twin_trajectory_inside_the_bounds_and_nothing_is_left_out(c):
    T = MH.traj_reference(c)
    assert T.lookups_decided.all() and T.accept_decided.all()
    f, ok = MH.traj_fracs(MH.traj_twin(c), T)
    w = show(f'TWIN trajectory {MH.case_id(c)} (seed redrawn {T.redraws} times, accepted {int(T.acc.sum())} of {c.B})', f)
    assert ok and w <= 1.0


@pytest.mark.parametrize('nb', MH.PLACEMENTS)
def test_placement_tables_put_each_chain_where_they_say(nb):
    p = MH.placement(nb)
    ref = MH.placement_reference(nb)
    lk = ref['look']
    t, d = MH.f64(lk.t), MH.f64(lk.d)
    print(f'PLACEMENT nb={nb}: qmax {p.tab.qmax:.6f} node {p.k}  t {np.array2string(t, precision=7)}  d {np.array2string(d, precision=7)}')
    assert ref['decided'].all()
    assert not lk.inside[0] and d[0] > 0.1 and MH.f64(ref['qm'][0])[0] > 0                  # the positive wall
    assert not lk.inside[1] and d[1] > 0.1 and MH.f64(ref['qm'][0])[1] < 0                  # the negative wall
    assert lk.inside[2] and lk.i[2] == 0 and lk.inside[3] and lk.i[3] == nb - 2              # the first and the last interval
    for b in (2, 3):
        assert abs(t[b] - round(t[b])) >= 0.1 - 1e-12
    # 1e-6 in t on either side of node k, to 1e-3 of that; the margin condition holds by a factor > 1e6
    assert abs((p.k - t[4]) / MH.NODE_OFFSET - 1) < 1e-3 and abs((t[5] - p.k) / MH.NODE_OFFSET - 1) < 1e-3
    assert lk.inside[4] and lk.i[4] == p.k - 1
    if nb == 2:                                  # node 1 ends the table: chain 5 is on the wall, 2e-6 qmax out
        assert p.k == 1 and not lk.inside[5] and abs(d[5] / (2 * MH.NODE_OFFSET * p.tab.qmax) - 1) < 1e-3
    else:
        assert lk.inside[5] and lk.i[5] == p.k and 0 < p.k < nb - 1
    assert np.all(MH.NODE_OFFSET > 1e6 * lk.et[4:6])
    # chain 5 is chain 4 but for one link
    assert int((p.x[4] != p.x[5]).sum()) == 1
    w = show(f'TWIN placement nb={nb}', MH.field_fracs(MH.field_twin(p.x, p.tab), ref))
    assert w <= 1.0


def test_zero_field_lands_on_a_node_with_zero_force():
    x, tab, node = MH.zero_field()
    assert node == 20
    tw = MH.field_twin(x, tab)
    assert np.array_equal(SC.bits(tw['vbias']), SC.bits(tab.V[np.arange(6), node])) and not tw['qm'].any()
    assert not SC.bits(tw['F']).any()
    assert np.all(tw['S'] == -MH.BETA * 64 + tab.V[np.arange(6), node])


# ---------------------------------------------------------------- the two references state the same thing
@pytest.mark.parametrize('c', [c for c in MH.FIELD_CASES if c.shape in ('rows', 'L36')], ids=MH.field_id)
def test_reference_agrees_with_the_long_double_twin_of_meta_cases(c):
    """meta_cases divides by the long double pi and the unrounded delta, the reference here by the device's doubles (<= 0.6 u relative
    in Q_m, t and c): the two agree inside the bounds; and meta_cases.trajectory with the same schedule gives the same accepts"""
    ref = MH.field_reference(c)
    F, _ = MC.force(ref['x'], MH.BETA, ref['tab'], LD)
    S, q, V, _ = MC.biased_action(ref['x'], MH.BETA, ref['tab'], LD)
    f = {'F': MH.worst(MH.f64(F), ref['F']), 'S': MH.worst(MH.f64(S), ref['S']), 'qm': MH.worst(MH.f64(q), ref['qm'])}
    assert show(f'META_CASES {MH.field_id(c)}', f) <= 1.0
    cc = next(k for k in MH.CASES if MH.field_id(k) == MH.field_id(c))
    T = MH.traj_reference(cc)
    r = MC.trajectory(T.x, T.v, T.u, MH.BETA, MH.DT, cc.nstep, cc.integrator, T.tab, dt=LD, sched=IC.schedule(cc.integrator, MH.DT, cc.nstep))
    assert np.array_equal(r['acc'], T.acc)
    assert MH.worst(MH.f64(r['dH']), T.dH)[0] <= 1.0 and MH.worst(MH.f64(r['x_new']), T.xr, angle=True)[0] <= 1.0


# ---------------------------------------------------------------- the mutants
# mutant -> (the committed case that shows it: 'field:<id>', 'placement:<nb>' or a trajectory case id; the output named for it; the
# chain, or the link / site of a chain, where that output is furthest outside its bound).  x_prop is the twin's proposed end point of
# every chain per link (meta_hard_cases.traj_fracs): a defect of the MD is then named by the bound of a link, whatever the accept does
CAUGHT_BY = {
    'row_mod': ('field:rows-G2-rough', 'F', (4, 0, 7, 0)),
    'row_zero': ('field:rows-G3-rough', 'F', (3, 1, 1, 1)),
    'next_interval': ('placement:41', 'F', (2, 1, 1, 2)),
    'wall_sign': ('placement:41', 'F', (1, 1, 4, 4)),
    'edge_far': ('placement:2', 'vbias', (5,)),
    'stale_qm': ('rows-G3-quad-n1-leapfrog', 'x_new', None),                    # every accept as the reference's: a bound of x_new
    'sums_first_pass': ('field:L36-G2-rough', 'qm', (0,)),
    'drop_wave': ('field:L60-G1-quad', 'F', (0, 1, 52, 58)),
    'gp_one_pass': ('L132-G2-rough-n1-force_gradient', 'x_prop', None),         # a link beyond k_meta_gp's first pass (asserted below)
    'energy_second_block': ('batch-G3-rough-n1-omelyan', 'H0', (256,)),
    'select_proposed': ('rows-G2-rough-n1-leapfrog', 'qm', (4,)),               # chain 4 is the rejected one
    'slope_3e8': ('field:rows-G2-quad', 'F', (2, 0, 4, 1)),
}
ACCEPTS_KEPT = ('stale_qm', 'slope_3e8', 'select_proposed', 'energy_second_block')      # shown by a bound, not by a turned accept
# the purely numeric yardstick, c (1 + 3e-8): 3e-8 / u = 2.7e8 roundings of c, against a force bound that is a few dozen u of the
# site's terms -- it must leave its bound by six orders of magnitude, or the bound has gone slack
FLOOR = {'slope_3e8': 1e6}


def run_named(name, mutant):
    if name.startswith('field:'):
        c = next(c for c in MH.FIELD_CASES if MH.field_id(c) == name[6:])
        ref = MH.field_reference(c)
        return MH.field_fracs(MH.field_twin(ref['x'], ref['tab'], mutant), ref), True
    if name.startswith('placement:'):
        nb = int(name[10:])
        p = MH.placement(nb)
        return MH.field_fracs(MH.field_twin(p.x, p.tab, mutant), MH.placement_reference(nb)), True
    c = next(c for c in MH.CASES if MH.case_id(c) == name)
    return MH.traj_fracs(MH.traj_twin(c, mutant), MH.traj_reference(c))


@pytest.mark.parametrize('mutant', MH.MUTANTS)
def test_every_mutant_leaves_a_bound_on_its_named_case(mutant):
    name, output, where = CAUGHT_BY[mutant]
    f0, ok0 = run_named(name, None)
    f, ok = run_named(name, mutant)
    w, at = f[output]
    print(f'MUTANT {mutant}: {name}: {output} {w:.3g} of the bound at {list(at)} (accept flags {"equal" if ok else "differ"}); the worst '
          f'output: {MH.worst_of(f)[1]} {MH.worst_of(f)[0]:.3g}; the twin itself: {MH.worst_of(f0)[0]:.3f}')
    assert ok0 and MH.worst_of(f0)[0] <= 1.0
    assert not w <= FLOOR.get(mutant, 1.0), f
    assert where is None or at == where
    if mutant in ACCEPTS_KEPT:
        assert ok
    if mutant == 'stale_qm':                     # an accepted chain's link, by a bound that is finite
        assert MH.traj_reference(next(c for c in MH.CASES if MH.case_id(c) == name)).acc[at[0]] and math.isfinite(w)
    if mutant == 'gp_one_pass':
        # finite, in the accepted chain, and on a link whose force reads gP of a site beyond the first pass (the site itself or the
        # neighbour its difference takes): the per-link bound of x_prop bites there, over the four stages of the force-gradient step
        L = 132
        b, mu, i, j = at
        other = ((i - 1) % L) * L + j if mu == 1 else i * L + (j - 1) % L                  # f1 = g(i - 1, j) - g, f0 = g - g(i, j - 1)
        assert math.isfinite(w) and max(i * L + j, other) >= MH.GP_STRIDE, at
        assert MH.traj_reference(next(c for c in MH.CASES if MH.case_id(c) == name)).stages == 4


def test_mutants_are_the_list_the_twin_knows():
    assert sorted(CAUGHT_BY) == sorted(MH.MUTANTS) and len(MH.MUTANTS) == 12


# ---------------------------------------------------------------- the shapes reach what they claim
def test_shapes_reach_the_launch_edges_they_claim():
    S = MH.SHAPES
    nt = MH.chain_threads
    # kernels.h chain_threads
    assert [nt(L) for L in (4, 8, 28, 32, 36, 60, 64, 132)] == [256, 256, 256, 512, 512, 512, 1024, 1024]
    # rows: 1 < G < B, and the row of some chain is neither b % G nor "0 or b"
    B, L, Gs, kinds, paths = S['rows']
    for G in Gs:
        r = np.arange(B) // (B // G)
        assert 1 < G < B and B % G == 0 and np.any(r != np.arange(B) % G) and np.any(r != 0) and np.any(r != np.arange(B))
    # batch: a second workgroup of k_meta_energy that is not full (its guard runs); chains 256, 257 read row 2 at G = 3
    B, L, Gs, kinds, paths = S['batch']
    blocks = -(-B // MH.ENERGY_BLOCK)
    assert blocks == 2 and blocks * MH.ENERGY_BLOCK > B and B - MH.ENERGY_BLOCK == 2
    assert set(Gs) == {1, 3, B} and list(np.arange(B)[256:] // (B // 3)) == [2, 2]
    assert L * L < nt(L)                                  # idle threads in every chain sum
    # L36, L60: ragged passes of the 512-thread sums and of the one-launch kernel's 1024 threads
    for sid, full512, rest512, full1024, rest1024 in (('L36', 2, 272, 1, 272), ('L60', 7, 16, 3, 528)):
        B, L, Gs, kinds, paths = S[sid]
        n = L * L
        assert nt(L) == 512 and divmod(n, 512) == (full512, rest512) and divmod(n, MH.ONE_LAUNCH_NT) == (full1024, rest1024)
        assert L <= MH.ONE_LAUNCH_MAXL and paths == (1, 2) and rest512 % 64 != 0 and rest1024 % 64 != 0     # a wave with idle lanes
        # in pass `full1024` of the one-launch kernel some threads own a site and others hold st[k] = -1, with k >= 1
        assert full1024 >= 1 and 0 < rest1024 < MH.ONE_LAUNCH_NT and -(-n // MH.ONE_LAUNCH_NT) <= 4
    # L132: a second pass of k_meta_gp's grid-stride loop, 1024-thread sums with a ragged last pass; the sequenced path only
    B, L, Gs, kinds, paths = S['L132']
    n = L * L
    gx = min(64, -(-n // 256))
    assert gx * 256 == MH.GP_STRIDE == 16384 and n - MH.GP_STRIDE == 1040 and nt(L) == 1024 and divmod(n, 1024) == (17, 16)
    assert L > MH.ONE_LAUNCH_MAXL and paths == (2,)
    assert {(c.nstep, c.integrator) for c in MH.CASES if c.shape == 'L132'} == {(1, 'leapfrog'), (1, 'force_gradient')}
    # every shape meets the rough table, rows and L60 the quadratic one; nstep 1 and 2 and the three integrators are all met
    for sid, (B, L, Gs, kinds, paths) in S.items():
        assert {(c.G, c.table) for c in MH.CASES if c.shape == sid} == {(G, k) for G in Gs for k in kinds}
        assert 'rough' in kinds and (('quad' in kinds) == (sid in ('rows', 'L60')))
    assert {c.integrator for c in MH.CASES} == set(IC.NAMES) and {c.nstep for c in MH.CASES} == {1, 2}
    assert MH.BETA == 2.5 and MH.DT == 0.05
    # R of e(q)
    assert MH.sum_count(8) == max(BC.sum_roundings(64, 256), 1 + 21) and MH.sum_count(132) == BC.sum_roundings(132 * 132, 1024)


def test_inputs_carry_the_hard_classes_and_the_cases_meet_walls_and_intervals():
    """pinned links on chain 0, the last chain never regularized, momenta x 3; over the cases chains sit on both walls and inside, and
    some chain is rejected and some accepted"""
    inside = wall_pos = wall_neg = rej = acc = 0
    forced = []
    for c in MH.CASES:
        T = MH.traj_reference(c)
        assert np.all(np.abs(T.x[0, 0, 0, :]) == math.pi - 1e-9) and np.all(np.abs(T.x[0, 1, :, 0]) == math.pi - 1e-9)
        assert np.abs(T.x[-1]).min() > 26.0 and np.abs(T.x[:-1]).max() <= math.pi and 2.5 < T.v.std() < 3.5
        rej += int((~T.acc).sum()); acc += int(T.acc.sum())
        forced += [MH.case_id(c)] * T.forced
        # x_new is held per link in every case but the one where no accept is possible (meta_hard_cases.traj_reference)
        assert T.acc.any() or (MH.case_id(c) == 'L132-G2-rough-n1-leapfrog' and np.all(MH.f64(T.dH[0]) > SC.DH_MAX)), MH.case_id(c)
    for c in MH.FIELD_CASES:
        ref = MH.field_reference(c)
        q = MH.f64(ref['qm'][0])
        inside += int(ref['look'].inside.sum())
        wall_pos += int((~ref['look'].inside & (q > 0)).sum()); wall_neg += int((~ref['look'].inside & (q < 0)).sum())
    print(f'chains of the field cases: {inside} inside, {wall_pos} on the positive wall, {wall_neg} on the negative; accepts {acc}, rejects {rej}')
    # the accept path does not rest on chain 0's u = 0: every shape has a case that accepts a chain on the undisturbed draw
    print('cases where chain 0 draws u = 0 because the draw accepts no chain:', forced)
    for sid in MH.SHAPES:
        assert any(T.acc.any() and not T.forced for T in (MH.traj_reference(c) for c in MH.CASES if c.shape == sid)), sid
    assert forced == ['L36-G2-rough-n2-leapfrog']
    assert inside >= 100 and wall_pos >= 2 and wall_neg >= 2 and rej >= 10 and acc >= 10
