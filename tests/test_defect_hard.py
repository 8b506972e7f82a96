"""CPU checks behind tests/test_z_defect_hard_gpu.py (tests/defect_hard_cases.py): the float64 twin of the defect kernels, in their
operation and summation order on either trajectory path, stays inside every derived bound against the long double reference on every
committed case with no chain left out -- the proof that the inputs can meet the bounds without the device --; every named mutant of the
twin leaves a bound, or differs in bits, on the case named for it here; the shapes and the defects reach the launch edges they claim,
computed from the launchers' arithmetic; the reference here and defect_cases' long double twin state the same operations."""
import math

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401

import batch_kernel_cases as BC
import defect_cases as DC
import defect_hard_cases as DH
import integrator_cases as IC
import stencil_cases as SC

LD = DH.LD


def show(tag, f):
    w, k, at = DH.worst_of(f)
    print(f'{tag}: worst {w:.4f} of the bound at {k}{list(at)}  ' + ' '.join(f'{k} {v[0]:.3f}' for k, v in f.items()))
    return w


def test_reference_is_extended_precision():
    assert np.finfo(np.longdouble).nmant == 63


# ---------------------------------------------------------------- the twin inside the bounds, nothing left out
@pytest.mark.parametrize('c', DH.FIELD_CASES, ids=DH.field_id)
def test_twin_force_and_action_inside_the_bounds(c):
    ref = DH.field_reference(c)
    print(f'left out: {int((~ref["decided"]).sum())} charges of {c.B}')
    assert ref['decided'].all(), np.flatnonzero(~ref['decided'])
    f, ok = DH.field_fracs(DH.field_twin(c), ref)
    w = show(f'TWIN field {DH.field_id(c)}', f)
    assert ok and w <= 1.0


@pytest.mark.parametrize('c', DH.CASES, ids=DH.case_id)
def test_twin_trajectory_inside_the_bounds_and_nothing_is_left_out(c):
    T = DH.traj_reference(c)
    print(f'left out: {int((~T.accept_decided).sum())} accepts, {int((~T.charges_decided).sum())} charges of {c.B} (no lookup here: the weight is '
          f'a selection); seed redrawn {T.redraws} times, accepted {int(T.acc.sum())}, forced {T.forced}')
    assert T.charges_decided.all() and T.accept_decided.all()
    assert T.acc.any() and not T.acc.all()                      # the selection between the two ends is tested both ways
    for path in c.paths:
        f, ok = DH.traj_fracs(DH.traj_twin(c, path), T)
        w = show(f'TWIN trajectory {DH.case_id(c)} path {path}', f)
        assert ok and w <= 1.0, path


# ---------------------------------------------------------------- the two references state the same thing
@pytest.mark.parametrize('c', [c for c in DH.CASES if (c.shape, c.kind) in (('batch', 'wrap'), ('L36', 'end'))], ids=DH.case_id)
def test_reference_agrees_with_the_long_double_twin_of_defect_cases(c):
    """defect_cases wraps and regularizes with the long double pi, the reference here with the device's doubles: the two agree inside
    the bounds (x_new as an angle), and defect_cases.trajectory with the same schedule and uniforms gives the same accepts and charges"""
    ref = DH.field_reference(c)
    x, g, df = ref['x'], ref['g'], ref['df']
    S, C, Dm, Q = DC.action(x, DH.BETA, g, df, LD)
    f = {'F': DH.worst(DH.f64(DC.force(x, DH.BETA, g, df, LD)), ref['F']), 'S': DH.worst(DH.f64(S), ref['S']),
         'csum': DH.worst(DH.f64(C), ref['csum']), 'dsum': DH.worst(DH.f64(Dm), ref['dsum'])}
    assert show(f'DEFECT_CASES {DH.field_id(c)}', f) <= 1.0 and np.array_equal(Q, ref['Q'])
    assert np.array_equal(DC.mask(c.L, df), DH.t_on(c.L, df))
    T = DH.traj_reference(c)
    r = DC.trajectory(T.x, T.v, T.u, DH.BETA, T.g, T.df, DH.DT, c.nstep, c.integrator, dt=LD, sched=IC.schedule(c.integrator, DH.DT, c.nstep))
    assert np.array_equal(r['acc'], T.acc) and np.array_equal(r['Q'], T.Q)
    f = {k: DH.worst(DH.f64(r[k]), getattr(T, k)) for k in ('H0', 'H1', 'dH', 'csum', 'dsum')}
    f['x_new'] = DH.worst(DH.f64(r['x_new']), T.xr, angle=True)
    assert show(f'DEFECT_CASES trajectory {DH.case_id(c)}', f) <= 1.0


# ---------------------------------------------------------------- the translation's twin
@pytest.mark.parametrize('sid', ('L132', 'slice'))
def test_translation_twin_is_numpy_roll_per_chain(sid):
    t = DH.translate_case(sid)
    B, L = t.x.shape[0], t.x.shape[-1]
    shifts = [t.shift] if sid == 'slice' else [np.array([s, (3, 3)], dtype=np.int32) for s in DH.L132_SHIFTS]
    for sh in shifts:
        got = DH.t_translate(t.x, t.rung, t.top, sh)
        on = np.flatnonzero(t.rung == t.top)
        assert np.array_equal(SC.bits(np.delete(got, on, axis=0)), SC.bits(np.delete(t.x, on, axis=0)))          # a copy elsewhere
        for b in (on if B < 100 else np.concatenate([on[:40], [DH.SLICE - 1, DH.SLICE]])):
            assert np.array_equal(SC.bits(got[b]), SC.bits(np.roll(t.x[b], (int(sh[b][0]), int(sh[b][1])), axis=(1, 2)))), b
    if sid == 'L132':
        assert np.array_equal(SC.bits(DH.t_translate(t.x, t.rung, t.top, shifts[-1])), SC.bits(DC.translate(t.x, t.rung, t.top, shifts[-1])))
    assert np.array_equal(SC.bits(DH.t_translate(t.x, t.rung, 9, shifts[0])), SC.bits(t.x))                      # a rung nobody sits on


# ---------------------------------------------------------------- the mutants
# mutant -> (the committed case that shows it: 'field:<id>', 'translate:<shape>' or a trajectory case id with its path; the output
# named for it; the chain, or the link / site of a chain, where that output is furthest outside its bound -- None where the test below
# states instead what must hold of the place)
CAUGHT_BY = {
    'gp_one_pass': ('L132-straddle-n1-force_gradient/2', 'x_prop', None),       # a link beyond k_defect_gp's first pass (asserted below)
    'force_one_pass': ('field:L132-straddle', 'F', (0, 0, 124, 16)),            # site 16384 = (124, 16): the first one never written
    'translate_one_pass': ('translate:L132', 'bits', None),
    'energy_second_block': ('batch-wrap-n1-omelyan/2', 'H0', None),             # chain 256 or 257 (asserted below)
    'energy_sign': ('field:batch-full', 'S', None),
    'line_no_wrap': ('field:L132-wrapback', 'dsum', None),
    'line_along_j': ('field:L36-col0', 'F', None),
    'ld_inclusive': ('field:L60-one', 'dsum', None),
    'neighbour_weight': ('field:L36-end', 'F', None),
    'selected_is_proposal': ('batch-end-n2-leapfrog/1', 'dsum', None),          # a rejected chain (asserted below)
    'slice_g_from_zero': ('field:slice-wrap', 'F', None),                       # chain 65535 or 65536 (asserted below)
    'slice_shift_stride': ('translate:slice', 'bits', None),
}


def run_named(name, mutant):
    if name.startswith('field:'):
        c = next(c for c in DH.FIELD_CASES if DH.field_id(c) == name[6:])
        f, ok = DH.field_fracs(DH.field_twin(c, mutant), DH.field_reference(c))
        return f, ok, c
    name, path = name.split('/')
    c = next(c for c in DH.CASES if DH.case_id(c) == name)
    f, ok = DH.traj_fracs(DH.traj_twin(c, int(path), mutant), DH.traj_reference(c))
    return f, ok, c


@pytest.mark.parametrize('mutant', [m for m in DH.MUTANTS if not CAUGHT_BY[m][0].startswith('translate:')])
def test_every_mutant_leaves_a_bound_on_its_named_case(mutant):
    name, output, where = CAUGHT_BY[mutant]
    f0, ok0, c = run_named(name, None)
    f, ok, _ = run_named(name, mutant)
    w, at = f[output]
    print(f'MUTANT {mutant}: {name}: {output} {w:.3g} of the bound at {list(at)} (accept flags and charges {"equal" if ok else "differ"}); '
          f'the worst output: {DH.worst_of(f)[1]} {DH.worst_of(f)[0]:.3g}; the twin itself: {DH.worst_of(f0)[0]:.3f}')
    assert ok0 and DH.worst_of(f0)[0] <= 1.0
    assert not w <= 1.0, f
    assert where is None or at == where
    if mutant == 'gp_one_pass':
        # finite, and on a link whose force reads gP of a site beyond the first pass (the site itself or the neighbour its difference
        # takes): the per-link bound of x_prop bites there, over the four stages of the force-gradient step
        L = c.L
        b, mu, i, j = at
        other = ((i - 1) % L) * L + j if mu == 1 else i * L + (j - 1) % L
        assert math.isfinite(w) and max(i * L + j, other) >= DH.STRIDE_SITES, at
        assert DH.traj_reference(c).stages == 4
    if mutant == 'energy_second_block':
        T = DH.traj_reference(c)
        assert at[0] in (256, 257) and T.g[at[0]] != DH.BETA and math.isfinite(w)
        # chains below 256 keep every bound; behind them dH loses (beta - g)(Dsum1 - Dsum0), which may turn an accept as well
        assert f['H0'][0] > 1.0 and DH.worst(DH.traj_twin(c, 2, mutant)['H0'][:256], (T.H0[0][:256], T.H0[1][:256]))[0] <= 1.0
    if mutant == 'selected_is_proposal':
        T = DH.traj_reference(c)
        assert not T.acc[at[0]] and np.array_equal(DH.traj_twin(c, 1, mutant)['acc'], T.acc) and not T.forced
    if mutant == 'slice_g_from_zero':
        ref = DH.field_reference(c)
        assert at[0] in (DH.SLICE, DH.SLICE + 1) and ref['g'][at[0]] != ref['g'][at[0] - DH.SLICE]
        F = DH.field_twin(c, mutant)['F']
        assert DH.worst(F[:DH.SLICE], (ref['F'][0][:DH.SLICE], ref['F'][1][:DH.SLICE]))[0] <= 1.0          # the first slice is untouched
    if mutant in ('line_no_wrap', 'line_along_j', 'ld_inclusive'):
        df = DH.field_reference(c)['df']
        assert not np.array_equal(DH.t_on(c.L, df, mutant), DH.t_on(c.L, df))


def test_the_translation_mutants_differ_in_bits_where_they_should():
    t = DH.translate_case('L132')
    sh = np.array([DH.L132_SHIFTS[-1], (3, 3)], dtype=np.int32)
    good, bad = DH.t_translate(t.x, t.rung, t.top, sh), DH.t_translate(t.x, t.rung, t.top, sh, 'translate_one_pass')
    diff = (SC.bits(good) != SC.bits(bad)).reshape(2, 2, -1)
    assert diff[:, :, DH.STRIDE_SITES:].all() and not diff[:, :, :DH.STRIDE_SITES].any()
    print(f'MUTANT translate_one_pass: translate:L132: {int(diff.sum())} links differ in bits, all at sites >= {DH.STRIDE_SITES}')
    t = DH.translate_case('slice')
    good, bad = DH.t_translate(t.x, t.rung, t.top, t.shift), DH.t_translate(t.x, t.rung, t.top, t.shift, 'slice_shift_stride')
    chains = np.flatnonzero((SC.bits(good) != SC.bits(bad)).reshape(len(t.x), -1).any(axis=1))
    print(f'MUTANT slice_shift_stride: translate:slice: chains {chains.tolist()} differ in bits')
    assert chains.tolist() == [DH.SLICE]                       # 65535: the one top-rung chain of the second slice


def test_mutants_are_the_list_the_twin_knows():
    assert sorted(CAUGHT_BY) == sorted(DH.MUTANTS) and len(DH.MUTANTS) == 12


# ---------------------------------------------------------------- the shapes reach what they claim
def sites_of(df, L):
    i0, j0, Ld = df
    return [((i0 + a) % L) * L + j0 for a in range(Ld)]


def test_shapes_and_defects_reach_the_launch_edges_they_claim():
    S = DH.SHAPES
    nt = DH.chain_threads
    assert [nt(L) for L in (4, 8, 28, 32, 36, 60, 64, 132)] == [256, 256, 256, 512, 512, 512, 1024, 1024]
    # batch: a second workgroup of k_defect_energy that is not full (its guard runs); three couplings on chains 255, 256, 257
    B, L, kinds, paths = S['batch']
    blocks = -(-B // DH.ENERGY_BLOCK)
    assert blocks == 2 and blocks * DH.ENERGY_BLOCK > B and B - DH.ENERGY_BLOCK == 2 and paths == (1, 2)
    for dk in kinds:
        g = DH.couplings(B, DH.KINDS.index(dk))
        assert sorted(g[255:258]) == [0.0, DH.BETA / 3.0, DH.BETA]
    assert L * L < nt(L)                                  # idle threads in every chain sum
    # L36, L60: ragged passes of the 512-thread sums and of the one-launch kernel's 1024 threads
    for sid, full512, rest512, full1024, rest1024 in (('L36', 2, 272, 1, 272), ('L60', 7, 16, 3, 528)):
        B, L, kinds, paths = S[sid]
        n = L * L
        assert nt(L) == 512 and divmod(n, 512) == (full512, rest512) and divmod(n, DH.ONE_LAUNCH_NT) == (full1024, rest1024)
        assert L <= DH.ONE_LAUNCH_MAXL and paths == (1, 2) and rest512 % 64 != 0 and rest1024 % 64 != 0
        assert full1024 >= 1 and 0 < rest1024 < DH.ONE_LAUNCH_NT and -(-n // DH.ONE_LAUNCH_NT) <= 4
        assert (-(-n // 256)) <= 64                        # one pass of the grid-stride kernels
    # L132: a second pass of df_stride_grid's kernels; the sequenced path only; nstep 1, leapfrog and force-gradient
    B, L, kinds, paths = S['L132']
    n = L * L
    gx = min(64, -(-n // 256))
    assert gx * 256 == DH.STRIDE_SITES == 16384 and n - DH.STRIDE_SITES == 1040 and nt(L) == 1024 and divmod(n, 1024) == (17, 16)
    assert L > DH.ONE_LAUNCH_MAXL and paths == (2,) and 128 * 128 == DH.STRIDE_SITES      # defect_cases' largest lattice: one pass exactly
    assert {(c.nstep, c.integrator) for c in DH.CASES if c.shape == 'L132'} == {(1, 'leapfrog'), (1, 'force_gradient')}
    # slice: a second slice of two chains, three couplings on 65534 .. 65536, and none of the second slice's is what g_b[0 ..] holds
    B, L, kinds, paths = S['slice']
    assert [min(DH.SLICE, B - b0) for b0 in range(0, B, DH.SLICE)] == [65535, 2] and paths == () and 2 * B * L * L * 8 < 18e6
    for dk in kinds:
        g = DH.couplings(B, DH.KINDS.index(dk))
        assert sorted(g[DH.SLICE - 1:]) == [0.0, DH.BETA / 3.0, DH.BETA] and g[DH.SLICE] != g[0] and g[DH.SLICE + 1] != g[1]
    t = DH.translate_case('slice')
    assert t.rung[DH.SLICE - 1] == t.top == t.rung[DH.SLICE] and t.rung[DH.SLICE - 2] != t.top != t.rung[DH.SLICE + 1]
    a, b = t.shift[DH.SLICE - 1] % L, t.shift[DH.SLICE] % L
    assert a.all() and b.all() and (a != b).any()
    flat = t.shift.reshape(-1)                             # what a second slice reading shift + b0 would take for chain 65535
    assert tuple(flat[DH.SLICE:DH.SLICE + 2] % L) != tuple(b)
    top = t.shift[t.rung == t.top]
    assert (top == 0).any() and (top % L == L - 1).any() and (top < 0).any() and (top >= L).any()
    sh = np.array(DH.L132_SHIFTS)
    assert (sh == 0).any() and (sh == 131).any() and (sh < -132).any() and (sh >= 264).any() and (sh == 132).any()
    # the defects: end starts on the last row and all but one of its plaquettes take the a + L branch
    for sid, (B, L, kinds, paths) in S.items():
        assert 'end' in kinds
        i0, j0, Ld = DH.defect_of('end', L)
        assert i0 == L - 1 and Ld == L and sum(1 for i in range(L) if i - i0 < 0) == L - 1
        for dk in kinds:
            i0, j0, Ld = DH.defect_of(dk, L)
            assert 0 <= i0 < L and 0 <= j0 < L and 0 < Ld <= L and int(DH.t_on(L, (i0, j0, Ld)).sum()) == Ld
    L = 132
    st = sites_of(DH.defect_of('straddle', L), L)
    assert st[4] == 124 * L + 5 == 16373 and st[5] == 125 * L + 5 == 16505 and st[4] < DH.STRIDE_SITES <= st[5] and st == sorted(st)
    wb = sites_of(DH.defect_of('wrapback', L), L)
    assert wb[0] >= DH.STRIDE_SITES and wb[3] >= DH.STRIDE_SITES and wb[4] == 131 and max(wb[4:]) < DH.STRIDE_SITES      # rows 128 .. 131, then 0 .. 3
    assert {c.integrator for c in DH.CASES} == set(IC.NAMES) and {c.nstep for c in DH.CASES} == {1, 2}
    assert DH.BETA == 2.5 and DH.DT == 0.05
    assert DH.sum_count(36) == max(BC.sum_roundings(36 * 36, 512), 2 + 21) and DH.sum_count(132) == BC.sum_roundings(132 * 132, 1024)


def test_inputs_carry_the_hard_classes_and_every_case_selects_both_ways():
    """pinned links on chain 0, the last chain never regularized, momenta x 3; every trajectory case holds an accepted and a rejected
    chain; the accept path and the reject path do not rest on the forced uniforms alone"""
    forced, natural_rej, natural_acc = [], 0, 0
    for c in DH.CASES:
        T = DH.traj_reference(c)
        assert np.all(np.abs(T.x[0, 0, 0, :]) == math.pi - 1e-9) and np.all(np.abs(T.x[0, 1, :, 0]) == math.pi - 1e-9)
        assert np.abs(T.x[-1]).min() > 26.0 and np.abs(T.x[:-1]).max() <= math.pi and 2.5 < T.v.std() < 3.5
        assert T.acc.any() and not T.acc.all()
        forced += [(DH.case_id(c),) + f for f in T.forced]
        hit = {f[1] for f in T.forced}
        natural_rej += sum(1 for b in np.flatnonzero(~T.acc) if b not in hit)
        natural_acc += sum(1 for b in np.flatnonzero(T.acc) if b not in hit)
    for c in DH.FIELD_CASES:
        x = DH.field_reference(c)['x']
        P = DH.f64(SC.r_plaq(DH.ld(x[-1:]), np.zeros(x[-1:].shape))[0])
        assert np.abs(P).max() > 100.0                    # plaquette angles of the field that was never regularized
    print(f'forced uniforms ({len(forced)}):')
    for f in forced:
        print('  ', f)
    print(f'chains of the trajectory cases decided by their drawn uniform: {natural_acc} accepted, {natural_rej} rejected')
    for sid in ('batch', 'L36', 'L60', 'L132'):
        Ts = [DH.traj_reference(c) for c in DH.CASES if c.shape == sid]
        assert any(not T.forced for T in Ts), sid             # a case of every shape whose two kinds both come from the draw
    assert natural_acc >= 100 and natural_rej >= 15
