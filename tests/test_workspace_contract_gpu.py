"""GPU: every entry point that takes a workspace, held to the scratch contract of include/fthmc_hip.h -- scratch of the queried size
suffices; nothing is kept between calls except the weight expansions in the fixed head; the head holds nothing else; a refused
call enqueues nothing.  Table, cases and the guarded buffers: tests/workspace_cases.py; the CPU side (size queries, what the table
reaches, the conditioning of the 65-layer case): tests/test_workspace_contract.py.

Every call goes through the ordinary fthmc_amd.ops functions.  `route` replaces ops._ws / _loops_ws / _inst_ws for one test: each
request is answered with a guarded buffer of exactly the size the original asks the library for (after release_workspaces(), so
never a cached larger one), and the outputs the op allocates are guarded NaN-filled buffers as well.

  (a) exact, NaN-filled scratch: the call succeeds, no output holds a NaN, every guard of every workspace, output and input keeps
      its bytes (the failure names the entry point, the case, the buffer and the side, front or back);
  (c) with it: the inputs keep their bits (the documented aliases -- y may be x for the forward layer, x_out may be x for
      instanton_hit -- run as aliases); the second-order calls leave the head as it was; train_force_grad leaves the expansion of
      its weights there;
  (b) the same call on NaN, 1e300, zero and stale scratch (what the same entry point just left at ANOTHER case) and through the
      ordinary cached route gives the same bits in every output, after a control of two runs on the same fill;
  (d) in ONE zero-headed scratch sized for the largest case, with the weights expanded once under a version: every versioned
      entry point at every default-net case leaves the head bit for bit what fthmc_pack_weights made of it, and returns the bits of
      the version-less call;
  (e) the 65-layer flow (one layer past the head) against oracle.ref_cpu per tensor and per chain at second_order_cases.BOUND =
      1e-9, under the default setting, with the small path off and with the VALU variant; versioned calls repeat their bits;
  (f) every cheap refusal -- scratch 8 bytes short, null scratch (FTHMC_ERR_WS), L % 4 != 0, mu = 2, off = 4, null weights
      (FTHMC_ERR_ARG), activation code 3, an unknown integrator (FTHMC_ERR_UNSUPPORTED) -- returns its code and leaves scratch,
      outputs, guards and inputs as they were.  fthmc_hmc_trajectory never looks at its workspace where one launch serves the
      trajectory (L <= 64, MFMA variant): its scratch refusals are made at L = 68.

Found and fixed: fthmc_instanton_ws_bytes was the one size query that did not return a multiple of 256 bytes (136 bytes at B = 2,
L = 8: part[B][nw][2] doubles + k[B] int32, unrounded; found by tests/test_workspace_contract.py before any GPU run), so a caller
who carves one allocation into workspaces by the queried sizes misaligned whatever came behind it.  csrc/api.hip now rounds it up
as ws_layout rounds its regions; tests/test_instanton.py and tests/hip/instanton_walk.cpp, which pinned the unrounded figure,
state the rounded one.  Nothing else: no entry point is other than bit-reproducible, none reads scratch it did not write, none
writes outside the queried size, none keeps anything in the head but the expansion, and no listed refusal had enqueued anything.

Observed on an MI355X (5142 tests, 47 s; the slowest 0.25 s).  (case, setting) pairs per entry point, each run by (a) and by (b),
2468 in all -- settings: default; `tiled` = small path off (L = 8, 12, 16 with layers); `valu` = variant 0; dual0 /
dual2 / dual3 = the other settings of the dual-path switch (train_force_grad only):
  flow_layer_fwd                    32   flow_layer_fwd_inplace            32   flow_layer_rev                    32
  flow_layer_bwd                    32   flow_layer_bwd_gw                 34   flow_layer_stash_pair             17
  plaq_coupling_fwd                 17   plaq_coupling_rev                 17   plaq_coupling_bwd                 17
  plaq_coupling_bwd_gw              17   flow_forward                     123   flow_reverse                     104
  ft_action                        123   ft_force                         123   ft_leapfrog_leapfrog             123
  ft_leapfrog_omelyan              123   ft_leapfrog_force_gradient       123   ft_trajectory_md                 123
  ft_trajectory_literal            104   ft_trajectory_per_chain_beta     123   ft_trajectory_force_gradient     123
  ft_trajectory_groups2             62   ft_trajectory_chained            123   leapfrog_leapfrog                 28
  leapfrog_omelyan                  28   leapfrog_force_gradient           28   hmc_trajectory                    28
  hmc_trajectory_per_chain_beta     28   hmc_trajectory_force_gradient     28   train_metrics                     14
  train_grad                       101   train_grad_groups2                50   ft_action_vjp                     53
  ft_force_vjp                      53   train_force_grad                 240   wilson_loops                      14
  instanton_hit_path2               14   instanton_hit_path2_inplace       14
(d): 600 versioned calls under the default setting, 180 with the small path off, 600 with the VALU variant, each set in one scratch
of 10 637 568 bytes; (f): 200 refusals.
(e), L = 8, B = 2, 65 layers at scale 1, where the oracle itself moves by 1.7e-14 at worst (S_eff of chain 0) under the nudges:
  setting    worst per tensor (gw)             worst per chain
  default    7.1e-15 (layer 1 tensor 1)        2.6e-12 (-logdet of flow_reverse, chain 0)
  tiled      1.1e-14 (layer 1 tensor 1)        2.6e-12 (the same)
  valu       1.8e-14 (layer 1 tensor 1)        1.5e-12 (the same)
against the bound 1e-9; the per-chain worst is the inverse's, solved per site to 1e-12 in each of 65 layers.

That the tests bite, measured once on copies of the tree with one change each in csrc/api.hip:
  1. the size queries and the scratch check see 64 doubles less than ws_layout(...).total, the pointers stay those of the true
     layout: 717 of the 2468 cases of (a) fail, every one naming the back guard of a workspace and none a front guard -- all of
     ft_force, ft_leapfrog_*, ft_trajectory_md / _per_chain_beta / _force_gradient / _chained / _groups2 (the stash, or xa .. vb
     without layers, ends the layout) but on the small path, the one-layer backwards, train_grad (gz), the plain MD and the
     multi-launch plain trajectory.  The case picked for it: ft_force at L4_B3_nl3, whose stash of 3 x 19 x 3 x 16 = 2736 doubles
     ends 16 doubles before its padded region does, so that 48 live doubles land in the guard.  flow_forward, ft_action and the
     forward layers pass: what they write ends before the last 64 doubles.
  2. the log J sum behind sweep_forward reads one partial more per chain than the forward kernels write: 352 cases of (a) fail
     ("output logdet / S_eff holds a NaN") and the same 352 of (b) ("differ between NaN and big scratch"): flow_forward and
     ft_action 78 each (every case with layers that is not on the small path), ft_trajectory_literal 78, train_grad 80,
     train_grad_groups2 38.
"""
import pytest
import torch

import first_order_cases as FC
import workspace_cases as W
from gpu_support import module_defaults, ops, switches

pytestmark = pytest.mark.gpu
_defaults = module_defaults(dual=1)                             # W.SETTING['default']

TABLE = W.table()
IDS = W.table_ids(TABLE)
FIRST_ORDER_SETTINGS = [W.SETTING[n] for n in ('default', 'tiled', 'valu')]
ARG, UNSUPPORTED, WS = -1, -2, -4
REFUSALS = {'short': WS, 'null': WS, 'Lmod4': ARG, 'mu2': ARG, 'off4': ARG, 'nullw': ARG, 'act3': UNSUPPORTED, 'integrator': UNSUPPORTED}


@pytest.fixture(scope='module', autouse=True)
def _workspaces_released():
    yield
    ops.release_workspaces()


@pytest.fixture()
def route(monkeypatch):
    r = W.Route(ops, monkeypatch)
    yield r
    torch.cuda.synchronize()
    monkeypatch.undo()
    ops.release_workspaces()


@pytest.fixture()
def under(setting):
    """the switches of the test's `setting` parameter, for the test"""
    with switches(variant=setting.variant, small=setting.small, dual=setting.dual):
        yield


def run(route, row, case, wkey=None, I=None, **mode):
    """one call of the row at the case on fresh inputs -> (outputs, inputs, their guards, their host copies)"""
    I, guards, host = W.device_inputs(case) if I is None else I
    route.reset(**mode)
    out = row.call(ops, I, wkey)
    torch.cuda.synchronize()
    return out, I, guards, host


def differing(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if not W.same_bits(a[k], b[k])]


def say(broken):
    return '; '.join(f'the {side} guard of {what} {i} broke' for what, i, side in broken)


# ---------------------------------------------------------------- (a), (c)
@pytest.mark.parametrize('row,case,setting', TABLE, ids=IDS)
def test_a_exact_scratch_suffices_and_nothing_else_is_written(route, under, row, case, setting):
    label = f'{row.name} at {case.name} under {setting.name}'
    out, I, guards, host = run(route, row, case, fill='nan')
    assert route.handed, f'{label}: no workspace was asked for'
    assert all(g.nbytes % 256 == 0 for g in route.handed)
    for name, t in out.items():
        assert t is None or not t.is_floating_point() or not bool(torch.isnan(t).any()), f'(a) {label}: output {name} holds a NaN'
    assert not route.broken(), f'(a) {label}: {say(route.broken())}'
    changed = W.inputs_changed(I, guards, host, skip=row.alias)
    assert not changed, f'(c) {label}: the inputs {changed} (or their guards) changed'
    ws, head = route.handed[0], route.head_bytes // 8
    if row.name in W.VJP_ROWS:                                  # the second order never writes the head
        assert bool((ws.body[:head].view(torch.int64) == W.NAN_BITS).all()), f'(d) {label}: the head was written'
    if row.name == 'train_force_grad' and case.arch is None and case.nl > 0:      # ... and force training leaves the expansion there
        ref = W.Guarded(ops.ws_bytes(1, 4, case.nl), 'zero')
        route.reset(mode='shared')
        route.shared = ref
        ops.pack_workspace(I.x, I.w, case.nl, 1, 4)
        torch.cuda.synchronize()
        n = min(case.nl, W.HEAD_LAYERS) * (head // W.HEAD_LAYERS)
        assert ref.intact() and bool((ref.body[:n] != 0).any())
        assert W.same_bits(ws.body[:n], ref.body[:n]), f'(d) {label}: the head is not the expansion of the weights'


# ---------------------------------------------------------------- (b)
@pytest.mark.parametrize('row,case,setting', TABLE, ids=IDS)
def test_b_no_read_of_unwritten_scratch(route, under, row, case, setting):
    label = f'{row.name} at {case.name} under {setting.name}'
    other = W.donor(row, case, setting)
    first = run(route, row, case, fill='nan')[0]
    again = run(route, row, case, fill='nan')[0]
    assert not differing(first, again), f'{label}: not bit-reproducible on one fill: {differing(first, again)}'
    for fill in ('big', 'zero'):
        got = run(route, row, case, fill=fill)[0]
        assert not differing(first, got) and not route.broken(), f'(b) {label}: {differing(first, got)} differ between NaN and {fill} scratch'
    run(route, row, other, fill='nan')
    got = run(route, row, case, fill='stale')[0]
    assert all(g.buf is p.buf or g.nd > p.nd for g, p in zip(route.handed, route.prior)) and len(route.prior) >= len(route.handed) > 0
    assert not differing(first, got), f'(b) {label}: {differing(first, got)} differ on the scratch {other.name} left'
    assert not route.broken(), f'(b) {label} on stale scratch: {say(route.broken())}'
    run(route, row, other, mode='cached')
    got = run(route, row, case, mode='cached')[0]
    assert not differing(first, got), f'(b) {label}: {differing(first, got)} differ from the cached ops route'


# ---------------------------------------------------------------- (d)
@pytest.mark.parametrize('setting', FIRST_ORDER_SETTINGS, ids=[s.name for s in FIRST_ORDER_SETTINGS])
def test_d_the_head_is_only_ever_the_weight_expansion(route, under, setting):
    cases = [c for c in W.CASES if c.arch is None and c.nl <= 8 and c.only is None]
    rows = [r for r in W.ROWS if r.versioned]
    head = route.head_bytes // 8
    shared = W.Guarded(max(ops.ws_bytes(c.B, c.L, c.nl) for c in cases), 'big', zero_head=route.head_bytes)
    wg, w = W.Guarded.of(W.pack(W._master()))
    route.reset(mode='shared')
    route.shared = shared
    ops.pack_workspace(w, w, 8, 1, 4, wkey=W.WKEY)
    torch.cuda.synchronize()
    head0 = shared.body[:head].clone()
    wint = head // W.HEAD_LAYERS
    assert bool((head0[:8 * wint].view(8, wint) != 0).any(1).all()) and not bool((head0[8 * wint:] != 0).any())
    n = 0
    for row in rows:
        for case in cases:
            if not W.serves(row, case, setting):
                continue
            label = f'{row.name} at {case.name} under {setting.name}'
            inp = W.device_inputs(case)
            inp[0].w = w[:case.nl * 955] if case.nl else None         # the same address and version for every case
            got = run(route, row, case, wkey=W.WKEY, I=inp, mode='shared')[0]
            assert W.same_bits(shared.body[:head], head0), f'(d) {label}: the head changed under an unchanged weight version'
            assert shared.intact() and wg.intact() and not route.broken(), label
            ref = run(route, row, case, fill='nan')[0]
            assert not differing(ref, got), f'(d) {label}: {differing(ref, got)} differ between the versioned and the version-less call'
            n += 1
    print(f'(d) {setting.name}: {n} versioned calls in one scratch of {shared.nbytes} bytes')
    assert n >= len(rows)


# ---------------------------------------------------------------- (e)
@pytest.mark.parametrize('setting', FIRST_ORDER_SETTINGS, ids=[s.name for s in FIRST_ORDER_SETTINGS])
def test_e_the_deep_flow_against_the_oracle(under, setting):
    ops.release_workspaces()
    try:
        c, inp, ref = W.DEEP, W.deep_inputs(), W.deep_oracle()
        x, w = inp.x.cuda(), W.host_inputs(c)['w'].cuda()
        calls = {'flow_forward': lambda k: ops.flow_forward(x, w, c.nl, wkey=k), 'ft_action': lambda k: ops.ft_action(x, w, c.nl, W.BETA, wkey=k),
                 'ft_force': lambda k: (ops.ft_force(x, w, c.nl, W.BETA, wkey=k),)}
        plain = {name: f(None) for name, f in calls.items()}
        y, ld = plain['flow_forward']
        S, ld_a, _, _ = plain['ft_action']
        t = ops.train_grad(x, w, c.nl, W.BETA)
        xb, ld_r = ops.flow_reverse(y, w, c.nl)
        tensors = FC.compare({'gw': t['gw']}, ref, inp.flow)
        chains = FC.compare({'y': y, 'logdet': ld, 'S_eff': S, 'F': plain['ft_force'][0], 'logq': t['logq'], 'logp': t['logp']}, ref, inp.flow)
        chains.update(FC.per_chain_angle(t['x'], ref['y'], 'x of train_grad'))
        chains.update(FC.per_chain(ld_a, ref['logdet'], 'logdet of ft_action'))
        chains.update(FC.per_chain_angle(xb, inp.x, 'flow_reverse(flow_forward(x))'))
        chains.update(FC.per_chain(-ld_r, ref['logdet'], '-logdet of flow_reverse'))
        print(f'(e) {setting.name}: worst per tensor %.1e (%s), worst per chain %.1e (%s)' % (FC.worst(tensors)[::-1] + FC.worst(chains)[::-1]))
        assert len(tensors) == 6 * c.nl and len(chains) == 10 * c.B
        FC.hold(tensors, FC.BOUND, f'{c.name} under {setting.name}')
        FC.hold(chains, FC.BOUND, f'{c.name} under {setting.name}')
        # a stated version: the 64 layers of the head are expanded by the first call only, layer 64 by every call
        for name, f in calls.items():
            a, b = f(W.WKEY), f(W.WKEY)
            assert all(W.same_bits(p, q) and W.same_bits(p, r) for p, q, r in zip(plain[name], a, b)), name
    finally:
        ops.release_workspaces()


# ---------------------------------------------------------------- (f)
def refusal_case(row):
    """where the row's refusals are made: L = 8 where it is served there; the plain trajectories at L = 68, the first shape at
    which they look at their workspace"""
    served = [c for c in W.CASES if W.serves(row, c, W.SETTING['default']) and c.arch is None and (c.nl >= 1 or row.kind == 'plain')]
    want = 68 if row.name.startswith('hmc_trajectory') else 8
    return next(c for c in served if c.L == want)


def refusals_of(row):
    kinds = ['short', 'null', 'Lmod4']
    kinds += ['mu2', 'off4'] if row.kind == 'layer' else []
    kinds += ['nullw'] if row.kind != 'plain' else []
    kinds += ['act3'] if row.act else []
    kinds += ['integrator'] if row.integ else []
    return kinds


REFUSED = [(row, kind) for row in W.ROWS for kind in refusals_of(row)]


@pytest.mark.parametrize('row,kind', REFUSED, ids=[f'{r.name}-{k}' for r, k in REFUSED])
def test_f_a_refused_call_enqueues_nothing(route, monkeypatch, row, kind):
    from fthmc_amd._lib import FthmcError
    case, code = refusal_case(row), REFUSALS[kind]
    label = f'{row.name} at {case.name}, {kind}'
    host = W.host_inputs(case, L=case.L + 2) if kind == 'Lmod4' else None
    inp = W.device_inputs(case, host)
    I = inp[0]
    if kind == 'Lmod4':                                         # past the wrapper's own check, to the library's
        monkeypatch.setattr(ops, '_field', lambda t, name='x': ops._dev(t, name))
        monkeypatch.setattr(ops, '_plaq_field', lambda t, name='P': ops._dev(t, name))
    elif kind == 'mu2':
        I.mu = 2
    elif kind == 'off4':
        I.off = 4
    elif kind == 'act3':
        monkeypatch.setattr(ops, 'act_code', lambda act: 3)
    elif kind == 'integrator':
        monkeypatch.setattr(ops, 'integrator_code', lambda name: 5)
    elif kind == 'nullw':
        p, weights = ops._p, {I.w.data_ptr(), I.w1.data_ptr()}
        monkeypatch.setattr(ops, '_p', lambda t: None if t is not None and t.data_ptr() in weights else p(t))
    mode = dict(fill='nan', keep=True, short=8 if kind == 'short' else 0, null=kind == 'null')
    if row.name == 'wilson_loops' and kind == 'Lmod4':          # ops refuses a size query of 0 itself: the C ABI directly
        route.reset(**mode)
        Wt = route.torch.empty(I.B, 3, I.L, dtype=torch.float64, device='cuda')
        ws = W.Guarded(4096, 'nan', keep=True)
        route.handed.append(ws)
        rc = ops._lib.load().fthmc_wilson_loops(I.x.data_ptr(), I.B, I.L, 3, I.L, Wt.data_ptr(), None, ws.ptr, ws.nbytes, ops._stream(I.x))
        assert rc == code, (label, rc)
    else:
        with pytest.raises(FthmcError) as e:
            run(route, row, case, I=inp, **mode)
        assert f'(code {code})' in str(e.value), f'{label}: {e.value}'
    torch.cuda.synchronize()
    assert route.handed or kind == 'Lmod4', label               # (a size query of 0: no scratch to hand out)
    touched = [(what, i) for what, gs in (('workspace', route.handed), ('output', route.torch.handed))
               for i, g in enumerate(gs) if not g.untouched()]
    assert not touched, f'(f) {label}: refused with code {code}, but {touched} were written'
    changed = W.inputs_changed(*inp)
    assert not changed, f'(f) {label}: the inputs {changed} changed'
