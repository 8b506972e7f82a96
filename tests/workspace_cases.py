"""The scratch contract of include/fthmc_hip.h as a table: every entry point that takes a workspace, the shapes at which each
kernel family, layout branch and launch shape of csrc/api_call.h ws_layout / vjp_layout / force_layout is reached, and the guarded
buffers the calls run in.  Shared by tests/test_workspace_contract.py (CPU: the size queries, and that the table reaches what it
claims) and tests/test_workspace_contract_gpu.py (the calls).  A plain module: nothing here touches a GPU at import.

Guarded memory (in the manner of `Poisoned`, tests/test_batch_kernels_gpu.py): n bytes sit GUARD = 256 doubles inside one larger
allocation with GUARD doubles behind them; 2 KB is a multiple of 32 doubles, so the 256-byte alignment the kernels rely on for
their 16-byte loads survives the offset.  Guards are compared to the byte.

Route: the scratch reaches the library through the ordinary fthmc_amd.ops functions.  `Route` replaces ops._ws (and _loops_ws,
_inst_ws) for the duration of a test: it asks the original for the size the op requests, after ops.release_workspaces(), so the
size is the queried one and not a cached larger one, and hands back a guarded buffer of exactly that size; it remembers every
buffer (chain groups on side streams ask once per stream).  It also stands in for the `torch` global of fthmc_amd.ops, so that
every output an op allocates (empty / empty_like / zeros) is a NaN-filled guarded buffer too.

Inputs are plain ones: seeded uniform links in (-pi, pi), oracle.ref_cpu.default_flow weights at scale 1 (DEEP: see its comment);
the hard inputs live in the numeric suites.  All default-net cases of up to 8 layers read a prefix of ONE weight tensor, so that a
weight version stated for it holds across the cases (test (d))."""
import collections
import math
import types

import torch

import first_order_cases as FC
import walk_model as M
from oracle import ref_cpu as R

GUARD = 256                                   # doubles in front of and behind every guarded region
NAN_BITS = 0x7FF8C0FFEE5EED00                 # a quiet NaN with a recognisable payload
BIG = 1e300                                   # finite: a stray read that is multiplied by zero still shows
FILLS = ('nan', 'big', 'zero', 'stale')
BETA, DT, NSTEP = 2.0, 0.05, 2
WKEY = 0x5EED0001                             # the weight version the versioned calls state
HEAD_LAYERS = 64                              # FLOW_WHEAD_LAYERS (csrc/kernels.h)


# ---------------------------------------------------------------- guarded memory
def fill_(t, fill):
    """fill a float64 tensor in place: 'nan' (NAN_BITS), 'big', 'zero'"""
    if fill == 'nan':
        t.view(torch.int64).fill_(NAN_BITS)
    elif fill == 'big':
        t.fill_(BIG)
    elif fill == 'zero':
        t.zero_()
    else:
        raise ValueError(fill)
    return t


class Guarded:
    """nbytes at offset GUARD doubles of one allocation, GUARD doubles (and the slack up to a whole double) behind them.
    fill: 'nan' | 'big' | 'zero', or 'stale' with `arena` = an earlier Guarded whose memory is taken over as it is (the guards are
    rewritten, the body keeps what the earlier call left; memory the arena did not have is NaN).  zero_head: that many leading
    bytes are zeroed (a workspace that will be used with a weight version).  keep: hold a copy of the whole allocation for
    untouched()."""

    def __init__(self, nbytes, fill='nan', device='cuda', arena=None, zero_head=0, keep=False):
        self.nbytes = int(nbytes)
        self.nd = (self.nbytes + 7) // 8
        total = self.nd + 2 * GUARD
        if fill == 'stale' and arena is not None:
            if arena.buf.numel() >= total:
                self.buf = arena.buf
            else:
                self.buf = fill_(torch.empty(total, dtype=torch.float64, device=device), 'nan')
                self.buf[:arena.buf.numel()].copy_(arena.buf)
            fill_(self.buf[:GUARD], 'nan')
            fill_(self.buf[GUARD + self.nd:GUARD + self.nd + GUARD], 'nan')
        else:
            self.buf = fill_(torch.empty(total, dtype=torch.float64, device=device), 'nan')
            if fill not in ('nan', 'stale'):
                fill_(self.body, fill)
        if zero_head:
            self.body[:min(self.nd, zero_head // 8)].zero_()
        raw = self.buf.view(torch.uint8)
        self._front, self._back = raw[:8 * GUARD], raw[8 * GUARD + self.nbytes:8 * (GUARD + self.nd + GUARD)]
        self._front0, self._back0 = self._front.clone(), self._back.clone()
        self._all0 = self.buf[:total].clone() if keep else None
        self._total = total

    @property
    def body(self):
        return self.buf[GUARD:GUARD + self.nd]

    @property
    def ptr(self):
        return self.body.data_ptr() if self.nd else self.buf.data_ptr() + 8 * GUARD

    def tensor(self, shape, dtype=torch.float64):
        n = 1
        for d in shape:
            n *= int(d)
        return self.body.view(dtype)[:n].view(tuple(shape))

    @classmethod
    def of(cls, t, device='cuda'):
        """a host tensor copied into guarded device memory -> (Guarded, the device tensor)"""
        g = cls(t.numel() * t.element_size(), 'nan', device)
        d = g.tensor(t.shape, t.dtype)
        d.copy_(t)
        return g, d

    def broken(self):
        """the sides whose guard changed: a sublist of ['front', 'back']"""
        return [side for side, now, was in (('front', self._front, self._front0), ('back', self._back, self._back0))
                if not torch.equal(now, was)]

    def intact(self):
        return not self.broken()

    def untouched(self):
        """guards AND body keep every bit (keep=True)"""
        return torch.equal(self.buf[:self._total].view(torch.int64), self._all0.view(torch.int64))


def same_bits(a, b):
    """two tensors with equal shape, dtype and bits (NaNs compare by payload)"""
    if a is None or b is None:
        return a is None and b is None
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.contiguous(), b.contiguous()
    if a.dtype == torch.float64:
        a, b = a.view(torch.int64), b.view(torch.int64)
    return torch.equal(a, b)


class GuardedTorch:
    """Stands in for the `torch` global of fthmc_amd.ops: empty / empty_like / zeros on a device hand out guarded memory (NaN-filled,
    zeros: zero-filled) and remember it; everything else is torch's own.  `on` False: all of it is torch's own."""

    def __init__(self):
        self.handed, self.on, self.keep = [], True, False

    def __getattr__(self, name):
        return getattr(torch, name)

    def _new(self, shape, dtype, device, fill):
        dtype = dtype or torch.float64
        n = 1
        for d in shape:
            n *= int(d)
        g = Guarded(n * torch.empty(0, dtype=dtype).element_size(), fill, device, keep=self.keep)
        self.handed.append(g)
        return g.tensor(shape, dtype)

    @staticmethod
    def _shape(size):
        return tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)

    def empty(self, *size, dtype=None, device=None, **kw):
        if not self.on or device is None or torch.device(device).type != 'cuda' or kw:
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        return self._new(self._shape(size), dtype, device, 'nan')

    def zeros(self, *size, dtype=None, device=None, **kw):
        if not self.on or device is None or torch.device(device).type != 'cuda' or kw:
            return torch.zeros(*size, dtype=dtype, device=device, **kw)
        return self._new(self._shape(size), dtype, device, 'zero')

    def empty_like(self, t, **kw):
        if not self.on or not t.is_cuda or kw:
            return torch.empty_like(t, **kw)
        return self._new(tuple(t.shape), t.dtype, t.device, 'nan')


class Route:
    """The workspaces and outputs of fthmc_amd.ops for the duration of a test (install with a monkeypatch, see the module
    docstring).  mode 'exact': every request gets a guarded buffer of exactly the size the original would have had, filled with
    `fill` ('stale': the k-th request takes over the k-th buffer of `prior`), head zeroed where `versioned`; 'shared': every
    request gets the one buffer `shared`; 'cached': the ordinary ops route, nothing guarded.  short / null: hand the library
    `short` bytes less than the buffer has / a null pointer (the refusals)."""

    def __init__(self, ops, monkeypatch):
        self.ops, self.torch = ops, GuardedTorch()
        self.orig = {name: getattr(ops, name) for name in ('_ws', '_loops_ws', '_inst_ws')}
        self.head_bytes = int(ops._lib.load().fthmc_ws_head_bytes())
        self.mode, self.fill, self.versioned, self.short, self.null, self.keep = 'exact', 'nan', False, 0, False, False
        self.handed, self.prior, self.shared = [], [], None
        monkeypatch.setattr(ops, 'torch', self.torch)
        monkeypatch.setattr(ops, '_ws', lambda t, *a, **k: self._route('_ws', t, a, k, head=True))
        monkeypatch.setattr(ops, '_loops_ws', lambda t, *a, **k: self._route('_loops_ws', t, a, k))
        monkeypatch.setattr(ops, '_inst_ws', lambda t, *a, **k: self._route('_inst_ws', t, a, k))

    def reset(self, mode='exact', fill='nan', versioned=False, short=0, null=False, keep=False):
        """forget what was handed out (a 'stale' fill takes it over as `prior`) and set the next call's mode"""
        self.prior = self.handed if fill == 'stale' else []
        self.handed, self.torch.handed = [], []
        self.mode, self.fill, self.versioned, self.short, self.null, self.keep = mode, fill, versioned, short, null, keep
        self.torch.on, self.torch.keep = mode != 'cached', keep

    def _route(self, name, t, a, k, head=False):
        if self.mode == 'cached':
            return self.orig[name](t, *a, **k)
        if self.mode == 'shared':
            return self.shared.ptr, self.shared.nbytes
        on, self.torch.on = self.torch.on, False
        try:
            self.ops.release_workspaces()
            try:
                ptr, nbytes = self.orig[name](t, *a, **k)
            except self.ops.FthmcError:                   # a shape whose size query is 0 (only the refusals ask for one)
                ptr, nbytes = None, 0
            self.ops.release_workspaces()
        finally:
            self.torch.on = on
        if ptr is None and name == '_inst_ws':              # the path needs no workspace
            return None, 0
        i = len(self.handed)
        arena = self.prior[i] if self.fill == 'stale' and i < len(self.prior) else None
        g = Guarded(nbytes, self.fill, t.device, arena=arena, zero_head=self.head_bytes if head and self.versioned else 0,
                    keep=self.keep)
        self.handed.append(g)
        return (None if self.null else g.ptr), max(0, nbytes - self.short)

    def broken(self):
        """[(what, index, side)] over every workspace and every output handed out since reset()"""
        return [(what, i, side) for what, gs in (('workspace', self.handed), ('output', self.torch.handed))
                for i, g in enumerate(gs) for side in g.broken()]


# ---------------------------------------------------------------- settings
Setting = collections.namedtuple('Setting', 'name variant small dual')
SETTINGS = [Setting('default', 1, True, 1), Setting('tiled', 1, False, 1), Setting('valu', 0, True, 1),
            Setting('dual0', 1, True, 0), Setting('dual2', 1, True, 2), Setting('dual3', 1, True, 3)]
SETTING = {s.name: s for s in SETTINGS}


def apply_setting(ops, s):
    ops.set_variant(s.variant)
    ops.set_small_path(s.small)
    ops.set_dual_path(s.dual)


# ---------------------------------------------------------------- cases
Case = collections.namedtuple('Case', 'name L B nl arch only')


def _d(L, B, nl, only=None):
    return Case(f'L{L}_B{B}_nl{nl}', L, B, nl, None, only)


# Default net: every L of (4, 8, 12, 16, 20, 32) with B in {1, 3} and n_layers in {0, 1, 3, 8} (odd counts end the gP ping-pong in the
# other field).  L = 4: tiled kernels below the small path, one ragged tile; 8, 12, 16: flow_small.hip, and with the small path off
# one wrapping tile, ragged tiles, one exact tile; 20: ragged, the two-kernel training backward; 32: exact tiles, the in-place
# forward sweep, flow_bwd_train.hip with one reduction behind the sweep; 64, B = 1: the row-strip leapfrog, the largest one-launch
# plain trajectory; 68, B = 1: the multi-launch plain trajectory.
GRID = [_d(L, B, nl) for L in (4, 8, 12, 16, 20, 32) for B in (1, 3) for nl in (0, 1, 3, 8)]
WALKED = _d(32, 257, 2, only=('flow_layer_bwd_gw', 'train_grad'))      # tests/walk_model.py LAYER_SHAPES (32, 257): both kernels walk
DEEP = _d(8, 2, 65)                                                    # deeper than the head: layer 64 is expanded by every call
NET = Case('net_4_6_k5_L8', 8, 2, 3, ((4, 6), 5, 3), None)             # flow_generic.hip: hbuf / gbuf
K15 = Case('net_k15_L8', 8, 2, 2, ((3,), 15, 3), None)                 # kernel_size > L (tests/net_shape_cases.py k15_L8)
CASES = GRID + [_d(64, 1, 1), _d(68, 1, 1), WALKED, DEEP, NET, K15]
BY_NAME = {c.name: c for c in CASES}
# DEEP runs at scale 1: the oracle moves by 1.7e-14 at most there (tests/test_workspace_contract.py asserts and prints the figure)
DEEP_SCALE = 1.0

_HOST = {}


def _master():
    """the eight default-net layers every default case of up to 8 layers reads a prefix of"""
    if 'master' not in _HOST:
        _HOST['master'] = R.default_flow(8, torch.Generator().manual_seed(90001))
    return _HOST['master']


def flow_of(case):
    """the case's weights as the oracle takes them (at least one layer: the one-layer rows use layer 0)"""
    key = ('flow', case.name)
    if key not in _HOST:
        gen = torch.Generator().manual_seed(90100 + CASES.index(case))
        if case.arch is not None:
            hidden, k, n_mix = case.arch
            _HOST[key] = R.default_flow(case.nl, gen, hidden=hidden, k=k, n_mix=n_mix)
        elif case.nl > 8:
            _HOST[key] = [tuple(t * DEEP_SCALE for t in lw) for lw in R.default_flow(case.nl, gen)]
        else:
            _HOST[key] = _master()[:max(case.nl, 1)]
    return _HOST[key]


def pack(flow):
    """flat canonical weights [layers * params] (what ops.pack_weights builds, without its device step)"""
    return torch.cat([t.reshape(-1) for lw in flow for t in lw]).to(torch.float64).contiguous()


def host_inputs(case, L=None):
    """the host tensors of a case, made once and never modified (L: another lattice size, for the refusals; not cached)"""
    key = ('inputs', case.name)
    if L is None and key in _HOST:
        return _HOST[key]
    B, LL = case.B, case.L if L is None else L
    gen = torch.Generator().manual_seed(91000 + CASES.index(case))
    u01 = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    ang = lambda *s: (u01(*s) * 2 - 1) * math.pi
    nrm = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    flow = flow_of(case)
    h = {'x': ang(B, 2, LL, LL), 'x2': ang(B, 2, LL, LL), 'v': nrm(B, 2, LL, LL), 'g': nrm(B, 2, LL, LL), 'u': u01(B),
         'P': ang(B, LL, LL), 'gfP': nrm(B, LL, LL), 'gS': nrm(B), 'glogdet': nrm(B), 'beta_b': 1.5 + u01(B),
         'seeds': torch.randint(0, 2 ** 62, (B,), generator=gen, dtype=torch.int64),
         'w': pack(flow), 'w1': pack(flow[:1])}
    if L is None:
        _HOST[key] = h
    return h


def device_inputs(case, host=None, device='cuda'):
    """-> (namespace of device tensors in guarded memory + the case's nl / arch / mu / off, {name: Guarded}, the host tensors)"""
    host = host_inputs(case) if host is None else host
    I, guards = types.SimpleNamespace(nl=case.nl, arch=case.arch, mu=1, off=2, B=case.B, L=host['x'].shape[-1]), {}
    for name, t in host.items():
        guards[name], d = Guarded.of(t, device)
        setattr(I, name, d)
    if case.nl == 0:
        I.w = None
    return I, guards, host


def inputs_changed(I, guards, host, skip=()):
    """names of the inputs that lost a bit or whose guards did"""
    return [name for name, t in host.items() if name not in skip
            and (not same_bits(getattr(I, name) if not (name == 'w' and I.nl == 0) else guards[name].tensor(t.shape, t.dtype),
                               t.to(guards[name].buf.device)) or not guards[name].intact())]


# ---------------------------------------------------------------- the entry points
# kind: 'layer' one layer (the case's layer count plays no part: served once per (L, B, net)), 'flow' a whole flow of any depth,
# 'train' a flow of at least one layer, 'plain' no net (served once per (L, B)).  call(ops, I, wkey) -> {name: output tensor}
# (None: not produced).  consts: the inputs that must keep their bits -- all of them, but for a documented alias.
# small: fthmc_set_small_path decides between two kernel families for it; valu: fthmc_set_variant(0) serves it on the default net.
Row = collections.namedtuple('Row', 'name kind call alias small valu versioned integ act')
ROWS = []


def _row(name, kind, call, alias=(), small=False, valu=True, versioned=False, integ=False, act=True):
    ROWS.append(Row(name, kind, call, tuple(alias), small, valu, versioned, integ, act))


def _named(names, values):
    return dict(zip(names, values))


def _stash_pair(o, I, k):
    y, logJ, stash = o.flow_layer_fwd_stash(I.x, I.w1, I.mu, I.off, arch=I.arch)
    gx, gw = o.flow_layer_bwd_stash(stash, I.x.shape, I.w1, I.g, I.gS, I.mu, I.off, need_gw=True, arch=I.arch)
    return {'y': y, 'logJ': logJ, 'gx': gx, 'gw': gw}


def _traj(o, I, k, **kw):
    beta = kw.pop('beta', BETA)
    r = o.ft_trajectory(I.x, I.v, I.u, I.w, I.nl, beta, DT, NSTEP, arch=I.arch, wkey=k, **kw)
    return dict(r)


def _chained(o, I, k):
    a = _traj(o, I, k)
    b = o.ft_trajectory(a['x_new'], I.v, I.u, I.w, I.nl, BETA, DT, NSTEP, arch=I.arch, wkey=k, state_in=a['state'])
    return {**{'first_' + n: t for n, t in a.items()}, **b}


def _loops(o, I, k):
    Rm, Tm = max(1, I.L // 2), I.L
    mean = o.torch.empty(Rm, Tm, dtype=torch.float64, device=I.x.device)
    return {'W': o.wilson_loops(I.x, Rm, Tm, mean_out=mean), 'Wmean': mean}


_row('flow_layer_fwd', 'layer', lambda o, I, k: _named(('y', 'logJ'), o.flow_layer_fwd(I.x, I.w1, I.mu, I.off, arch=I.arch)))
_row('flow_layer_fwd_inplace', 'layer',                                                       # y may alias x
     lambda o, I, k: _named(('y', 'logJ'), o.flow_layer_fwd(I.x, I.w1, I.mu, I.off, arch=I.arch, inplace=True)), alias=('x',))
_row('flow_layer_rev', 'layer', lambda o, I, k: _named(('x', 'logJ'), o.flow_layer_rev(I.x, I.w1, I.mu, I.off, arch=I.arch)))
_row('flow_layer_bwd', 'layer',
     lambda o, I, k: _named(('gx', 'gw'), o.flow_layer_bwd(I.x, I.w1, I.g, I.gS, I.mu, I.off, need_gw=False, arch=I.arch)))
_row('flow_layer_bwd_gw', 'layer',
     lambda o, I, k: _named(('gx', 'gw'), o.flow_layer_bwd(I.x, I.w1, I.g, I.gS, I.mu, I.off, need_gw=True, arch=I.arch)))
_row('flow_layer_stash_pair', 'layer', _stash_pair, valu=False)
_row('plaq_coupling_fwd', 'layer', lambda o, I, k: _named(('fP', 'logJ'), o.plaq_coupling_fwd(I.P, I.w1, I.mu, I.off, arch=I.arch)),
     valu=False)
_row('plaq_coupling_rev', 'layer', lambda o, I, k: _named(('P', 'logJ'), o.plaq_coupling_rev(I.P, I.w1, I.mu, I.off, arch=I.arch)),
     valu=False)
_row('plaq_coupling_bwd', 'layer', valu=False, call=lambda o, I, k: _named(
    ('gP', 'gw'), o.plaq_coupling_bwd(I.P, I.w1, I.gfP, I.gS, I.mu, I.off, need_gw=False, arch=I.arch)))
_row('plaq_coupling_bwd_gw', 'layer', valu=False, call=lambda o, I, k: _named(
    ('gP', 'gw'), o.plaq_coupling_bwd(I.P, I.w1, I.gfP, I.gS, I.mu, I.off, need_gw=True, arch=I.arch)))
_row('flow_forward', 'flow', lambda o, I, k: _named(('y', 'logdet'), o.flow_forward(I.x, I.w, I.nl, arch=I.arch, wkey=k)),
     small=True, versioned=True)
_row('flow_reverse', 'flow', lambda o, I, k: _named(('x', 'logdet'), o.flow_reverse(I.x, I.w, I.nl, arch=I.arch, wkey=k)),
     versioned=True)
_row('ft_action', 'flow', lambda o, I, k: _named(('S_eff', 'logdet', 'plaq', 'Q'), o.ft_action(I.x, I.w, I.nl, BETA, arch=I.arch, wkey=k)),
     small=True, versioned=True)
_row('ft_force', 'flow', lambda o, I, k: {'F': o.ft_force(I.x, I.w, I.nl, BETA, arch=I.arch, wkey=k)}, small=True, versioned=True)
for _name in ('leapfrog', 'omelyan', 'force_gradient'):                                          # every integrator of ops.integrator_code
    _row('ft_leapfrog_' + _name, 'flow', small=True, versioned=True, integ=True, call=lambda o, I, k, _n=_name: _named(
        ('x', 'v'), o.ft_leapfrog(I.x, I.v, I.w, I.nl, BETA, DT, NSTEP, arch=I.arch, wkey=k, integrator=_n)))
_row('ft_trajectory_md', 'flow', lambda o, I, k: _traj(o, I, k, mode='md'), small=True, versioned=True, integ=True)
_row('ft_trajectory_literal', 'flow', lambda o, I, k: _traj(o, I, k, mode='literal'), versioned=True)
_row('ft_trajectory_per_chain_beta', 'flow', lambda o, I, k: _traj(o, I, k, beta=I.beta_b), small=True, versioned=True, integ=True)
_row('ft_trajectory_force_gradient', 'flow', lambda o, I, k: _traj(o, I, k, integrator='force_gradient'), small=True, versioned=True)
_row('ft_trajectory_groups2', 'flow', lambda o, I, k: _traj(o, I, k, groups=2), small=True)
_row('ft_trajectory_chained', 'flow', _chained, small=True, versioned=True)
for _name in ('leapfrog', 'omelyan', 'force_gradient'):
    _row('leapfrog_' + _name, 'plain', integ=True, act=False,
         call=lambda o, I, k, _n=_name: _named(('x', 'p'), o.leapfrog(I.x, I.v, BETA, DT, NSTEP, integrator=_n)))
_row('hmc_trajectory', 'plain', lambda o, I, k: dict(o.hmc_trajectory(I.x, I.v, I.u, BETA, DT, NSTEP)), integ=True, act=False)
_row('hmc_trajectory_per_chain_beta', 'plain', lambda o, I, k: dict(o.hmc_trajectory(I.x, I.v, I.u, I.beta_b, DT, NSTEP)),
     integ=True, act=False)
_row('hmc_trajectory_force_gradient', 'plain', act=False,
     call=lambda o, I, k: dict(o.hmc_trajectory(I.x, I.v, I.u, BETA, DT, NSTEP, integrator='force_gradient')))
_row('train_metrics', 'plain', lambda o, I, k: {'row': o.train_metrics(I.x, I.x2, I.gS, I.glogdet, BETA)}, valu=False, act=False)
_row('train_grad', 'train', lambda o, I, k: dict(o.train_grad(I.x, I.w, I.nl, BETA, arch=I.arch)), small=True)
_row('train_grad_groups2', 'train', lambda o, I, k: dict(o.train_grad(I.x, I.w, I.nl, BETA, groups=2, arch=I.arch)), small=True)
# the second order runs on the plain kernels whatever the switches say (include/fthmc_hip.h): served under the default setting
_row('ft_action_vjp', 'flow', valu=False, call=lambda o, I, k: _named(
    ('gx', 'gw'), o.ft_action_vjp(I.x, I.w, I.nl, BETA, I.gS, I.glogdet, arch=I.arch)))
_row('ft_force_vjp', 'flow', valu=False, call=lambda o, I, k: _named(('gx', 'gw'), o.ft_force_vjp(I.x, I.w, I.nl, BETA, I.g, arch=I.arch)))
_row('train_force_grad', 'flow', lambda o, I, k: dict(o.train_force_grad(I.x, I.w, I.nl, BETA, arch=I.arch)), small=True)
_row('wilson_loops', 'plain', _loops, valu=False, act=False)
_row('instanton_hit_path2', 'plain', valu=False, act=False,
     call=lambda o, I, k: _named(('x', 'k', 'nacc'), o.instanton_hit(I.x, BETA, I.seeds, n_hit=3, path=2)))
_row('instanton_hit_path2_inplace', 'plain', valu=False, act=False, alias=('x',),                # x_out may be x
     call=lambda o, I, k: _named(('x', 'k', 'nacc'), o.instanton_hit(I.x, BETA, I.seeds, n_hit=3, path=2, out=I.x)))
ROW = {r.name: r for r in ROWS}
VJP_ROWS = ('ft_action_vjp', 'ft_force_vjp')
# the plain entry points never run the generic kernels; the deep, walked and generic cases add nothing to them
_PLAIN_SKIP = (WALKED.name, DEEP.name, NET.name, K15.name)


def serves(row, case, setting):
    """does the row run at the case under the setting (each distinct launch once)"""
    if case.only is not None and row.name not in case.only:
        return False
    if setting.name.startswith('dual'):
        return row.name == 'train_force_grad' and case.arch is None and case.nl > 0
    if setting.name == 'valu' and (not row.valu or case.arch is not None):
        return False
    if setting.name == 'tiled' and not (row.small and case.arch is None and M.ft_small_shape(case.L, case.nl)):
        return False
    if row.name.endswith('groups2') and case.B < 2:
        return False
    if row.kind == 'train':
        return case.nl >= 1
    if row.kind == 'plain':
        return case.name not in _PLAIN_SKIP and case is _first_with(case.L, case.B, None, plain=True)
    if row.kind == 'layer':
        return case is WALKED or case is _first_with(case.L, case.B, case.arch)
    return True


def _first_with(L, B, arch, plain=False):
    for c in CASES:
        if (c.L, c.B, c.arch) == (L, B, arch) and c.only is None and not (plain and c.name in _PLAIN_SKIP):
            return c
    return None


def table():
    """[(row, case, setting)] of every call the GPU tests make"""
    return [(r, c, s) for r in ROWS for s in SETTINGS for c in CASES if serves(r, c, s)]


def table_ids(t=None):
    return [f'{r.name}-{c.name}-{s.name}' for r, c, s in (table() if t is None else t)]


def donor(row, case, setting):
    """the case whose call leaves the 'stale' scratch: the next one the row serves under the setting"""
    served = [c for c in CASES if serves(row, c, setting)]
    return served[(served.index(case) + 1) % len(served)] if len(served) > 1 else None


# ---------------------------------------------------------------- the oracle at the deep case
def deep_inputs():
    """the DEEP case as first_order_cases.Inputs"""
    h = host_inputs(DEEP)
    return FC.Inputs(flow_of(DEEP), h['x'], h['g'], h['gS'], h['glogdet'], 'silu')


def deep_results(inp, beta=BETA):
    """the first-order quantities test (e) compares, keyed like first_order_cases.oracle_results"""
    with torch.no_grad():
        y, logdet = R.flow_forward(inp.x, inp.flow, inp.act)
        S = R.ft_action(inp.x, inp.flow, beta, inp.act)
    out, grads = R.train_grads(inp.x, inp.flow, beta, inp.act)
    return {'y': y, 'logdet': logdet, 'S_eff': S, 'F': R.ft_force(inp.x, inp.flow, beta, inp.act).detach(),
            'logq': out['logq'].detach(), 'logp': out['logp'].detach(), 'gw': [tuple(g.detach() for g in lg) for lg in grads]}


def deep_oracle():
    if 'deep' not in _HOST:
        _HOST['deep'] = deep_results(deep_inputs())
    return _HOST['deep']


def deep_sensitivity(seed=9300):
    """worst move per entry of deep_results under FC.NUDGES nudges of every link and weight by one relative 2^-52"""
    inp, ref, errs = deep_inputs(), deep_oracle(), {}
    for n in range(FC.NUDGES):
        for key, e in FC.compare(deep_results(FC.nudged(inp, seed + n)), ref, inp.flow).items():
            errs[key] = max(errs.get(key, 0.0), e) if e == e else e
    return errs
