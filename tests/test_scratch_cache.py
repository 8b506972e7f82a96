"""CPU-only tests of the host plumbing of fthmc_amd/ops.py that needs no device to go wrong: the state machine of the one
scratch cache (ops._stream_buffer behind the seams _ws, _loops_ws, _inst_ws) and the fork and join of the chain groups
(ops._chain_groups).  A stand-in for the `torch` global of fthmc_amd.ops (in the manner of workspace_cases.GuardedTorch) supplies
streams with a handle the test sets, a capture flag the test sets, and `empty` on the host, pre-filled with a nonzero value."""
import contextlib

import pytest
import torch

from fthmc_amd import _lib, ops
from fthmc_amd._lib import FthmcError

FILL = 7.25                                    # what the stand-in's fresh memory holds
SMALL, LARGE = (1, 8, 1), (4, 16, 2)            # B, L, n_layers of the flow-sized requests
FAMILIES = ('flow', 'train_force', 'loops', 'instanton')


class FakeStream:
    def __init__(self, handle, log):
        self.cuda_stream, self.log = handle, log

    def wait_stream(self, other):
        self.log.append((self, other))


class FakeCuda:
    def __init__(self):
        self.log, self.capturing = [], False                   # log: (waiting stream, stream waited for), in order
        self.current = FakeStream(0x1000, self.log)
        self.made = []

    def current_stream(self, device=None):
        return self.current

    def is_current_stream_capturing(self):
        return self.capturing

    def Stream(self, device=None):
        self.made.append(FakeStream(0x2000 + 0x100 * len(self.made), self.log))
        return self.made[-1]

    @contextlib.contextmanager
    def stream(self, st):
        was, self.current = self.current, st
        try:
            yield
        finally:
            self.current = was


class FakeTorch:
    """everything is torch's own but `cuda` and `empty` (host memory filled with FILL, every tensor remembered)"""

    def __init__(self):
        self.cuda, self.allocated = FakeCuda(), []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, **kw):
        t = torch.empty(*size, **kw).fill_(FILL)
        self.allocated.append(t)
        return t


@pytest.fixture
def fake(monkeypatch):
    ft = FakeTorch()
    monkeypatch.setattr(ops, 'torch', ft)
    monkeypatch.setattr(ops, '_SIDE_STREAMS', {})
    ops.release_workspaces()
    yield ft
    ops.release_workspaces()


T = torch.zeros(1, dtype=torch.float64)         # the tensor whose device and stream a request goes by


def request(family, big=False):
    """(ptr, nbytes) of one request of the family through its seam, at the small or the large size"""
    B, L, nl = LARGE if big else SMALL
    if family == 'flow':
        return ops._ws(T, B, L, nl)
    if family == 'train_force':
        return ops._ws(T, B, L, nl, force=True)
    return {'loops': ops._loops_ws, 'instanton': ops._inst_ws}[family](T, 40960 if big else 520)


def needed(family, big=False):
    B, L, nl = LARGE if big else SMALL
    return {'flow': ops.ws_bytes(B, L, nl), 'train_force': ops.train_force_ws_bytes(B, L, nl)}.get(family, 40960 if big else 520)


def key_of(family, fake):
    return (None, fake.cuda.current.cuda_stream) + (() if family == 'flow' else (family,))


def snapshot():
    return ({k: (b.data_ptr(), b.numel()) for k, b in ops._WS.items()}, set(ops._WS_CAPTURED),
            [b.data_ptr() for b in ops._WS_RETIRED])


@pytest.mark.parametrize('family', FAMILIES)
def test_a_buffer_is_reused_until_a_larger_request_replaces_it(fake, family):
    assert 0 < needed(family) < needed(family, big=True)
    ptr, nb = request(family)
    assert nb >= needed(family) and len(fake.allocated) == 1
    assert ops._WS[key_of(family, fake)].data_ptr() == ptr
    assert request(family) == (ptr, nb)                          # equal size: the same buffer
    ptr2, nb2 = request(family, big=True)
    assert ptr2 != ptr and nb2 >= needed(family, big=True) and len(fake.allocated) == 2
    assert request(family) == (ptr2, nb2) == request(family, big=True)      # smaller and equal: the same buffer
    assert len(fake.allocated) == 2 and list(ops._WS) == [key_of(family, fake)]


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('captured', (False, True))
def test_an_outgrown_buffer_is_retired_iff_a_capture_saw_it(fake, family, captured):
    key = key_of(family, fake)
    ptr, _ = request(family)                                     # the eager warm-up
    fake.cuda.capturing = captured
    assert request(family)[0] == ptr                             # handed out again: during a capture, or not
    fake.cuda.capturing = False
    assert (key in ops._WS_CAPTURED) == captured
    ptr2, _ = request(family, big=True)
    assert [b.data_ptr() for b in ops._WS_RETIRED] == ([ptr] if captured else [])
    assert key not in ops._WS_CAPTURED                           # the new buffer has not been seen by a capture
    request(family, big=True)
    assert len(ops._WS_RETIRED) == int(captured) and ops._WS[key].data_ptr() == ptr2


@pytest.mark.parametrize('family', FAMILIES)
def test_allocation_and_growth_are_refused_during_a_capture(fake, family):
    fake.cuda.capturing = True
    with pytest.raises(FthmcError, match='graph capture'):
        request(family)                                          # would have to be allocated
    assert snapshot() == ({}, set(), []) and not fake.allocated
    fake.cuda.capturing = False
    ptr, nb = request(family)
    before, n = snapshot(), len(fake.allocated)
    fake.cuda.capturing = True
    with pytest.raises(FthmcError, match='graph capture'):
        request(family, big=True)                                # would have to be grown
    assert snapshot() == before and len(fake.allocated) == n
    assert request(family) == (ptr, nb)                          # what is there serves the capture


def test_streams_and_families_do_not_share_and_growth_leaves_the_others_alone(fake):
    first = {f: request(f) for f in FAMILIES}
    other = FakeStream(0x5000, fake.cuda.log)
    with fake.cuda.stream(other):
        second = {f: request(f) for f in FAMILIES}
        assert {(None, 0x5000), (None, 0x5000, 'loops')} <= set(ops._WS)
    ptrs = [p for r in (first, second) for p, _ in r.values()]
    assert len(set(ptrs)) == 8 == len(ops._WS) == len(fake.allocated)
    for grown in FAMILIES:
        was = {f: request(f) for f in FAMILIES}
        now = request(grown, big=True)
        assert now[0] != was[grown][0]
        assert {f: request(f) for f in FAMILIES if f != grown} == {f: r for f, r in was.items() if f != grown}
        with fake.cuda.stream(other):
            assert {f: request(f) for f in FAMILIES} == second       # nor the other stream's
    assert not ops._WS_RETIRED


def test_the_head_of_a_fresh_flow_or_train_force_buffer_is_zeroed_and_nothing_else(fake):
    head = int(_lib.load().fthmc_ws_head_bytes()) // 8
    assert head > 0
    for family, big in (('flow', False), ('train_force', False), ('flow', True), ('train_force', True)):
        _, nb = request(family, big)
        buf = ops._WS[key_of(family, fake)]
        assert buf is fake.allocated[-1] and nb // 8 > head, (family, big, nb, head)       # else the test shows nothing
        assert bool((buf[:head] == 0).all()) and bool((buf[head:] == FILL).all()), (family, big)
    for family in ('loops', 'instanton'):
        request(family)
        assert bool((ops._WS[key_of(family, fake)] == FILL).all()), family


def test_no_instanton_scratch_where_none_is_needed_and_release_empties_everything(fake):
    assert ops._inst_ws(T, 0) == (None, 0)
    assert snapshot() == ({}, set(), []) and not fake.allocated
    for f in FAMILIES:
        request(f)
    fake.cuda.capturing = True
    for f in FAMILIES:
        request(f)
    fake.cuda.capturing = False
    for f in FAMILIES:
        request(f, big=True)
    assert len(ops._WS) == 4 == len(ops._WS_RETIRED)
    ops.release_workspaces()
    assert snapshot() == ({}, set(), [])


# ---------------------------------------------------------------- the chain-group fork and join
@pytest.mark.parametrize('groups', (3, [1, 4, 2]), ids=('int', 'sizes'))
@pytest.mark.parametrize('own_sides', (False, True), ids=('pool', 'callers'))
def test_chain_groups_fork_tile_and_join(fake, groups, own_sides):
    B, cuda = 7, fake.cuda
    main = cuda.current
    edges = ops._group_edges(groups, B)
    assert edges == ([0, 2, 4, 7] if groups == 3 else [0, 1, 5, 7])
    mine = [FakeStream(0x9000 + i, cuda.log) for i in range(2)] if own_sides else None
    seen, log_at_yield = [], []
    for lo, hi, st in ops._chain_groups(torch.device('cpu'), edges, mine):
        log_at_yield.append(list(cuda.log))
        seen.append((lo, hi, st))
    sides = mine if own_sides else cuda.made
    assert len(sides) == 2 and (own_sides or ops._SIDE_STREAMS == {None: sides})
    # groups 1, 2, then 0: the pieces tile 0 .. B, and only group 0 is on the current stream
    assert [(lo, hi) for lo, hi, _ in seen] == [(edges[1], edges[2]), (edges[2], edges[3]), (edges[0], edges[1])]
    assert sorted((lo, hi) for lo, hi, _ in seen) == list(zip(edges[:-1], edges[1:])) and edges[0] == 0 and edges[-1] == B
    assert [st for _, _, st in seen] == [sides[0], sides[1], main]
    # the fork stands before the first group, nothing is added while the groups run, the join comes behind the last one
    fork, join = [(s, main) for s in sides], [(main, s) for s in sides]
    assert all(log == fork for log in log_at_yield)
    assert cuda.log == fork + join


def test_chain_groups_of_one_group_touch_no_stream_and_a_short_list_of_sides_is_refused(fake):
    main = fake.cuda.current
    assert list(ops._chain_groups(torch.device('cpu'), [0, 5])) == [(0, 5, main)]
    assert not fake.cuda.log and not fake.cuda.made
    with pytest.raises(FthmcError, match='side_streams'):
        list(ops._chain_groups(torch.device('cpu'), [0, 2, 4, 7], [FakeStream(0x9000, fake.cuda.log)]))
    assert not fake.cuda.log
