"""The host arithmetic the sampler drivers share (fthmc_amd/graph_loop.py), on CPU tensors: the named row layout of every driver, the
row ring, the run_hmc-keyed history of a chain loop and the argument checks.  The documented layouts ("Rows of the
captured loops") are written out here as offsets counted by hand."""
import numpy as np
import pytest
import torch

from fthmc_amd.graph_loop import Row, RowRing, chain_history, instanton_arg, loops_arg

CPU = torch.device('cpu')


def layouts(B, loops, M, K):
    """every driver's row as the driver builds it -> {name: (Row, [(field, offset, shape), ...] as documented)}"""
    nl = loops[0] * loops[1]
    return {
        'ft_hmc': (Row(CPU, acc=B, dH=B, plaq=B, Q=B, wloops=loops),
                   [('acc', 0, (B,)), ('dH', B, (B,)), ('plaq', 2 * B, (B,)), ('Q', 3 * B, (B,)), ('wloops', 4 * B, loops)]),
        'ft_hmc without loops': (Row(CPU, acc=B, dH=B, plaq=B, Q=B, wloops=None),
                                 [('acc', 0, (B,)), ('dH', B, (B,)), ('plaq', 2 * B, (B,)), ('Q', 3 * B, (B,))]),
        'ft_run': (Row(CPU, dH=1, acc=1, plaq=1, Q=1, exp_mdH=1, k=1, nacc=1),
                   [('dH', 0, (1,)), ('acc', 1, (1,)), ('plaq', 2, (1,)), ('Q', 3, (1,)), ('exp_mdH', 4, (1,)), ('k', 5, (1,)), ('nacc', 6, (1,))]),
        'ft_run without hits': (Row(CPU, dH=1, acc=1, plaq=1, Q=1, exp_mdH=1, k=0, nacc=0),
                                [('dH', 0, (1,)), ('acc', 1, (1,)), ('plaq', 2, (1,)), ('Q', 3, (1,)), ('exp_mdH', 4, (1,))]),
        'run_local': (Row(CPU, plaq=B, Q=B, wloops=loops, k=B, nacc=B),
                      [('plaq', 0, (B,)), ('Q', B, (B,)), ('wloops', 2 * B, loops), ('k', 2 * B + nl, (B,)), ('nacc', 3 * B + nl, (B,))]),
        'run_local without loops': (Row(CPU, plaq=B, Q=B, wloops=None, k=B, nacc=B),
                                    [('plaq', 0, (B,)), ('Q', B, (B,)), ('k', 2 * B, (B,)), ('nacc', 3 * B, (B,))]),
        'run_local without hits': (Row(CPU, plaq=B, Q=B, wloops=loops, k=0, nacc=0),
                                   [('plaq', 0, (B,)), ('Q', B, (B,)), ('wloops', 2 * B, loops)]),
        'run_meta': (Row(CPU, acc=B, dH=B, plaq=B, Q=B, qm=B, vbias=B),
                     [('acc', 0, (B,)), ('dH', B, (B,)), ('plaq', 2 * B, (B,)), ('Q', 3 * B, (B,)), ('qm', 4 * B, (B,)), ('vbias', 5 * B, (B,))]),
        'run_tempered': (Row(CPU, acc=M * K, dH=M * K, plaq=M * K, Q=M * K, rung=M * K, swap_acc=(M, K - 1)),
                         [(f, i * M * K, (M * K,)) for i, f in enumerate(('acc', 'dH', 'plaq', 'Q', 'rung'))] + [('swap_acc', 5 * M * K, (M, K - 1))]),
    }


CASES = [(1, (1, 1), 1, 2), (3, (2, 3), 2, 3)]


@pytest.mark.parametrize('B,loops,M,K', CASES)
def test_every_driver_row_has_the_documented_offsets(B, loops, M, K):
    for name, (row, fields) in layouts(B, loops, M, K).items():
        assert list(row.fields) == [f for f, _, _ in fields], name                        # the order, and nothing omitted takes room
        assert row.width == sum(int(np.prod(s)) for _, _, s in fields) == row.flat.numel(), name
        assert row.flat.dtype == torch.float64 and row.flat.is_contiguous() and not row.flat.any(), name
        for f, offset, shape in fields:
            view = row[f]
            assert tuple(view.shape) == shape, (name, f)
            assert view.data_ptr() == row.flat.data_ptr() + 8 * offset and view.is_contiguous(), (name, f)


@pytest.mark.parametrize('B,loops,M,K', CASES)
def test_values_written_through_the_views_come_back_under_their_names(B, loops, M, K):
    for name, (row, fields) in layouts(B, loops, M, K).items():
        n, want = 4, {}
        rows = np.zeros((n, row.width))
        for i in range(n):                                                               # n iterations: write by name, copy the flat row as the loop does
            for j, (f, _, shape) in enumerate(fields):
                val = 1000.0 * i + 100.0 * j + torch.arange(int(np.prod(shape)), dtype=torch.float64).view(shape)
                row[f].copy_(val)
                want.setdefault(f, []).append(val.numpy())
            rows[i] = row.flat.numpy()
        assert len(np.unique(rows)) == rows.size, name                                   # distinct values: a shifted field would show
        for split in (row.split(rows), {k: v.numpy() for k, v in row.split(torch.from_numpy(rows)).items()}):
            assert list(split) == [f for f, _, _ in fields], name
            for f, _, shape in fields:
                assert split[f].shape == (n,) + shape and np.array_equal(split[f], np.stack(want[f])), (name, f)
        one = row.split(rows[2])                                                         # a single row: n = 1
        assert all(one[f].shape == (1,) + shape and np.array_equal(one[f][0], want[f][2]) for f, _, shape in fields), name


def test_a_layout_laid_over_the_lines_of_a_block_is_the_tempering_period():
    M, K, P = 2, 3, 4
    layout = Row(None, acc=M * K, dH=M * K, plaq=M * K, Q=M * K, rung=M * K, swap_acc=(M, K - 1))
    assert layout.flat is None and layout.width == 5 * M * K + M * (K - 1)
    block = torch.zeros(P, layout.width, dtype=torch.float64)
    for j in range(P):
        line = layout.over(block[j])
        line['rung'].fill_(j + 1.0)
        line['swap_acc'].copy_(torch.full((M, K - 1), -(j + 1.0), dtype=torch.float64))
    c = layout.split(block.numpy().reshape(1, -1).reshape(P, layout.width))
    assert c['rung'].shape == (P, M * K) and c['swap_acc'].shape == (P, M, K - 1)
    assert np.array_equal(c['rung'][:, 0], np.arange(1.0, P + 1)) and np.array_equal(c['swap_acc'][:, 1, 1], -np.arange(1.0, P + 1))
    assert not c['acc'].any() and not c['Q'].any()


def test_ring_returns_every_pushed_row_in_order_and_resets():
    ring = RowRing(5, 3, CPU)
    assert ring.rows().shape == (0, 5) and ring.rows().dtype == np.float64 and ring.n == 0
    row = torch.zeros(5, dtype=torch.float64)
    for i in range(7):
        row.copy_(10.0 * i + torch.arange(5, dtype=torch.float64))
        ring.push(row.view(1, 5) if i % 2 else row)                                      # any shape of the right size
        assert ring.n == i + 1 and len(ring.flushed) == (i + 1) // 3
        assert np.array_equal(ring.rows(), 10.0 * np.arange(i + 1)[:, None] + np.arange(5.0)[None, :])
    got = ring.rows()
    row.fill_(-1.0)                                                                      # what was read is a copy
    assert got.shape == (7, 5) and np.array_equal(got[:, 0], 10.0 * np.arange(7))
    ring.reset()
    assert ring.n == 0 and ring.rows().shape == (0, 5)
    ring.push(row)
    assert np.array_equal(ring.rows(), -np.ones((1, 5)))
    full = RowRing(2, 2, CPU)                                                            # exactly full: nothing left in the device part
    for i in range(4):
        full.push(torch.full((2,), float(i), dtype=torch.float64))
    assert np.array_equal(full.rows(), np.repeat(np.arange(4.0), 2).reshape(4, 2))


@pytest.mark.parametrize('B,loops_every', [(1, 1), (3, 2), (3, 3)])
def test_chain_history_builds_the_run_hmc_keys(B, loops_every):
    ntraj, n = 7, 2                                                                      # the third run of an experiment of 7 per run
    rng = np.random.default_rng(5)
    q0 = rng.integers(-3, 4, B).astype(np.float64)
    q = rng.integers(-3, 4, (ntraj, B)).astype(np.float64)
    plaq, dH = rng.random((ntraj, B)), rng.standard_normal((ntraj, B))
    wl = rng.random((ntraj, 2, 3))
    k = rng.integers(-2, 3, (ntraj, B)).astype(np.int32)
    build = [i < 4 for i in range(ntraj)]
    h = chain_history(n * ntraj + 1, 0.25, q0, {'acc': np.ones((ntraj, B)), 'dH': dH, 'plaq': plaq, 'q': q, 'build': build},
                      wloops=wl, loops_every=loops_every, late={'inst_acc': k / 2, 'inst_dq': k})
    assert list(h) == ['traj', 'dt', 'acc', 'dH', 'plaq', 'q', 'dq', 'build', 'wloops', 'inst_acc', 'inst_dq']
    assert h['traj'] == [n * ntraj + i + 1 for i in range(ntraj)] and h['dt'] == [0.25] * ntraj and h['build'] == build
    prev = np.concatenate([q0[None], q[:-1]])
    for i in range(ntraj):
        assert np.array_equal(h['dq'][i].numpy(), np.sqrt((q[i] - prev[i]) ** 2))
        for key, col in (('acc', np.ones((ntraj, B))), ('dH', dH), ('plaq', plaq), ('q', q), ('inst_acc', k / 2), ('inst_dq', k)):
            e = h[key][i]
            assert isinstance(e, torch.Tensor) and e.device.type == 'cpu' and e.shape == (B,) and np.array_equal(e.numpy(), col[i]), key
    assert h['inst_dq'][0].dtype == torch.int32 and h['inst_acc'][0].dtype == torch.float64 and h['acc'][0].dtype == torch.float64
    measured = [i for i in range(ntraj) if i % loops_every == 0]
    assert len(h['wloops']) == len(measured) and all(np.array_equal(t.numpy(), wl[i]) for t, i in zip(h['wloops'], measured))
    h['q'][0][0] = 99.0                                                                  # entries are copies: the rows stay what they were
    assert q[0, 0] != 99.0
    # without the options the keys are run_local's; before a trajectory has been recorded, the late keys do not exist
    h = chain_history(1, 0.5, q0, {'acc': np.ones((ntraj, B)), 'plaq': plaq, 'q': q})
    assert list(h) == ['traj', 'dt', 'acc', 'plaq', 'q', 'dq'] and h['traj'][0] == 1
    empty = np.zeros((0, B))
    h = chain_history(1, 0.5, q0, {'acc': empty, 'plaq': empty, 'q': empty}, wloops=np.zeros((0, 2, 3)), late={'inst_acc': empty})
    assert h == {'traj': [], 'dt': [], 'acc': [], 'plaq': [], 'q': [], 'dq': []}


def test_shared_checks_raise_what_the_drivers_raised():
    L = 8
    for bad in (0, (L + 1, 1), (1, L + 1), (0, 3)):
        with pytest.raises(ValueError) as e:
            loops_arg(bad, L)
        assert str(e.value) == f'loops: (Rmax, Tmax) with 1 <= Rmax, Tmax <= L = {L} expected, got {bad!r}'
    assert loops_arg(None, L) is None and loops_arg(3, L) == (3, 3) and loops_arg([2, L], L) == (2, L) and loops_arg((1, 1), L) == (1, 1)
    for bad in (-1, 1025):
        with pytest.raises(ValueError) as e:
            instanton_arg(bad)
        assert str(e.value) == f'instanton: a number of hits in 0 .. 1024 expected, got {bad}'
        with pytest.raises(ValueError) as e:
            instanton_arg(bad, 'run_local')
        assert str(e.value) == f'run_local: instanton: a number of hits in 0 .. 1024 expected, got {bad}'
    assert instanton_arg(0) == 0 and instanton_arg(1024, 'run_local') == 1024 and instanton_arg(True) == 1
    from fthmc_amd.ft_hmc import FieldTransformation, LazyHistory
    from fthmc_amd import graph_loop
    assert FieldTransformation._loops_arg is loops_arg and LazyHistory is graph_loop.LazyHistory


def test_the_graph_default_is_read_in_one_place(monkeypatch):
    from fthmc_amd.graph_loop import run_graph_default
    for val, want in ((None, True), ('1', True), ('0', False), ('', False), ('yes', True)):
        if val is None:
            monkeypatch.delenv('FTHMC_RUN_GRAPH', raising=False)
        else:
            monkeypatch.setenv('FTHMC_RUN_GRAPH', val)
        assert run_graph_default() is want
    import glob, os
    import fthmc_amd
    root = os.path.dirname(fthmc_amd.__file__)
    readers = [p for p in glob.glob(os.path.join(root, '**', '*.py'), recursive=True) if "environ.get('FTHMC_RUN_GRAPH'" in open(p).read()]
    assert [os.path.relpath(p, root) for p in readers] == ['graph_loop.py']
