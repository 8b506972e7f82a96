"""CPU-only: the workspace layouts of csrc/api_call.h (ws_layout, vjp_layout, force_layout and the carver under them).

  * Every size query answers what it answered before the layouts were restated on one carver: tests/golden/ws_sizes.json, recorded
    by tests/golden/make_ws_sizes.py from the library of the commit before.  The scratch contract tests
    (tests/test_workspace_contract_gpu.py) run in scratch of exactly the queried size: a query and a layout that shrank together
    would pass them, and fail here.
  * Where a size leaves size_t, all four workspace queries answer 0 together.
  * tests/hip/layout_walk.cpp walks the three layouts stand-alone under AddressSanitizer + UBSan (with the unsigned-overflow
    check): order, disjointness, alignment and end of the regions, the null base, the public queries, the edge of size_t.
"""
import importlib.util
import json
import os
import subprocess

from conftest import ROOT

GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def _generator():
    spec = importlib.util.spec_from_file_location('make_ws_sizes', os.path.join(GOLDEN, 'make_ws_sizes.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _untuple(a):
    return [_untuple(v) for v in a] if isinstance(a, (tuple, list)) else a


def test_every_size_query_answers_what_it_answered_before_the_restatement():
    from fthmc_amd import _lib, ops
    G, lib = _generator(), _lib.load()
    doc = json.load(open(os.path.join(GOLDEN, 'ws_sizes.json')))
    archs = G.archs()
    # the file is the generator's grid: every net shape, every B, L and layer count of the grid, a few hundred rows
    assert doc['archs'] == _untuple(archs) and doc['columns'] == ['arch', 'B', 'L', 'n_layers'] + list(G.COLUMNS)
    assert [tuple(r[:4]) for r in doc['rows']] == G.grid() and 300 <= len(doc['rows']) <= 400
    for col, values in ((0, range(len(archs))), (1, G.BS), (2, G.LS), (3, G.NLS)):
        assert {r[col] for r in doc['rows']} == set(values)
    assert int(lib.fthmc_ws_head_bytes()) == doc['head_bytes']
    wrong = [(r[:4], name, was, now) for r in doc['rows']
             for name, was, now in zip(G.COLUMNS, r[4:], G.query(lib, ops, archs[r[0]], *r[1:4])) if was != now]
    assert wrong == [], wrong[:10]
    assert all(r[4] > doc['head_bytes'] for r in doc['rows'])                      # ... and none of them is a refusal's 0


def test_sizes_beyond_size_t_are_zero_in_all_four_workspace_queries():
    """the overflowing shapes of tests/test_force_training.py (test_train_force_workspace_sizes), legal in B and L: fthmc_ws_bytes
    and fthmc_train_ws_bytes wrapped there, fthmc_vjp_ws_bytes and fthmc_train_force_ws_bytes answered 0"""
    from fthmc_amd import _lib, ops
    lib = _lib.load()
    queries = (lib.fthmc_ws_bytes, lib.fthmc_train_ws_bytes, lib.fthmc_vjp_ws_bytes, lib.fthmc_train_force_ws_bytes)
    for a in (None, ((4, 6), 5, 3)):
        ap = ops._arch(a)
        for B, L, nl in ((4194303, 32764, 64), (1 << 20, 32764, 1 << 20), (1, 32764, (1 << 31) - 1), (4194303, 64, (1 << 31) - 1)):
            assert [int(q(ap, B, L, nl)) for q in queries] == [0, 0, 0, 0], (a, B, L, nl)
        # the largest legal lattice with one chain and a few layers is far from the edge: every query answers
        assert all(int(q(ap, 1, 32764, 2)) > 0 for q in queries), a


def test_layouts_walk_clean_under_asan_and_ubsan(tmp_path):
    """tests/hip/layout_walk.cpp: a stand-alone program that includes csrc/api_call.h, built with -fsanitize=address,undefined (and
    the unsigned-overflow check) by the recipe next to `make san`'s and linked against the host-side sanitizer build of the library
    for the public queries.  Its own process, nothing preloaded."""
    csrc = os.path.join(ROOT, 'fthmc_amd', 'csrc')
    exe = str(tmp_path / 'layout_walk')
    r = subprocess.run(['make', '-C', csrc, '-f', 'san.mk', 'san_layout', 'SANLAYOUT=' + exe], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and os.path.exists(exe), r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ)
    env.update(ASAN_OPTIONS='detect_leaks=1:abort_on_error=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error:' not in r.stderr, r.stderr[-6000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out['failed'] == 0 and out['layouts'] > 30000 and out['regions'] > 400000 and out['queries'] > 20000 and out['overflows'] >= 200
