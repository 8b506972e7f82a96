"""CPU-only tests of the instanton hit (the Metropolis update across topological sectors): the C ABI declares and exports the entry
points and the wrappers, the operator schema and the `fthmc` aliases exist, the refusals refuse; the numpy twin of
tests/instanton_cases.py has the closed-form action difference, moves the charge by k, forms its shifts from reduced integers and
stays inside its own derived bound when run in float64; the exact charge distribution; the twin as a sampler against it; the entry
point's host side and the integer reductions as a stand-alone program under AddressSanitizer + UBSan."""
import inspect
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import instanton_cases as IC
import local_update_cases as LC

LD = np.longdouble
Q2_EXACT = {(4, 1.5): 0.4388851871, (8, 4.0): 0.4820159295, (8, 6.0): 0.2792008453, (16, 6.0): 1.1947014482, (64, 6.0): 19.1152232818}


def test_header_library_wrappers_schema_and_alias_carry_the_new_entry_points():
    import ctypes
    from fthmc_amd import _lib, ops
    import fthmc_amd.torch_ops as TO
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'fthmc_hip.h')).read()
    declared = set(re.findall(r'\b(fthmc_[a-z0-9_]+)\s*\(', header))
    for name in ('fthmc_instanton_hit', 'fthmc_instanton_ws_bytes'):
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    sig = _lib.SIGNATURES['fthmc_instanton_hit']
    assert len(sig) == 16 and sig[3] is ctypes.c_double and sig[7] is ctypes.c_int64 and sig[14] is ctypes.c_size_t
    assert len(_lib.SIGNATURES['fthmc_instanton_ws_bytes']) == 3 and lib.fthmc_instanton_ws_bytes.restype is ctypes.c_size_t
    p = inspect.signature(ops.instanton_hit).parameters
    assert list(p) == ['x', 'beta', 'seeds', 'n_hit', 'hit0', 'path', 'out']
    assert (p['n_hit'].default, p['hit0'].default, p['path'].default, p['out'].default) == (1, 0, 0, None)
    assert list(inspect.signature(ops.instanton_sums).parameters)[0] == 'x'
    schema = str(torch.ops.fthmc_hip.instanton_hit.default._schema)
    assert schema == 'fthmc_hip::instanton_hit(Tensor x, float beta, Tensor? beta_b, Tensor? seeds, int n_hit=1, int hit0=0) -> (Tensor, Tensor, Tensor)', schema
    assert 'instanton_hit' in TO.__all__
    y = torch.ops.fthmc_hip.instanton_hit(torch.empty(3, 2, 8, 8, dtype=torch.float64, device='meta'), 2.0, None, None, 0)
    assert [tuple(t.shape) for t in y] == [(3, 2, 8, 8), (3,), (3,)] and [t.dtype for t in y] == [torch.float64, torch.int32, torch.int32]
    import fthmc.local as l1
    import fthmc.utils.qed_helpers as q1
    import fthmc.utils.observables as o1
    import fthmc_amd.utils.qed_helpers as q2
    from fthmc.hmc import run_hmc
    assert q1 is q2 and callable(q1.instanton_hit) and callable(o1.exact_charge_distribution) and callable(o1.exact_charge_moment)
    p = inspect.signature(q1.instanton_hit).parameters
    assert list(p) == ['param', 'x', 'n_hit', 'seeds'] and p['n_hit'].default == 1 and p['seeds'].default is None
    for f in (run_hmc, l1.run_local, q1.ft_run):
        assert inspect.signature(f).parameters['instanton'].default == 0, f
    assert inspect.signature(o1.exact_charge_moment).parameters['power'].default == 2
    assert list(inspect.signature(o1.exact_charge_distribution).parameters)[:3] == ['beta', 'L', 'qmax']


def test_refusals_refuse_and_the_workspace_rule():
    """the argument checks of the C entry point come before anything touches the device: stand-in addresses are never read"""
    from fthmc_amd import _lib, ops
    from fthmc_amd._lib import FthmcError
    lib = _lib.load()
    X, S, O, W = 0x10000000, 0x20000000, 0x30000000, 0x40000000
    ARG, WS = -1, -4

    def call(x=X, B=2, L=8, beta=2.0, bb=None, seeds=S, n_hit=1, hit0=0, path=1, out=O, ws=None, nb=0):
        return lib.fthmc_instanton_hit(x, B, L, beta, bb, seeds, n_hit, hit0, path, out, None, None, None, ws, nb, None)
    assert call(x=None) == ARG and call(out=None) == ARG and call(seeds=None) == ARG
    for B in (0, -1, 4194304):
        assert call(B=B) == ARG
    for L in (0, 2, 6, 10, -8, 32768):
        assert call(L=L) == ARG
    for n in (-1, 1025, 2 ** 31 - 1):
        assert call(n_hit=n) == ARG
    for p in (-1, 3, 255):
        assert call(path=p) == ARG
    assert call(hit0=-1) == ARG and call(hit0=2 ** 32) == ARG and call(hit0=2 ** 32 - 63, n_hit=64) == ARG and call(hit0=2 ** 62) == ARG
    assert call(hit0=-2 ** 63) == ARG and call(hit0=2 ** 63 - 1, n_hit=1024) == ARG
    # the workspace: none for one workgroup per chain, part[B][nw][2] doubles + k[B] int32 for the split form; path 0 splits when
    # B < 64 and L >= 128
    wsb = lib.fthmc_instanton_ws_bytes
    assert wsb(2, 8, 1) == 0 and wsb(2, 128, 1) == 0 and wsb(2, 8, 0) == 0 and wsb(64, 128, 0) == 0 and wsb(2, 124, 0) == 0
    # (rounded up to a multiple of 256 bytes, like every workspace size: tests/test_workspace_contract.py)
    up = lambda n: (n + 255) // 256 * 256
    assert wsb(2, 8, 2) == up(2 * 4 * 2 * 8 + 8) == 256 and wsb(3, 128, 0) == wsb(3, 128, 2) == up(3 * 16 * 2 * 8 + 16) == 1024
    assert wsb(63, 128, 0) > 0
    assert wsb(0, 8, 2) == 0 and wsb(2, 6, 2) == 0 and wsb(2, 8, 3) == 0 and wsb(2, 8, -1) == 0
    need = wsb(2, 8, 2)
    assert call(path=2) == WS and call(path=2, ws=W, nb=need - 1) == WS and call(path=2, ws=None, nb=need) == WS
    assert call(B=3, L=128, path=0) == WS
    assert call(x=None, path=2) == ARG                                   # the arguments come first
    x = torch.zeros(2, 2, 8, 8, dtype=torch.float64)
    with pytest.raises(FthmcError):
        ops.instanton_hit(x, 2.0, None, n_hit=0)                         # a CPU tensor: there is no CPU fallback
    with pytest.raises(FthmcError):
        ops.instanton_sums(x)
    import fthmc_amd.torch_ops  # noqa: F401
    with pytest.raises(NotImplementedError):
        torch.ops.fthmc_hip.instanton_hit(x, 2.0, None, None, 0)


# ---------------------------------------------------------------- the twin: the construction
@pytest.mark.parametrize('L', [4, 8, 12])
def test_twin_closed_form_equals_the_direct_action_difference(L):
    beta = 2.0
    x = LC.uniform_links(3, L, 50 + L)
    C, Sn, dC, dSn = IC.sums(x)
    assert np.all(np.abs((C - IC.action_sum(x)).astype(np.float64)) <= dC)          # the device's order of addition, the same sum
    A = IC.instanton(L)
    for k in (1, -1, 3, -3, L * L // 2):
        direct = -LD(beta) * (IC.action_sum(x.astype(LD) + k * A) - IC.action_sum(x))
        closed, bound = IC.path_delta_s(C, Sn, beta, k, L, dC=dC, dSn=dSn)
        err = np.abs((direct - closed).astype(np.float64))
        print(f'L {L} k {k}: closed - direct {err.max():.2e}, bound {bound.min():.2e}')
        assert np.all(err <= bound), (k, err, bound)
        assert np.all(err <= 1e-13 * abs(k))                             # and far inside it: both sides are long double


@pytest.mark.parametrize('L', [4, 8, 12])
def test_twin_charge_moves_by_k_and_shifts_come_from_reduced_integers(L):
    V = L * L
    smooth, rough = LC.uniform_links(3, L, 60 + L, 0.3), LC.uniform_links(3, L, 70 + L)
    q0, d0 = IC.charge(smooth)
    assert np.all(q0 == 0) and d0.max() < 1e-15
    A = IC.instanton(L)
    for k in (1, -1, 3, -3, V // 2, -5 * V + 2, 1024, -1024):
        kk = np.full(3, k)
        xs, moved, _ = IC.apply_charge(smooth, kk)
        if abs(k) <= 3:                                                  # |P + k w| stays below pi: no plaquette wraps
            q, d = IC.charge(xs)
            assert np.all(q == k) and d.max() < 1e-15, (k, q)
        xr, moved_r, _ = IC.apply_charge(rough, kk)
        qa, da = IC.charge(xr)
        qb, db = IC.charge(rough.astype(LD) + k * A)                     # the unreduced x + k A
        assert np.array_equal(qa, qb) and max(da.max(), db.max()) < 1e-14 * V, (k, qa, qb)
        # the shifts: reduced = unreduced mod 2 pi
        s1, r1 = IC.shift_x1(kk, L)
        s1u, _ = IC.shift_x1(kk, L, reduced=False)
        ss, rs = IC.shift_seam(kk, L)
        ssu, _ = IC.shift_seam(kk, L, reduced=False)
        assert np.all((r1 >= 0) & (r1 < V)) and np.all((rs >= 0) & (rs < L))
        assert np.all(s1.astype(np.float64) < 2 * math.pi) and np.all(ss.astype(np.float64) < 2 * math.pi)
        tol = 2.0 ** -60 * (1 + abs(k) * L)
        assert LC.circ_dist(s1, s1u).max() <= tol and LC.circ_dist(ss, ssu).max() <= tol
        assert LC.circ_dist(xr, rough.astype(LD) + k * A).max() <= 2.0 ** -58 * (1 + abs(k) * L)
        # zero-shift links are bit-equal: all of x0 above its last row, row 0 of x1, column 0 of the seam, and whatever else reduces to 0
        assert not moved_r[:, 0, :L - 1].any() and not moved_r[:, 1, 0].any() and not moved_r[:, 0, L - 1, 0].any()
        assert np.array_equal(xr.astype(np.float64)[~moved_r], rough[~moved_r])
        assert moved_r.any() == (k % V != 0 or k % L != 0)
    x0, m0, b0 = IC.apply_charge(rough, np.zeros(3, dtype=np.int64))
    assert not m0.any() and np.array_equal(x0.astype(np.float64), rough) and not b0.any()


def test_twin_draws_use_counter_plane_four_and_both_signs():
    import philox_ref as PR
    seeds = LC.chain_seeds(4, 9)
    u, s = IC.draws(seeds, 300, 2 ** 32 - 300)
    assert np.all((u >= 0) & (u < 1)) and set(np.unique(s)) == {-1, 1} and abs(s.mean()) < 0.12 and abs(u.mean() - 0.5) < 0.06
    k0, k1 = PR._key(seeds)
    w = PR.philox4x32_10((2 ** 32 - 1, 0, 4, 0), (k0, k1))
    assert np.array_equal(u[:, -1], PR.accept_u(PR.u53(w[0], w[1]))) and np.array_equal(s[:, -1] > 0, (w[2] & np.uint64(1)) == 1)
    u2, s2 = IC.draws(seeds, 5, 7)
    u1 = np.concatenate([IC.draws(seeds, 1, 7 + h)[0] for h in range(5)], axis=1)
    assert np.array_equal(u2, u1)


# ---------------------------------------------------------------- the twin inside its own bound
@pytest.mark.parametrize('B,L,amp,beta', IC.CASES, ids=lambda v: f'{v:g}')
def test_float64_twin_stays_inside_the_derived_bound_and_no_chain_is_left_out(B, L, amp, beta):
    """the bound is derived for fp64 arithmetic: the same formulas in float64 numpy must land inside it; and on the fields and seeds
    the device tests use (IC.case) no accept decision is closer than its bound: no chain is left out"""
    for n_hit, hit0 in IC.HITS:
        x, seeds, a = IC.case(B, L, amp, beta, n_hit, hit0)
        b = IC.hits(x, beta, seeds, n_hit, hit0, dt=np.float64)
        assert not a['ambiguous'].any() and not b['ambiguous'].any()
        assert np.array_equal(a['k'], b['k']) and np.array_equal(a['nacc'], b['nacc']) and np.array_equal(a['accepted'], b['accepted'])
        assert np.array_equal(a['s'], b['s']) and np.array_equal(a['u'], b['u'])
        eC = np.abs((a['C'] - b['C']).astype(np.float64)) / a['dC']
        eS = np.abs((a['Sn'] - b['Sn']).astype(np.float64)) / a['dSn']
        eD = np.abs((a['dS'] - b['dS']).astype(np.float64)) / a['dS_bound']
        mv = a['moved']
        assert np.array_equal(mv, b['moved'])
        d = LC.circ_dist(a['x'], b['x'].astype(LD))
        assert max(eC.max(), eS.max(), eD.max()) <= 1.0, (n_hit, eC.max(), eS.max(), eD.max())
        assert not d[~mv].any() and np.array_equal(b['x'][~mv], x[~mv])
        if mv.any():
            assert float((d[mv] / a['bound'][mv]).max()) <= 1.0
            assert float(np.median(a['bound'][mv])) < 1e-13              # a bound that still sees an index error
        assert float(a['dC'].max()) < 1e-14 * L * L * max(1.0, amp)      # and one that still sees a missing site
        assert int(np.abs(a['k']).max()) <= n_hit and np.all(a['nacc'] >= np.abs(a['k']))


# ---------------------------------------------------------------- the exact charge distribution
@pytest.mark.parametrize('L,beta', sorted(Q2_EXACT))
def test_exact_charge_distribution(L, beta):
    from fthmc_amd.utils import observables as O
    qmax = 40 if L == 64 else 16
    p = O.exact_charge_distribution(beta, L, qmax)
    assert p.shape == (2 * qmax + 1,) and abs(p.sum() - 1.0) <= 1e-10 and np.abs(p - p[::-1]).max() <= 1e-14 and p.min() > -1e-14
    Q = np.arange(-qmax, qmax + 1)
    q2 = float((Q ** 2 * p).sum())
    assert abs(q2 - Q2_EXACT[(L, beta)]) <= 1e-7 * Q2_EXACT[(L, beta)], q2
    m = O.exact_charge_moment(beta, L)
    assert abs(m - Q2_EXACT[(L, beta)]) <= 1e-7 * Q2_EXACT[(L, beta)], m
    assert abs(O.exact_charge_moment(beta, L, power=1)) <= 1e-12 and abs(O.exact_charge_moment(beta, L, power=0) - 1.0) <= 1e-10
    assert np.argmax(p) == qmax
    if (L, beta) == (64, 6.0):
        large_beta = L * L / (4 * math.pi ** 2 * beta)
        assert abs(m - large_beta) <= 0.15 * m
        assert abs(O.exact_charge_distribution(beta, L, 30).sum() - 1.0) <= 1e-10
        assert abs(O.exact_charge_distribution(beta, L, 12).sum() - 1.0) > 1e-4           # the tail is the caller's to cover


# ---------------------------------------------------------------- the twin as a sampler
def test_twin_sampler_reproduces_the_exact_charge_distribution():
    """heatbath sweeps (LC.sweep) each followed by two twin hits at L = 4, beta = 1.5 from a random start: <Q^2> and P(0) against the
    exact finite-volume values, the standard error from the chain means"""
    from fthmc_amd.utils import observables as O
    B, L, beta, ntherm, nmeas, n_hit = 256, 4, 1.5, 30, 150, 2
    x = LC.uniform_links(B, L, 91)
    seeds_hb, seeds_hit = LC.chain_seeds(B, 92), LC.chain_seeds(B, 93)
    q2, p0, acc = np.zeros(B), np.zeros(B), 0.0
    for t in range(ntherm + nmeas):
        x = LC.sweep(x, beta, seeds_hb, t)
        r = IC.hits(x, beta, seeds_hit, n_hit, hit0=n_hit * t, dt=np.float64)
        x = r['x'].astype(np.float64)
        if t >= ntherm:
            q, d = IC.charge(x)
            assert d.max() < 1e-12
            q2 += q ** 2; p0 += q == 0; acc += r['nacc'].mean() / n_hit
    q2, p0, acc = q2 / nmeas, p0 / nmeas, acc / nmeas
    p = O.exact_charge_distribution(beta, L, 8)
    for name, v, exact in (('<Q^2>', q2, Q2_EXACT[(4, 1.5)]), ('P(0)', p0, float(p[8]))):
        se = v.std(ddof=1) / math.sqrt(B)
        z = (v.mean() - exact) / se
        print(f'{name}: {v.mean():.5f} +- {se:.5f}, exact {exact:.5f}, z {z:+.2f}; hit acceptance {acc:.3f}')
        assert abs(z) <= 4.0, (name, z)
    assert 0.2 < acc < 0.7


# ---------------------------------------------------------------- the entry point under the sanitizers
def test_instanton_entry_point_walks_clean_under_asan_and_ubsan(tmp_path):
    """tests/hip/instanton_walk.cpp: a stand-alone program against the host-side sanitizer build of the library (launches are no-ops
    there), built with -fsanitize=address,undefined by the recipe next to `make san`'s: every refusal, the hit0 arithmetic at its
    edges, legal calls on both paths up to the largest shapes, and the integer reductions of csrc/topo_int.h walked for the largest
    |k| at the smallest and the largest L.  Its own process, nothing preloaded."""
    csrc = os.path.join(ROOT, 'fthmc_amd', 'csrc')
    exe = str(tmp_path / 'instanton_walk')
    r = subprocess.run(['make', '-C', csrc, '-f', 'san.mk', 'san_instanton', 'SANINST=' + exe], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and os.path.exists(exe), r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ)
    env.update(ASAN_OPTIONS='detect_leaks=1:abort_on_error=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error:' not in r.stderr, r.stderr[-6000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out['calls'] > 200 and out['refusals'] >= 40 and out['reductions'] > 100000
