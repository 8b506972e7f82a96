"""The random draws of csrc/rng.hip held to a stream definition outside the kernels (tests/philox_ref.py, pinned by
tests/test_rng_reference.py): Philox4x32-10 blocks, the three counter planes, u53, the accept uniform and the prior bit for bit,
Box-Muller within a derived bound, at the shapes where the kernels' pair loop, odd tail and grid-stride loop differ; the device
chain seeds past one workgroup's width; and the accept step of every trajectory kernel at the ends of u's range.

The helpers of csrc/rng_common.h are also applied to free words (tests/hip/device_probe.hip), which reaches the ends of u53's
range: no seed gets there in a test's lifetime.

The Box-Muller bound.  v = rad (cos, sin)(FT_TWO_PI u2), rad = sqrt(-2 log u1), all in fp64.  Per element, in units of
rad 2^-53 (half an ulp of a value in [1, 2) times rad):
    rounding of the argument FT_TWO_PI u2: half an ulp on [4, 8) = 2^-51 = 4 units, |d sin|, |d cos| <= 1            4
    the fp64 2 pi's own error, 2.449e-16, times u2 <= 1                                                              2.21
    sincos: 2 ulp of a result <= 1, an ulp there being at most 2^-53 ... 2^-52: 2 units at 2 ulp of [1/2, 1)         2
    log: 1 ulp relative on -2 log u1, halved by the square root; the correctly rounded sqrt's own half ulp:
        relative 2^-53 + 2^-53 on rad                                                                                2
    the product's rounding, half an ulp of |v| <= rad                                                                1
                                                                                                             total   11.2
and the test asks for 12.  The two library terms are taken as given: sincos at 2 ulp and log at 1 ulp are what the ROCm
documentation's HIP math API reference (double precision functions, maximum ulp error) states for the device library's fp64
functions, sqrt being the correctly rounded IEEE one; no copy of that table ships with the toolchain, so nothing here re-reads
it, and the measured maxima are the check on those two terms.
Not yet measured on an MI355X: the tests print their maxima (test_draws_from_random_words, test_box_muller_at_the_axes,
test_momenta_through_the_c_abi); the CPU fp64 restatement of the same expressions reaches 6.35 over the seeds and n of
test_momenta_through_the_c_abi.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import philox_ref as PR
from conftest import ROOT
from fthmc_amd import parallel
from gpu_support import R, capture, module_defaults, ops, switches

pytestmark = pytest.mark.gpu
_defaults = module_defaults()

import mpmath          # a plain import: a missing mpmath must fail this file, not skip its bit-exact tests

mpmath.mp.dps = 40

CSRC = os.path.join(ROOT, 'fthmc_amd', 'csrc')
PROBE = os.path.join(ROOT, 'tests', 'hip', 'libdevice_probe.so')
LD = np.longdouble
U = 2.0 ** -53
BM_BOUND = 12.0                                      # units of rad 2^-53: derived above
RAD_MAX = math.sqrt(2 * 53 * math.log(2))            # k1 = 1
_U32 = ctypes.POINTER(ctypes.c_uint32)
_D = ctypes.POINTER(ctypes.c_double)
NS = [1, 2, 3, 511, 512, 513, 16383, 16384, 16385, 32768, 131071, 131072]
EDGE_SEEDS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1]
GUARD = 64


@pytest.fixture(scope='module')
def probe():
    r = subprocess.run(['make', '-C', CSRC, 'probe'], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'warning' not in (r.stdout + r.stderr).lower(), r.stdout[-3000:] + r.stderr[-3000:]
    lib = ctypes.CDLL(PROBE)
    lib.probe_philox.argtypes = [_U32, _U32, _U32, ctypes.c_int]
    lib.probe_draws.argtypes = [_U32, ctypes.c_double, ctypes.c_double, _D, ctypes.c_int]
    return lib


def philox_dev(lib, ctr, key):
    ctr = np.ascontiguousarray(ctr, dtype=np.uint32)
    key = np.ascontiguousarray(key, dtype=np.uint32)
    out = np.zeros_like(ctr)
    rc = lib.probe_philox(ctr.ctypes.data_as(_U32), key.ctypes.data_as(_U32), out.ctypes.data_as(_U32), len(ctr))
    assert rc == 0, f'probe_philox: HIP error {rc}'
    return out


def draws_dev(lib, k1, k2, lo=0.0, hi=1.0, low_bits=0):
    """the probe's seven planes for word blocks whose u53 integers are (k1, k2) -> dict; low_bits: the 11 bits below m"""
    h1, l1 = PR.words_of(k1)
    h2, l2 = PR.words_of(k2)
    w = np.ascontiguousarray(np.stack([h1, l1 | np.uint32(low_bits), h2, l2 | np.uint32(low_bits)], axis=1), dtype=np.uint32)
    n = len(w)
    out = np.full((7, n), np.nan)
    rc = lib.probe_draws(w.ctypes.data_as(_U32), float(lo), float(hi), out.ctypes.data_as(_D), n)
    assert rc == 0, f'probe_draws: HIP error {rc}'
    return dict(zip(('u1', 'u2', 'a', 'b', 'acc', 'p1', 'p2'), out))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def ku(vals):
    return np.array(vals, dtype=np.uint64)


def bm_units(dev, ref_ld, rad_ld):
    """|dev - ref| in units of rad 2^-53 (longdouble reference); 0 where rad = 0 and the device value is +-0"""
    d = np.abs(np.asarray(dev, dtype=LD) - ref_ld)
    r = np.asarray(rad_ld, dtype=LD) * LD(U)
    out = np.where(r > 0, d / np.where(r > 0, r, 1), np.where(d == 0, 0.0, np.inf))
    return np.asarray(out, dtype=np.float64)


def seed_set():
    return torch.cat([torch.tensor(EDGE_SEEDS, dtype=torch.int64), parallel.chain_seeds(1331, 0, 3, 0)])


def guarded(B, n):
    """-> (buffer full of NaN, its inner [B, n] view)"""
    buf = torch.full((B * n + 2 * GUARD,), float('nan'), dtype=torch.float64, device='cuda')
    return buf, buf[GUARD:GUARD + B * n].view(B, n)


def check_guard(buf, B, n, what):
    h = buf.cpu().numpy()
    assert np.isnan(h[:GUARD]).all() and np.isnan(h[GUARD + B * n:]).all(), f'{what}: written outside its {B} x {n} elements'
    inner = h[GUARD:GUARD + B * n].reshape(B, n)
    assert not np.isnan(inner).any(), f'{what}: {int(np.isnan(inner).sum())} of {B} x {n} elements not written'
    return inner


# ----------------------------------------------------------------------------------------------------------- the probe: Philox
def test_philox_blocks_equal_the_reference(probe):
    """csrc/rng_common.h philox4x32_10 = Philox4x32-10: Random123's known answers and 10^6 random (counter, key) pairs, bit for bit"""
    KAT = PR.KAT
    ctr = np.array([k[0] for k in KAT], dtype=np.uint32)
    key = np.array([k[1] for k in KAT], dtype=np.uint32)
    assert np.array_equal(philox_dev(probe, ctr, key), np.array([k[2] for k in KAT], dtype=np.uint32))
    g = np.random.default_rng(11)
    n = 10 ** 6
    ctr = g.integers(0, 2 ** 32, (n, 4), dtype=np.uint64).astype(np.uint32)
    key = g.integers(0, 2 ** 32, (n, 2), dtype=np.uint64).astype(np.uint32)
    # the counters the kernels form: (p, 0, plane, 0) with small p
    ctr[:1000] = np.stack([np.arange(1000), np.zeros(1000), np.arange(1000) % 3, np.zeros(1000)], axis=1).astype(np.uint32)
    ref = np.stack(PR.philox4x32_10([ctr[:, i] for i in range(4)], [key[:, i] for i in range(2)]), axis=1).astype(np.uint32)
    dev = philox_dev(probe, ctr, key)
    bad = np.flatnonzero((dev != ref).any(axis=1))
    assert bad.size == 0, (bad.size, ctr[bad[0]], key[bad[0]], dev[bad[0]], ref[bad[0]])


# ----------------------------------------------------------------------------------------------------------- the probe: edges
def test_u53_top_of_range_m_all_ones(probe):
    """m = 2^53 - 1: u53 = 1 exactly, so rad = sqrt(-2 log 1) = 0 and both normals are zeros (of either sign), finite, for any
    angle; the accept uniform is 0; the prior is `lo` exactly"""
    k2 = ku([1, 2, 1 << 51, (1 << 51) + 1, 1 << 52, 3 << 51, (1 << 53) - 1, 1 << 53, 12345678901234])
    k1 = np.full(len(k2), 1 << 53, dtype=np.uint64)
    for low in (0, 0x7ff):                                           # the 11 bits below m do not count
        for lo, hi in ((-math.pi, math.pi), (0.0, 1.0), (1e6, 1e6 + 1)):
            d = draws_dev(probe, k1, k2, lo, hi, low)
            assert np.all(d['u1'] == 1.0)
            assert np.all(d['a'] == 0.0) and np.all(d['b'] == 0.0), (d['a'], d['b'])
            assert np.all(d['acc'] == 0.0) and not np.signbit(d['acc']).any()
            assert np.all(d['p1'] == lo)
            assert np.array_equal(d['u2'], k2.astype(np.float64) * U)
            sw = draws_dev(probe, k2, k1, lo, hi, low)               # the second word pair at the top: the prior's second value
            assert np.all(sw['p2'] == lo) and np.all(sw['u2'] == 1.0)


def test_u53_bottom_of_range_m_zero(probe):
    """m = 0: u53 = 2^-53 > 0, log never sees 0: rad = sqrt(106 ln 2) = 8.57, the largest momentum there is; the accept uniform
    is 1 - 2^-53 < 1; the prior on (-pi, pi) is below pi (and is the correctly rounded value)"""
    k2 = ku([1, 2, 1 << 51, (1 << 51) + 1, 1 << 52, 3 << 51, (1 << 53) - 1, 1 << 53, 12345678901234, 1 << 50])
    k1 = np.ones(len(k2), dtype=np.uint64)
    for low in (0, 0x7ff):
        d = draws_dev(probe, k1, k2, -math.pi, math.pi, low)
        assert np.all(d['u1'] == U)
        assert np.all(np.isfinite(d['a'])) and np.all(np.isfinite(d['b']))
        for i in range(len(k2)):
            ma, mb, mr = PR.normal_pair_mp(1, k2[i])
            assert abs(float(mr) - RAD_MAX) < 1e-14
            for dev, ref in ((d['a'][i], ma), (d['b'][i], mb)):
                assert abs(mpmath.mpf(float(dev)) - ref) <= BM_BOUND * mr * U, (int(k2[i]), float(dev), float(ref))
        assert max(np.abs(d['a']).max(), np.abs(d['b']).max()) <= RAD_MAX * (1 + BM_BOUND * U)
        assert np.all(d['acc'] == 1.0 - U)
        top = PR.uniform_exact([1], -math.pi, math.pi)[0]
        assert np.all(d['p1'] == top) and top < math.pi
        d01 = draws_dev(probe, k1, k2, 0.0, 1.0, low)
        assert np.all(d01['p1'] == 1.0 - U)


def test_box_muller_at_the_axes(probe):
    """u2 words that put the angle 2 pi u2 next to 0, pi / 2, pi, 3 pi / 2 and 2 pi -- where one of the two values passes
    through 0 and the fp64 2 pi's own error is the whole result (at u2 = 1: sin(fl(2 pi)) = -2.449e-16, 2.21 units) -- against
    mpmath, within the derived bound"""
    k2 = []
    for c in (0, 1 << 51, 1 << 52, 3 << 51, 1 << 53):
        k2 += [c + j for j in range(-4, 5) if 1 <= c + j <= 1 << 53]
    k1s = [1, 2, 1 << 30, 1 << 52, (1 << 53) - 1, 6004799503160661, 3]
    K1, K2 = np.meshgrid(ku(k1s), ku(k2))
    K1, K2 = K1.ravel(), K2.ravel()
    d = draws_dev(probe, K1, K2)
    worst = 0.0
    for i in range(len(K1)):
        ma, mb, mr = PR.normal_pair_mp(K1[i], K2[i])
        for dev, ref in ((d['a'][i], ma), (d['b'][i], mb)):
            e = float(abs(mpmath.mpf(float(dev)) - ref) / (mr * U))
            worst = max(worst, e)
            assert e <= BM_BOUND, (int(K1[i]), int(K2[i]), float(dev), float(ref), e)
    print(f'Box-Muller at the axes: max {worst:.3f} units of rad 2^-53 (bound {BM_BOUND})')


def test_prior_on_a_general_range(probe):
    """fthmc_random_uniform's value is the correctly rounded (1 - k / 2^53) w + lo with w = fl(hi - lo) -- one fma -- on any
    range.  That is >= lo always and < hi on (0, 1) and (-pi, pi); it is NOT below hi on every range: where the width is small
    next to |lo| -- (1e6, 1e6 + 1): the spacing of doubles there is 1.16e-10, the top value is 1.1e-16 below hi -- the rounding
    reaches hi itself.  The device returns hi there, as the correctly rounded reference does (include/fthmc_hip.h says so)."""
    g = np.random.default_rng(12)
    k = np.concatenate([g.integers(1, (1 << 53) + 1, 200000, dtype=np.uint64), ku([1, 2, 3, 1 << 52, (1 << 53) - 1, 1 << 53])])
    for lo, hi in ((0.0, 1.0), (-math.pi, math.pi), (1e6, 1e6 + 1), (-3.0, 3.0), (-1e-3, 7.0)):
        d = draws_dev(probe, k, k[::-1].copy(), lo, hi)
        assert np.array_equal(bits(d['p1']), bits(PR.uniform(k, lo, hi))), (lo, hi)
        assert np.array_equal(bits(d['p2']), bits(PR.uniform(k[::-1], lo, hi))), (lo, hi)
        assert d['p1'].min() >= lo and d['p1'].max() <= hi
        if (lo, hi) in ((0.0, 1.0), (-math.pi, math.pi)):
            assert d['p1'].max() < hi
    d = draws_dev(probe, ku([1, 2, 1 << 20]), ku([1, 1, 1]), 1e6, 1e6 + 1)
    assert d['p1'][0] == 1e6 + 1 and d['p1'][1] == 1e6 + 1 and d['p1'][2] < 1e6 + 1


def test_draws_from_random_words(probe):
    """2^20 random word blocks through every helper: u53 and the accept uniform exact, Box-Muller within the bound"""
    g = np.random.default_rng(13)
    n = 1 << 20
    k1 = g.integers(1, (1 << 53) + 1, n, dtype=np.uint64)
    k2 = g.integers(1, (1 << 53) + 1, n, dtype=np.uint64)
    k1[:4096] = g.integers(1, 1 << 20, 4096, dtype=np.uint64)                      # large radii
    k1[4096:8192] = np.uint64(1 << 53) - g.integers(0, 1 << 20, 4096, dtype=np.uint64)      # radii next to 0
    d = draws_dev(probe, k1, k2, low_bits=0x3a5)
    assert np.array_equal(d['u1'], k1.astype(np.float64) * U) and np.array_equal(d['u2'], k2.astype(np.float64) * U)
    assert np.array_equal(bits(d['acc']), bits(PR.accept_u(k1)))
    a, b, rad = PR.normal_pair_ld(k1, k2)
    ea, eb = bm_units(d['a'], a, rad), bm_units(d['b'], b, rad)
    i, j = int(np.argmax(ea)), int(np.argmax(eb))
    print(f'Box-Muller over 2^20 random words: max {max(ea[i], eb[j]):.3f} units of rad 2^-53 (bound {BM_BOUND})')
    assert ea[i] <= BM_BOUND and eb[j] <= BM_BOUND, (ea[i], int(k1[i]), int(k2[i]), eb[j], int(k1[j]), int(k2[j]))


# ----------------------------------------------------------------------------------------------------------- the C ABI: values
def _uniform_case(seeds, n, lo, hi):
    B = len(seeds)
    buf, out = guarded(B, n)
    got = ops.random_uniform(seeds.cuda(), (B, n), lo, hi, out=out)
    assert got.data_ptr() == out.data_ptr()
    dev = check_guard(buf, B, n, 'random_uniform')
    ref = PR.uniform(PR.uniform_bits(seeds.numpy(), n), lo, hi)
    bad = np.argwhere(bits(dev) != bits(ref))
    assert bad.size == 0, (n, lo, hi, len(bad), bad[0], dev[tuple(bad[0])], ref[tuple(bad[0])])
    assert dev.min() >= lo and dev.max() < hi


@pytest.mark.parametrize('n', NS)
def test_random_uniform_is_the_reference_bit_for_bit(n):
    """ops.random_uniform on (0, 1) and (-pi, pi) = the correctly rounded reference values of counter plane 2, every element
    written, nothing outside: odd tails, one grid's worth (16384 values) exactly, the grid-stride loop with and without a
    ragged end; seeds at the ends of both key words"""
    for lo, hi in ((0.0, 1.0), (-math.pi, math.pi)):
        _uniform_case(seed_set(), n, lo, hi)


@pytest.mark.parametrize('B', [1, 37, 300])
def test_random_uniform_over_many_chains(B):
    for n in (3, 513, 16385):
        _uniform_case(parallel.chain_seeds(1338, 5, 5 + B, 9), n, -math.pi, math.pi)


def _momenta_case(seeds, n):
    """-> the largest Box-Muller error of the case, in units of rad 2^-53"""
    B = len(seeds)
    bv, v = guarded(B, n)
    bu, u = guarded(B, 1)
    gv, gu = ops.random_momenta(seeds.cuda(), (B, n), out_v=v, out_u=u.view(B))
    assert gv.data_ptr() == v.data_ptr() and gu.data_ptr() == u.data_ptr()
    dv = check_guard(bv, B, n, 'random_momenta v')
    du = check_guard(bu, B, 1, 'random_momenta u')[:, 0]
    sn = seeds.numpy()
    uref = PR.accept_u(PR.accept_bits(sn))
    assert np.array_equal(bits(du), bits(uref)), (n, du, uref)
    ref, rad = PR.momenta_ld(sn, n)
    e = bm_units(dv, ref, rad)
    k = np.unravel_index(int(np.argmax(e)), e.shape)
    assert e[k] <= BM_BOUND, (n, k, e[k], dv[k], float(ref[k]))
    # without u: the same v, and no u
    bv2, v2 = guarded(B, n)
    _, none = ops.random_momenta(seeds.cuda(), (B, n), need_u=False, out_v=v2)
    assert none is None
    assert np.array_equal(bits(check_guard(bv2, B, n, 'random_momenta v (no u)')), bits(dv))
    return float(e[k])


@pytest.mark.parametrize('n', NS)
def test_momenta_through_the_c_abi(n):
    """ops.random_momenta: u = the reference's accept uniform (counter plane 1) bit for bit; every momentum within 12 units of
    rad 2^-53 of the reference's pair of counter (p, 0, 0, 0) -- the bound derived in the module docstring (11.2 of it
    accounted for) -- with pairs in (cos, sin) order, an odd n ending on a cos; every element written, nothing outside.

    Not yet measured on an MI355X (the test prints the maximum per n)."""
    e = _momenta_case(seed_set(), n)
    print(f'n = {n}: Box-Muller max {e:.3f} units of rad 2^-53 (bound {BM_BOUND})')


@pytest.mark.parametrize('B', [1, 37, 300])
def test_momenta_over_many_chains(B):
    e = max(_momenta_case(parallel.chain_seeds(1338, 5, 5 + B, 9), n) for n in (3, 513, 16385))
    print(f'B = {B}: Box-Muller max {e:.3f} units of rad 2^-53 (bound {BM_BOUND})')


# ----------------------------------------------------------------------------------------------------------- sharding and order
@pytest.mark.parametrize('n', [513, 2 * 64 * 64, 2 * 128 * 128])
def test_draws_do_not_depend_on_batch_order_or_capture(n):
    """a chain's draws are a function of its seed: any sub-batch and any order of the seeds give the same bits, and so does a
    call replayed from a captured graph"""
    B = 12
    seeds = parallel.chain_seeds(1362, 1000, 1000 + B, 17).cuda()
    v, u = ops.random_momenta(seeds, (B, n))
    xi = ops.random_uniform(seeds, (B, n), -math.pi, math.pi)
    for sl in (slice(0, 1), slice(5, 9), slice(B - 1, B), slice(3, B)):
        vs, us = ops.random_momenta(seeds[sl], (sl.stop - sl.start, n))
        assert torch.equal(vs, v[sl]) and torch.equal(us, u[sl])
        assert torch.equal(ops.random_uniform(seeds[sl], (sl.stop - sl.start, n), -math.pi, math.pi), xi[sl])
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(5)).cuda()
    vp, up = ops.random_momenta(seeds[perm], (B, n))
    assert torch.equal(vp, v[perm]) and torch.equal(up, u[perm])
    assert torch.equal(ops.random_uniform(seeds[perm], (B, n), -math.pi, math.pi), xi[perm])
    vg, ug, xg = torch.zeros_like(v), torch.zeros_like(u), torch.zeros_like(xi)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        g = torch.cuda.CUDAGraph()
        with capture(g, st):
            ops.random_momenta(seeds, (B, n), out_v=vg, out_u=ug)
            ops.random_uniform(seeds, (B, n), -math.pi, math.pi, out=xg)
        for t in (vg, ug, xg):
            t.zero_()
        g.replay()
        st.synchronize()
    torch.cuda.current_stream().wait_stream(st)
    assert torch.equal(vg, v) and torch.equal(ug, u) and torch.equal(xg, xi)
    del g


# ----------------------------------------------------------------------------------------------------------- chain seeds
@pytest.mark.parametrize('B', [255, 256, 257, 1000, 4096])
def test_device_chain_seeds_past_one_workgroup(B):
    """fthmc_chain_seeds = parallel.chain_seeds where the kernel's one workgroup of 256 threads loops over the chains, with
    chain ids and trajectories beyond 32 bits; with a device counter and advance, K launches -- eager, then K replays of one
    captured launch -- walk traj .. traj + K - 1 and leave the counter at K"""
    K = 4
    for seed, lo, traj in ((1331, (1 << 40) - 100, (1 << 33) - 2), (1362, 0, 0), (7, (1 << 40) + 12345, (1 << 33) + 5)):
        want = [parallel.chain_seeds(seed, lo, lo + B, traj + k) for k in range(K)]
        buf = torch.full((B + 2 * GUARD,), -1, dtype=torch.int64, device='cuda')
        out = buf[GUARD:GUARD + B]
        ops.chain_seeds(seed, lo, B, traj=traj, out=out)
        assert torch.equal(out.cpu(), want[0])
        counter = torch.zeros(1, dtype=torch.int64, device='cuda')
        for k in range(K):
            ops.chain_seeds(seed, lo, B, traj=traj, counter=counter, advance=True, out=out)
            assert torch.equal(out.cpu(), want[k]), k
        assert int(counter[0]) == K
        ops.chain_seeds(seed, lo, B, traj=traj, counter=counter, advance=False, out=out)      # reads, does not move
        assert int(counter[0]) == K and torch.equal(out.cpu(), parallel.chain_seeds(seed, lo, lo + B, traj + K))
        assert bool((buf[:GUARD] == -1).all()) and bool((buf[GUARD + B:] == -1).all())
    counter.zero_()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        g = torch.cuda.CUDAGraph()
        with capture(g, st):
            ops.chain_seeds(seed, lo, B, traj=traj, counter=counter, advance=True, out=out)
        for k in range(K):
            g.replay()
            st.synchronize()
            assert torch.equal(out.cpu(), want[k]), k
        assert int(counter[0]) == K
    torch.cuda.current_stream().wait_stream(st)
    del g


# ----------------------------------------------------------------------------------------------------------- the accept step
def _hmc(x, v, u):
    return ops.hmc_trajectory(x, v, u, 2.0, 0.15, 4)


def _flow(nl):
    return ops.pack_weights(R.default_flow(nl, torch.Generator().manual_seed(21)), device='cuda')


def _ft(nl):
    w = _flow(nl)
    return lambda x, v, u: ops.ft_trajectory(x, v, u, w, nl, 2.0, 0.15, 3, mode='md')


# every accept site: k_hmc_trajectory (one launch, L <= 64), k_metropolis behind the step kernels (the row-strip leapfrog at
# L = 64 with the VALU variant, which leaves the one-launch kernel aside), the small-lattice ftHMC kernel (flow_small.hip), and
# k_metropolis behind the tiled flow kernels at L = 8 (small path off) and L = 32; the third entry: the switches of the site
SITES = {'plain, one launch, L = 8': (8, lambda: _hmc, {}),
         'plain, row strips, L = 64': (64, lambda: _hmc, {'variant': 0}),
         'ftHMC, small-lattice path, L = 8': (8, lambda: _ft(2), {}),
         'ftHMC, small-lattice path off, L = 8': (8, lambda: _ft(2), {'small': False}),
         'ftHMC, tiled, L = 32': (32, lambda: _ft(2), {})}


@pytest.mark.parametrize('site', list(SITES))
def test_accept_step_at_the_ends_of_u(site):
    """acc = u < exp(-dH) at both ends of the accept uniform's range [0, 1 - 2^-53], and next to a chain whose dH is NaN:
      u = 0            accepts every chain whose dH is finite (exp(-dH) > 0 for dH < 745)
      u = 1 - 2^-53    rejects every chain with dH > 0 (exp(-dH) <= 1 - 2^-53 once dH >= 2^-53) and accepts dH <= 0
      a NaN among a chain's momenta makes its H0, H1 and dH NaN: rejected (u < NaN is false, as rand < exp(-nan) is in the
      reference), acc = 0 and x_new = x bit for bit, whatever u; the other chains of the batch keep the bits they have without it"""
    L, make, ctx = SITES[site]
    B = 4
    gen = torch.Generator().manual_seed(31 + L)
    x = ((torch.rand(B, 2, L, L, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi).cuda()
    v = torch.randn(B, 2, L, L, generator=gen, dtype=torch.float64).cuda()
    zero = torch.zeros(B, dtype=torch.float64, device='cuda')
    top = torch.full((B,), 1.0 - U, dtype=torch.float64, device='cuda')
    with switches(**ctx):
        run = make()
        lo = {k: t.clone() for k, t in run(x, v, zero).items() if k in ('x_new', 'dH', 'acc')}
        hi = {k: t.clone() for k, t in run(x, v, top).items() if k in ('x_new', 'dH', 'acc')}
        vp = v.clone()
        vp[1, 0, 2, 3] = float('nan')
        nan = {k: t.clone() for k, t in run(x, vp, zero).items() if k in ('x_new', 'dH', 'acc')}
    dH = lo['dH'].cpu()
    assert torch.isfinite(dH).all() and float(dH.abs().max()) < 700 and float(dH.abs().min()) > 1e-12, dH
    assert torch.equal(hi['dH'].cpu(), dH)
    assert bool((lo['acc'] == 1.0).all()), (lo['acc'], dH)
    assert not torch.equal(lo['x_new'], x)
    want = (dH <= 0).to(torch.float64)
    assert torch.equal(hi['acc'].cpu(), want), (hi['acc'], dH)
    assert float(want.sum()) < B, 'no chain with dH > 0: the rejecting end of the table was not exercised'
    sel = torch.where(want.cuda()[:, None, None, None] > 0.5, lo['x_new'], x)
    assert torch.equal(hi['x_new'], sel)
    # the poisoned chain
    assert float(nan['acc'][1]) == 0.0 and bool(torch.isnan(nan['dH'][1]))
    assert torch.equal(nan['x_new'][1], x[1])
    keep = [0, 2, 3]
    for k in ('x_new', 'dH', 'acc'):
        assert torch.equal(nan[k][keep], lo[k][keep]), k


# ----------------------------------------------------------------------------------------------------------- the loop's stride
def test_grid_stride_loop_does_each_pair_once():
    """A grid-stride loop whose stride is short of the grid (p += blockDim.x) still writes every element, with the right value:
    every workgroup then walks all the pairs behind its start, and no comparison of outputs can tell.  Only the work shows it.
    Two launches over the same 2^25 values, hence the same number of Philox blocks, logs and sincos:
      wide   65536 chains of n = 512: one workgroup per chain, one pair per thread, the loop body runs once
      long     256 chains of n = 131072: 32 workgroups per chain, 8 pairs per thread through the loop
    A correct loop does the same arithmetic in both; the short stride makes workgroup g of the long case walk 256 - g
    iterations instead of 8, 240.5 / 8 = 30 times the work.  Asked for: long <= 4 x wide (medians of interleaved event timings):
    room for a launch shape that suits the machine four times worse, an eighth of what the fault costs.  The ratio of the
    correct kernels has not been measured on an MI355X yet; the test prints it for both draws."""
    wide_B, wide_n, long_B, long_n = 65536, 512, 256, 131072
    assert wide_B * wide_n == long_B * long_n
    seeds = parallel.chain_seeds(1332, 0, wide_B, 3).cuda()
    out = torch.empty(wide_B * wide_n, dtype=torch.float64, device='cuda')
    times = {}
    for draw in ('momenta', 'uniform'):
        def launch(B, n):
            if draw == 'momenta':
                ops.random_momenta(seeds[:B], (B, n), need_u=False, out_v=out.view(B, n))
            else:
                ops.random_uniform(seeds[:B], (B, n), -math.pi, math.pi, out=out.view(B, n))
        t = {'wide': [], 'long': []}
        for rep in range(8):
            for name, B, n in (('wide', wide_B, wide_n), ('long', long_B, long_n)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch(B, n)
                e1.record()
                e1.synchronize()
                if rep >= 2:                                         # two warm-up rounds
                    t[name].append(e0.elapsed_time(e1))
        wide, long_ = float(np.median(t['wide'])), float(np.median(t['long']))
        times[draw] = (wide, long_)
        print(f'{draw}: wide {wide:.3f} ms, long {long_:.3f} ms, ratio {long_ / wide:.2f} (bound 4)')
    for draw, (wide, long_) in times.items():
        assert long_ <= 4 * wide, (draw, wide, long_)


# ---------------------------------------------------------------- seeds on the device
@pytest.mark.parametrize('seed,lo,B,traj', [(1331, 0, 128, 0), (7, 96, 32, 41), (2 ** 40 + 3, 1000, 5, 2 ** 33)])
def test_chain_seeds_on_the_device_equal_the_host_helper(seed, lo, B, traj):
    """fthmc_chain_seeds = parallel.chain_seeds (SplitMix64 of (seed, global chain id, trajectory)), also through a device
    counter that a captured launch advances."""
    from fthmc_amd import parallel
    want = parallel.chain_seeds(seed, lo, lo + B, traj)
    got = ops.chain_seeds(seed, lo, B, traj=traj, device='cuda')
    assert torch.equal(got.cpu(), want)
    counter = torch.tensor([traj], dtype=torch.int64, device='cuda')
    out = torch.empty(B, dtype=torch.int64, device='cuda')
    for k in range(3):
        ops.chain_seeds(seed, lo, B, counter=counter, advance=True, out=out)
        assert torch.equal(out.cpu(), parallel.chain_seeds(seed, lo, lo + B, traj + k)), k
    assert int(counter) == traj + 3
