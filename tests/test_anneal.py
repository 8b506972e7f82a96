"""CPU tests of annealed importance sampling (fthmc_anneal): the entry point is declared, exported and signed and
refuses what the header says it refuses before any launch; the host logic -- the schedules, the exact partition function, the
Jarzynski estimate and the effective sample size; the twin of tests/anneal_cases.py against a hand-written loop."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import anneal_cases as AC
import local_update_cases as LC


def test_entry_point_is_declared_exported_and_signed_and_stays_out_of_the_operator_table():
    from fthmc_amd import _lib, ops
    import fthmc_amd.torch_ops as TO
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'fthmc_hip.h')).read()
    declared = set(re.findall(r'\b(fthmc_[a-z0-9_]+)\s*\(', header))
    assert 'fthmc_anneal' in declared and hasattr(lib, 'fthmc_anneal') and 'fthmc_anneal' in _lib.SIGNATURES
    sig = _lib.SIGNATURES['fthmc_anneal']
    assert len(sig) == 16 and sig[9] is ctypes.c_int64 and sig[3] is ctypes.c_void_p and sig[4] is ctypes.c_int
    assert lib.fthmc_anneal.restype is ctypes.c_int
    assert callable(ops.anneal) and not any('anneal' in n for n in TO.__all__)
    import fthmc.anneal as A
    import fthmc_amd.anneal as A2
    assert A is A2 and callable(A.run_annealed) and callable(A.beta_schedule)


def test_every_refusal_returns_its_code_before_any_launch():
    """the argument checks come before anything touches the device: stand-in addresses are never read"""
    from fthmc_amd import _lib, ops
    from fthmc_amd._lib import FthmcError
    lib = _lib.load()
    X, S, O, W, Bt = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
    ARG = -1

    def call(x=X, B=2, L=8, betas=Bt, n_step=3, seeds=S, n_hb=1, n_or=0, nsweep=1, sweep0=0, path=1, work_in=None, out=O, work=W, trace=None):
        return lib.fthmc_anneal(x, B, L, betas, n_step, seeds, n_hb, n_or, nsweep, sweep0, path, work_in, out, work, trace, None)
    assert call(x=None) == ARG and call(out=None) == ARG and call(betas=None) == ARG and call(work=None) == ARG
    assert call(seeds=None) == ARG and call(seeds=None, n_hb=2, n_or=1) == ARG
    for B in (0, -1, 4194304):
        assert call(B=B) == ARG
    for L in (0, 2, 6, 10, -8, 32768):
        assert call(L=L) == ARG
    for kw in (dict(n_step=-1), dict(n_hb=-1), dict(n_or=-1), dict(nsweep=-1), dict(sweep0=-1), dict(sweep0=-2 ** 63)):
        assert call(**kw) == ARG, kw
    assert call(n_hb=0, n_or=0) == ARG and call(n_hb=0, n_or=0, seeds=None, n_step=1) == ARG
    assert call(n_step=65537) == ARG and call(n_step=2 ** 31 - 1) == ARG
    for p in (-1, 3, 255):
        assert call(path=p) == ARG
    assert call(path=1, L=68) == ARG and call(path=1, L=128) == ARG
    # the heatbath-sweep index is one 32-bit word: sweep0 + n_step nsweep n_hb <= 2^32, whatever the factors
    assert call(sweep0=2 ** 32 - 2) == ARG and call(sweep0=2 ** 32 + 1, n_step=0) == ARG and call(sweep0=2 ** 62) == ARG
    assert call(n_step=65536, nsweep=65536, n_hb=2) == ARG and call(n_step=65536, nsweep=2 ** 31 - 1, n_hb=2 ** 31 - 1) == ARG
    assert call(n_step=2, nsweep=2 ** 31 - 1, n_hb=2) == ARG and call(sweep0=2 ** 63 - 1, n_step=1) == ARG
    assert call(x=None, path=7, L=68) == ARG
    x = torch.zeros(2, 2, 8, 8, dtype=torch.float64)
    with pytest.raises(FthmcError):
        ops.anneal(x, [0.0, 1.0], None, n_hb=0, n_or=1)                  # a CPU tensor: there is no CPU fallback


def test_beta_schedule_endpoints_and_monotonicity():
    from fthmc_amd.anneal import beta_schedule
    for kind in ('quadratic', 'linear'):
        for b0, b1, n in ((0.0, 6.0, 2048), (0.0, 6.0, 1), (1.5, 0.25, 7), (0.1, 0.1 + 1e-9, 1000), (2.0, 2.0, 5)):
            b = beta_schedule(b0, b1, n, kind)
            assert b.dtype == np.float64 and b.shape == (n + 1,) and b[0] == b0 and b[-1] == b1
            d = np.diff(b)
            assert np.all(d >= 0) if b1 >= b0 else np.all(d <= 0)
            assert np.all(np.isfinite(b)) and b.min() >= 0
    q, l = beta_schedule(0.0, 6.0, 4), beta_schedule(0.0, 6.0, 4, 'linear')
    assert np.array_equal(q, [0.0, 0.375, 1.5, 3.375, 6.0]) and np.array_equal(l, [0.0, 1.5, 3.0, 4.5, 6.0])
    assert np.all(np.diff(q, 2) > 0)                                     # small steps first
    assert np.array_equal(beta_schedule(2.0, 2.0, 0), [2.0])
    for bad in ((0.0, 6.0, -1, 'quadratic'), (0.0, 6.0, 4, 'cubic'), (-1.0, 6.0, 4, 'linear'), (0.0, math.inf, 4, 'linear'),
                (0.0, math.nan, 4, 'linear'), (0.0, 6.0, 0, 'linear')):
        with pytest.raises(ValueError):
            beta_schedule(*bad)


def _log_z_by_quadrature(beta, N):
    """log of int prod dx / 2 pi exp(beta sum cos P) over the 8 links of the 2 x 2 torus (4 plaquettes) by the periodic trapezoid rule
    on N points per link, in np.longdouble"""
    LD = np.longdouble
    a = (2 * LD(math.pi) / N) * np.arange(N, dtype=LD)
    g = np.meshgrid(*([a] * 6), indexing='ij', sparse=True)              # x0[0][1], x0[1][0], x0[1][1], x1[0][1], x1[1][0], x1[1][1]
    tot = LD(0)
    for x000 in a:
        for x100 in a:
            x0 = {(0, 0): x000, (0, 1): g[0], (1, 0): g[1], (1, 1): g[2]}
            x1 = {(0, 0): x100, (0, 1): g[3], (1, 0): g[4], (1, 1): g[5]}
            s = 0
            for i in range(2):
                for j in range(2):
                    s = s + np.cos(x0[i, j] + x1[(i + 1) % 2, j] - x0[i, (j + 1) % 2] - x1[i, j])
            tot += np.exp(LD(beta) * s).sum()
    return float(np.log(tot) - 8 * np.log(LD(N)))


def test_exact_log_partition_against_quadrature_and_the_loop_formula():
    from fthmc_amd.utils import observables as O
    # With exp(beta cos P) = sum_n I_n e^{i n P}, a link shared by two plaquettes forces their n to be equal when it is integrated
    # exactly, and equal MODULO N under the trapezoid rule on N points (which integrates e^{i m x} to 1 for every m = 0 mod N).  On the
    # 2 x 2 torus every plaquette shares links with the others, so the rule gives sum over (n_1 .. n_4) all congruent modulo N of
    # I_n1 I_n2 I_n3 I_n4 = sum_r (sum_m I_{r + m N})^4 instead of Z = sum_n I_n^4.  The excess is known, so the quadrature
    # checks the formula to the rounding of the two; it is below 1e-7 of Z at beta = 0.7, N = 8 (8 I_0^3 I_8 + 8 I_1^3 I_7 lead)
    beta, N = 0.7, 8
    In = {n: _bessel(abs(n), beta) for n in range(-4 * N, 4 * N + 1)}
    Z = sum(In[n] ** 4 for n in range(-3 * N, 3 * N + 1))
    Zq = sum(sum(In[r + m * N] for m in range(-3, 4)) ** 4 for r in range(N))
    got, want = O.exact_log_partition(beta, 2), _log_z_by_quadrature(beta, N)
    print(f'log Z(2 x 2, beta = {beta}): formula {got:.12f}, quadrature {want:.12f}, difference {want - got:.3e}, the rule\'s excess '
          f'{math.log(Zq / Z):.3e}')
    assert 0 < math.log(Zq / Z) < 1e-7
    assert abs((want - got) - math.log(Zq / Z)) < 1e-13
    assert abs(got - math.log(float(np.i0(beta) ** 4) * (1 + 2 * sum((_bessel(n, beta) / float(np.i0(beta))) ** 4 for n in range(1, 12))))) < 1e-13
    # against the denominator of exact_loop_of_area, sum_n (I_n / I_0)^V, with V log I_0 put back
    for beta, L in ((6.0, 16), (2.0, 8), (0.5, 4), (7.0, 64)):
        V, nmax = L * L, 40
        l = O._log_bessel_ratios(beta, nmax)
        den = np.exp(V * l[np.abs(np.arange(-nmax, nmax + 1))]).sum()
        want = V * math.log(float(np.i0(beta))) + float(np.log(den))
        assert abs(O.exact_log_partition(beta, L) - want) <= 4e-15 * V * (1 + abs(math.log(float(np.i0(beta))))) + 1e-13, (beta, L)
        # the loop of area 0 is 1: the same denominator, as exact_loop_of_area forms it
        assert abs(O.exact_loop_of_area(beta, V, 0) - 1.0) < 1e-15
    assert abs(O.exact_log_partition(6.0, 16) - 1077.30) < 5e-3           # the figure of the design note
    assert O.exact_log_partition(0.0, 16) == 0.0


def _bessel(n, beta):
    """I_n(beta) by its power series (small beta)"""
    return sum((beta / 2) ** (2 * k + n) / (math.factorial(k) * math.factorial(k + n)) for k in range(40))


def test_jarzynski_log_mean_and_work_ess_on_constructed_weights():
    from fthmc_amd.utils import observables as O
    # equal work: the mean is exact, the error 0, every chain counts
    v, e = O.jarzynski_log_mean(np.full(64, -1077.25))
    assert abs(v - 1077.25) < 1e-12 and e < 1e-12 and abs(O.work_ess(np.full(64, -1077.25)) - 64) < 1e-9
    # one chain carries everything: log mean = -W_min - log n, ESS 1
    w = np.full(32, 50.0); w[5] = -100.0
    v, e = O.jarzynski_log_mean(w)
    assert abs(v - (100.0 - math.log(32))) < 1e-12 and abs(O.work_ess(w) - 1.0) < 1e-12 and math.isfinite(e)
    # two values, half and half: weights 1 and 1/3 -> mean 2/3, ESS = n (4/3)^2 / (2 (1 + 1/9)) = 0.8 n; huge offsets cancel
    for off in (0.0, -5000.0, 5000.0):
        w = np.where(np.arange(48) % 2 == 0, 0.0, math.log(3.0)) + off
        v, e = O.jarzynski_log_mean(w, 16)
        assert abs(v - (math.log(2.0 / 3.0) - off)) < 1e-11 and abs(O.work_ess(w) - 0.8 * 48) < 1e-9
    w = np.where(np.arange(48) % 2 == 0, 0.0, math.log(3.0))
    v, e = O.jarzynski_log_mean(w, 16)
    # blocks of 3 hold the weights (1, 1/3, 1) or (1/3, 1, 1/3): delete-one means (32 - 7/3) / 45 and (32 - 5/3) / 45
    jk = np.log(np.array([(32 - 7 / 3) / 45, (32 - 5 / 3) / 45] * 8))
    assert abs(e - math.sqrt(15 * np.mean((jk - jk.mean()) ** 2))) < 1e-14
    # the jackknife error of a log-normal sample agrees with the spread of independent repetitions
    rng = np.random.default_rng(3)
    est = np.array([O.jarzynski_log_mean(rng.normal(0.0, 0.5, 4096), 16) for _ in range(64)])
    assert abs(est[:, 0].mean() - 0.125) < 4 * est[:, 0].std() / 8           # log E exp(-W) = sigma^2 / 2
    assert 0.6 < est[:, 1].mean() / est[:, 0].std() < 1.6
    assert math.isnan(O.jarzynski_log_mean([1.0])[1]) and O.jarzynski_log_mean([1.0])[0] == -1.0
    with pytest.raises(ValueError):
        O.jarzynski_log_mean([])


def test_twin_run_of_two_steps_equals_a_hand_written_loop():
    L, betas = 4, (0.0, 0.75, 3.0)
    x, seeds, w0 = AC.fields(L)
    r = AC.run(x, betas, seeds, n_hb=1, n_or=1, nsweep=1, sweep0=AC.SWEEP0, work_in=w0)
    # by hand
    LD = np.longdouble
    C0 = LC.action_sum(x)
    y1 = LC.sweep(x, betas[1], seeds, AC.SWEEP0, n_or=1, dt=LD)
    C1 = LC.action_sum(y1)
    y2 = LC.sweep(y1, betas[2], seeds, AC.SWEEP0 + 1, n_or=1, dt=LD)
    C2 = LC.action_sum(y2)
    W = w0.astype(LD) + (LD(betas[0]) - LD(betas[1])) * C0 + (LD(betas[1]) - LD(betas[2])) * C1
    assert np.array_equal(r['x'], y2) and np.array_equal(r['fields'][1], y1) and np.array_equal(r['fields'][0], x)
    assert r['trace'].shape == (AC.B, 3) and r['dtrace'].shape == (AC.B, 3)
    for k, C in enumerate((C0, C1, C2)):
        assert np.all(np.abs((r['trace'][:, k] - C).astype(np.float64)) < 1e-16 * L * L)      # two orders of one longdouble sum
    assert np.all(np.abs((r['work'] - W).astype(np.float64)) < 1e-15)
    assert not np.array_equal(y1, x) and not np.array_equal(y2, y1) and np.all(np.abs(C1 - C0) > 1e-3)
    # the bound is derived for fp64 arithmetic: the same steps in float64 land inside it, and it is small
    C64 = [AC.IC.sums(f, np.float64)[0] for f in r['fields']]
    W64 = w0.copy()
    for k in range(2):
        W64 = W64 + (betas[k] - betas[k + 1]) * C64[k]
    assert np.all(np.abs((W64 - r['work']).astype(np.float64)) <= r['work_bound']) and np.all(r['work_bound'] < 1e-12)
    assert np.all(np.abs((np.stack(C64, 1) - r['trace']).astype(np.float64)) <= r['dtrace'])
    # a cut twin run is the run
    a = AC.run(x, betas[:2], seeds, n_hb=1, n_or=1, sweep0=AC.SWEEP0, work_in=w0)
    b = AC.run(a['x'], betas[1:], seeds, n_hb=1, n_or=1, sweep0=AC.SWEEP0 + 1, work_in=a['work'])
    assert np.array_equal(b['x'], r['x']) and np.all(np.abs((b['work'] - r['work']).astype(np.float64)) < 1e-15)


def test_cases_cover_the_shapes_and_counts():
    cs = AC.cases()
    assert {L for L, _ in cs} == {4, 8, 12, 64, 68} and {c for L, c in cs if L < 64} == set(AC.COUNTS)
    assert len([c for L, c in cs if L >= 64]) == 2
    d = np.diff(AC.BETAS)
    assert (d == 0).any() and (d < 0).any() and (d > 0).any() and len(AC.BETAS) == AC.N_STEP + 1
    assert [AC.lu_threads(L) for L in AC.SHAPES] == [64, 64, 128, 1024, 1024]
    assert len(set(AC.fields(8)[1].tolist())) == AC.B
