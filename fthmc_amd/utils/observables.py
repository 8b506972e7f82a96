"""Host-side analysis of sampling histories: topological-charge tunnelling versus MD-time lag and the
topological susceptibility; the exact finite-volume Wilson loops of 2D U(1), Creutz ratios and the
blocked mean of a history of loop tables (`exact_wilson_loop`, `string_tension_exact`, `creutz_ratios`, `loop_table`:
beyond the reference, which measures no loops); the exact finite-volume distribution of the topological charge
(`exact_charge_distribution`, `exact_charge_moment`).  numpy only; the histories come from
`FieldTransformation.run` / `run_hmc` (lists or arrays of per-trajectory charges, optionally per chain).

Reference: ipynb/ft_hmc.py:16-53 (`average`, `sigma`, `sub_avg`, `block_list`, `change_sqr`, `change_sqr_vs_dt`),
:168-176 (`save_topo_change_sqr`); hmc_2dU1.py:661 (susceptibility 1.23 +- 0.02 at L=8, beta=2).  Pinned to the
outputs of those reference functions on seeded charge histories (tests/golden/observables.npz, written by
tests/golden/make_golden.py section 10 and compared in the CPU test suite)."""
from typing import Optional, Sequence

import numpy as np

from .distributions import bootstrap

N_BLOCK = 16          # blocks used for the error of a mean (the reference's `n_block`)


def block_means(v: np.ndarray, n_block: int = N_BLOCK) -> np.ndarray:
    """Means of `n_block` equal blocks of `v` along axis 0; a remainder is dropped from the FRONT (the
    oldest samples), a series shorter than `n_block` falls back to blocks of one."""
    v = np.asarray(v, dtype=np.float64)
    n = v.shape[0]
    if n == 0:
        return v[:0]
    size = n // n_block
    if size < 1:
        size, n_block = 1, n
    start = n - n_block * size
    return v[start:].reshape(n_block, size, *v.shape[1:]).mean(axis=1)


def sub_avg(v) -> np.ndarray:
    """v - mean(v) (ipynb/ft_hmc.py:25-27)."""
    v = np.asarray(v, dtype=np.float64)
    return v - v.mean(axis=0)


def sigma(v, reference_literal: bool = False) -> float:
    """Error of the mean of `v`.  The standard error sqrt(var / (n - 1)) (var = population variance); with
    `reference_literal` what ipynb/ft_hmc.py:20-23 returns: var / sqrt(n - 1), a variance where a standard
    deviation is meant (pinned by tests/golden/observables.npz)."""
    v = np.asarray(v, dtype=np.float64)
    if len(v) < 2:
        return float('nan')
    var = float(np.mean((v - v.mean()) ** 2))
    return var / np.sqrt(len(v) - 1) if reference_literal else float(np.sqrt(var / (len(v) - 1)))


def change_sqr(q: np.ndarray, lag: int, n_block: int = N_BLOCK, reference_literal: bool = False):
    """<(Q(t + lag) - Q(t))^2> over the history (axis 0 = trajectory; further axes = chains, averaged) and the
    error of that mean from `n_block` block means -> (mean, sigma).  ipynb/ft_hmc.py:42-50; `reference_literal`
    selects the reference's error formula (see `sigma`)."""
    q = np.asarray(q, dtype=np.float64)
    if lag < 1 or q.shape[0] <= lag:
        return float('nan'), float('nan')
    d2 = (q[lag:] - q[:-lag]) ** 2
    if d2.ndim > 1:
        d2 = d2.reshape(d2.shape[0], -1).mean(axis=1)
    bm = block_means(d2, n_block)
    return float(bm.mean()), sigma(bm, reference_literal)


def change_sqr_vs_dt(q: np.ndarray, dt_range: int = 10, n_block: int = N_BLOCK, reference_literal: bool = False):
    """[[lag, mean, sigma], ...] for lag = 1..dt_range: how fast the topological charge decorrelates in units
    of trajectories (the figure of merit of arXiv:2112.01586; ipynb/ft_hmc.py:52-53)."""
    return [[lag, *change_sqr(q, lag, n_block, reference_literal)] for lag in range(1, dt_range + 1)]


def topological_susceptibility(q: np.ndarray, volume: int, nboot: int = 100, binsize: int = 16):
    """chi_Q = (<Q^2> - <Q>^2) / V with a binned-bootstrap error -> (chi, err)."""
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    q2_mean, q2_err = bootstrap(q ** 2, nboot=nboot, binsize=binsize)
    chi = (q2_mean - q.mean() ** 2) / volume
    return float(chi), float(q2_err / volume)


def save_topo_change_sqr(fn: str, q_history: Sequence, drop_len: Optional[int] = None, dt_range: int = 10,
                         reference_literal: bool = False):
    """Write `lag mean sigma` lines for the history with its first `drop_len` entries (default: a third,
    `len // 3`, ipynb/ft_hmc.py:168-176) dropped as thermalisation."""
    q = np.asarray(q_history, dtype=np.float64)
    rows = change_sqr_vs_dt(q[len(q) // 3 if drop_len is None else drop_len:], dt_range,
                            reference_literal=reference_literal)
    with open(fn, 'w') as f:
        for lag, mean, sig in rows:
            f.write(f'{lag} {mean} {sig}\n')
    return rows


# ---------------------------------------------------------------- Wilson loops: the exact solution and the analysis of a history
def _log_bessel_ratios(beta: float, nmax: int) -> np.ndarray:
    """l[n] = log(I_n(beta) / I_0(beta)), n = 0 .. nmax, from the ratios r_n = I_{n+1} / I_n = 1 / (2 (n + 1) / beta + r_{n+1})
    run DOWNWARD from r_N = 0 far beyond nmax (the recurrence contracts in that direction: every step keeps the relative
    error at a few ulps).  Logarithms, so that I_n^V of V = 4096 neither overflows nor underflows."""
    beta = float(beta)
    if not beta > 0.0:
        raise ValueError(f'beta > 0 expected, got {beta}')
    N = nmax + 64 + int(2 * beta)
    r = np.zeros(N + 1, dtype=np.longdouble)
    b = np.longdouble(beta)
    for n in range(N - 1, -1, -1):
        r[n] = 1 / (2 * np.longdouble(n + 1) / b + r[n + 1])
    l = np.zeros(nmax + 1, dtype=np.longdouble)
    l[1:] = np.cumsum(np.log(r[:nmax]))
    return l


def exact_wilson_loop(beta: float, L: int, R: int, T: int, nmax: int = 40) -> float:
    """<W(R, T)> of 2D U(1) with the Wilson action on the periodic L x L lattice (V = L^2 plaquettes), for a non-self-intersecting
    R x T rectangle of area A = R T (character expansion; the sum over n runs over the topological sectors):
        sum_n I_n(beta)^(V - A) I_{n+1}(beta)^A / sum_n I_n(beta)^V .
    A = 1 is the plaquette; the formula is symmetric under A <-> V - A; T = L makes it the Polyakov-loop correlator at distance R;
    W(L, L) = 1.  Evaluated in logarithms relative to I_0 (log-sum-exp in extended precision): beta = 6, V = 4096, A = V / 2 gives
    its 1e-82 to 1e-10 relative."""
    if not (1 <= R <= L and 1 <= T <= L):
        raise ValueError(f'1 <= R, T <= L = {L} expected, got {R}, {T}')
    return exact_loop_of_area(beta, int(L) * int(L), int(R) * int(T), nmax)


def exact_loop_of_area(beta: float, V: int, A: int, nmax: int = 40) -> float:
    """The formula of `exact_wilson_loop` as a function of the enclosed area A, 0 <= A <= V, alone (what it depends on)."""
    if not 0 <= A <= V:
        raise ValueError(f'0 <= A <= V = {V} expected, got {A}')
    l = _log_bessel_ratios(beta, nmax + 1)
    n = np.arange(-nmax, nmax + 1)
    ln, ln1 = l[np.abs(n)], l[np.abs(n + 1)]                     # I_{-n} = I_n
    num = (V - A) * ln + A * ln1
    den = V * ln
    m = max(num.max(), den.max())
    return float(np.exp(num - m).sum() / np.exp(den - m).sum())


def exact_defect_plaquette(beta: float, L: int, c: float, Ld: int, on_defect: bool = True, nmax: int = 40) -> float:
    """<cos P> of one plaquette of 2D U(1) on the periodic L x L lattice whose Ld plaquettes of a defect carry the coupling c beta in
    place of beta (boundary-condition tempering), on the defect or off it.  The plaquettes still decouple sector by sector,
        Z = sum_n I_n(beta)^(V - Ld) I_n(c beta)^Ld = sum_n w_n,      <cos P> = sum_n w_n I_n'(y) / I_n(y) / sum_n w_n,
    y = c beta on the defect and beta off it, I_n'(y) / I_n(y) = I_{n+1}(y) / I_n(y) + n / y (n >= 0; I_{-n} = I_n).  At c = 0 only
    n = 0 is left on an open line: 0 on the defect, I_1(beta) / I_0(beta) off it.  c = 1 or Ld = 0 is `exact_wilson_loop(beta, L, 1, 1)`.
    Logarithms relative to I_0 in extended precision, as there."""
    beta, c, V, Ld = float(beta), float(c), int(L) * int(L), int(Ld)
    if not (0.0 <= c <= 1.0 and 0 <= Ld <= V):
        raise ValueError(f'0 <= c <= 1 and 0 <= Ld <= V = {V} expected, got {c}, {Ld}')
    if on_defect and Ld == 0:
        raise ValueError('on_defect: the defect has no plaquette (Ld = 0)')
    LD = np.longdouble
    n = np.abs(np.arange(-nmax, nmax + 1))
    lb = _log_bessel_ratios(beta, nmax + 1)
    open_line = c == 0.0 and Ld > 0                                          # I_n(0) = 0 for n != 0
    if open_line and on_defect:
        return 0.0
    ly = lb if (not on_defect or c == 1.0) else _log_bessel_ratios(c * beta, nmax + 1)
    y = LD(beta) if not on_defect else LD(c) * LD(beta)
    ratio = np.exp(ly[n + 1] - ly[n]) + n.astype(LD) / y                       # I_n'(y) / I_n(y)
    if open_line:
        return float(ratio[nmax])                                            # the sector n = 0 alone
    lc = lb if (c == 1.0 or Ld == 0) else _log_bessel_ratios(c * beta, nmax + 1)
    logw = (V - Ld) * lb[n] + Ld * lc[n]
    w = np.exp(logw - logw.max())
    return float((w * ratio).sum() / w.sum())


def string_tension_exact(beta: float) -> float:
    """sigma = -log(I_1(beta) / I_0(beta)): W(R, T) = exp(-sigma R T) in infinite volume, an exact area law."""
    return float(-_log_bessel_ratios(beta, 1)[1])


def creutz_ratios(W) -> np.ndarray:
    """chi(R, T) = -log[ W(R, T) W(R - 1, T - 1) / (W(R, T - 1) W(R - 1, T)) ] for R, T >= 2 from a table W[..., R - 1, T - 1]
    -> [..., Rmax - 1, Tmax - 1] (entry [R - 2, T - 2]); an exact area law gives the string tension everywhere.  NaN where the
    argument of the logarithm is not positive (a noisy large loop)."""
    W = np.asarray(W, dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return -np.log(W[..., 1:, 1:] * W[..., :-1, :-1] / (W[..., 1:, :-1] * W[..., :-1, 1:]))


def loop_table(samples, n_block: int = N_BLOCK):
    """(mean, error) of a history of loop tables `samples` [n, ..., Rmax, Tmax] (axis 0 = trajectory, e.g. history['wloops'];
    axes between it and the table = chains, averaged): the error of the mean from `n_block` block means, as `change_sqr`."""
    v = np.asarray([np.asarray(getattr(t, 'cpu', lambda: t)()) for t in samples], dtype=np.float64) if isinstance(samples, (list, tuple)) \
        else np.asarray(samples, dtype=np.float64)
    if v.ndim < 3:
        raise ValueError(f'loop_table: [n, ..., Rmax, Tmax] expected, got {v.shape}')
    if v.ndim > 3:
        v = v.reshape(v.shape[0], -1, *v.shape[-2:]).mean(axis=1)
    bm = block_means(v, n_block)
    nb = bm.shape[0]
    err = np.sqrt(bm.var(axis=0) / (nb - 1)) if nb > 1 else np.full(bm.shape[1:], np.nan)
    return bm.mean(axis=0), err


# ---------------------------------------------------------------- the topological charge: its exact finite-volume distribution
def exact_charge_distribution(beta: float, L: int, qmax: int, nmax: int = 12, nodes: int = 200) -> np.ndarray:
    """P(Q), Q = -qmax .. qmax, of the geometric charge Q = sum wrap(P) / 2 pi of 2D U(1) with the Wilson action on the periodic
    L x L lattice (V = L^2 plaquettes) -> [2 qmax + 1] float64.  With a theta term the plaquettes decouple sector by sector,
        Z(theta) = sum_n c_n(theta)^V,     c_n(theta) = int_{-pi}^{pi} dP / 2 pi  e^{beta cos P} cos((theta / 2 pi - n) P),
    and P(Q) = int_0^{2 pi} d theta / 2 pi  e^{-i theta Q} Z(theta) / Z(0).  c_n by Gauss-Legendre (`nodes` points: the integrand is
    entire), n = -nmax .. nmax (c_n / c_0 falls like e^{-beta} / (pi n I_0(beta)), taken to the power V), theta by the periodic
    trapezoid rule on N = max(4 qmax + 4, 256) points (Z is 2 pi-periodic and even: spectrally accurate; the charges the rule
    aliases onto |Q| <= qmax lie beyond 3 qmax).  V log|c_n| with the common maximum taken out: V = 4096 neither overflows nor
    underflows.  The caller chooses qmax wide enough for its purpose: the sum of the result is 1 minus the tail beyond qmax
    (L = 64, beta = 6 needs qmax >= 30 for 1e-10; exact_charge_moment chooses its own)."""
    beta, V, qmax = float(beta), int(L) * int(L), int(qmax)
    if not beta > 0.0 or V < 1 or qmax < 0:
        raise ValueError(f'beta > 0, L >= 1 and qmax >= 0 expected, got {beta}, {L}, {qmax}')
    LD = np.longdouble
    g, wg = np.polynomial.legendre.leggauss(int(nodes))
    P = (LD(np.pi) * g.astype(LD))                                       # nodes on (-pi, pi); the weights carry pi / 2 pi = 1 / 2
    wP = (wg.astype(LD) * LD(0.5)) * np.exp(LD(beta) * (np.cos(P) - 1))  # e^{-beta} taken out of every c_n: cancels in Z / Z(0)
    N = max(4 * qmax + 4, 256)
    a = (np.arange(N, dtype=LD) / N)[:, None] - np.arange(-nmax, nmax + 1, dtype=LD)[None, :]      # theta / 2 pi - n
    c = (np.cos(a[:, :, None] * P[None, None, :]) * wP).sum(axis=2)
    logc = V * np.log(np.abs(c))
    sign = np.where((c < 0) & (V % 2 == 1), LD(-1), LD(1))
    m = logc.max()
    Z = (sign * np.exp(logc - m)).sum(axis=1)
    ratio = Z / Z[0]
    Q = np.arange(-qmax, qmax + 1)
    k = np.arange(N)
    ph = (np.outer(Q, k) % N).astype(LD) * (2 * LD(np.pi) / N)           # the phase reduced in integers first
    return ((np.cos(ph) * ratio[None, :]).sum(axis=1) / N).astype(np.float64)


def exact_charge_moment(beta: float, L: int, power: int = 2) -> float:
    """<Q^power> of `exact_charge_distribution`, over a range of charges wide enough that the tail beyond it is below 1e-15
    (eight standard deviations of the wider of the large-beta form V / 4 pi^2 beta and the beta = 0 limit V / 12)."""
    V = int(L) * int(L)
    sig2 = V * min(1.0 / 12.0, 1.5 / (4 * np.pi ** 2 * float(beta)))
    qmax = int(8 * np.sqrt(sig2)) + 6
    p = exact_charge_distribution(beta, L, qmax)
    Q = np.arange(-qmax, qmax + 1, dtype=np.float64)
    return float((Q ** int(power) * p).sum())


# ---------------------------------------------------------------- annealed importance sampling: the exact partition function, the work
def exact_log_partition(beta: float, L: int, nmax: int = 40) -> float:
    """log Z(beta) of 2D U(1) with the Wilson action on the periodic L x L lattice in the measure prod dx / 2 pi (Z(0) = 1):
        Z = int prod dx / 2 pi  exp(beta sum cos P) = sum_n I_n(beta)^V,      log Z = V log I_0 + log sum_n (I_n / I_0)^V,
    the denominator of `exact_loop_of_area` with its common factor put back.  log I_0 from the generating function at its maximum,
    e^beta = I_0 + 2 sum_{n >= 1} I_n, with the ratios of `_log_bessel_ratios`: extended precision throughout (V log I_0 is 1077.30
    at L = 16, beta = 6).  What <exp(-W)> of an annealing run from beta = 0 estimates (anneal.run_annealed)."""
    beta, V = float(beta), int(L) * int(L)
    if beta == 0.0:
        return 0.0
    N = nmax + 64 + int(2 * beta) + int(12 * np.sqrt(beta))                # I_n / I_0 ~ exp(-n^2 / 2 beta) beyond n ~ beta: < e^-70 at N
    l = _log_bessel_ratios(beta, N)
    log_i0 = np.longdouble(beta) - np.log1p(2 * np.exp(l[1:]).sum())
    n = np.arange(-nmax, nmax + 1)
    return float(V * log_i0 + np.log(np.exp(V * l[np.abs(n)]).sum()))      # l <= 0: the largest term is 1


def jarzynski_log_mean(work, n_block: int = N_BLOCK):
    """log < exp(-W) > over the chains of an annealing run -> (value, delete-one-block jackknife error): the estimate of
    log Z(beta_1) / Z(beta_0) (Jarzynski's equality).  The smallest work is taken out before exponentiating; the chains are dealt
    into `n_block` blocks (at most one per chain) as `reweighted_mean` deals its units."""
    w = np.asarray(work, dtype=np.float64).reshape(-1)
    if w.size == 0:
        raise ValueError('jarzynski_log_mean: no work values')
    w0 = w.min()
    e = np.exp(-(w - w0))
    nb = max(1, min(int(n_block), e.size))
    parts = np.array_split(e, nb)
    sums, cnts = np.array([c.sum() for c in parts]), np.array([c.size for c in parts], dtype=np.float64)
    val = float(np.log(sums.sum() / cnts.sum()) - w0)
    if nb < 2:
        return val, float('nan')
    rest = np.array([np.delete(sums, i).sum() for i in range(nb)])         # added, not subtracted: one block may carry all the weight
    jk = np.log(rest / (cnts.sum() - cnts))
    return val, float(np.sqrt((nb - 1) * np.mean((jk - jk.mean()) ** 2)))


def work_ess(work) -> float:
    """The effective sample size (sum w)^2 / sum w^2 of the weights w = exp(-W): between 1 and the number of chains."""
    w = np.asarray(work, dtype=np.float64).reshape(-1)
    e = np.exp(-(w - w.min()))
    return float(e.sum() ** 2 / (e * e).sum())


def reweighted_mean(values, vbias, n_block: int = N_BLOCK):
    """Unbiased mean of an observable sampled under a frozen metadynamics bias (meta.run_meta):
        <O> = sum O e^{V} / sum e^{V},      V = `vbias`, the bias potential at each sample's Q_m
    -> (mean, jackknife error).  values, vbias: arrays of one shape, [samples] or [trajectories, chains].  The common maximum of
    vbias is subtracted before exponentiating (it cancels in the ratio).  The independent units -- the chains of a 2-D history
    (every chain's weighted sums over its trajectories), the samples of a 1-D one -- are dealt into `n_block` blocks (at most one
    per unit) and the error is that of the delete-one-block jackknife of the ratio."""
    o, vb = np.asarray(values, dtype=np.float64), np.asarray(vbias, dtype=np.float64)
    if o.shape != vb.shape or o.ndim not in (1, 2) or o.size == 0:
        raise ValueError(f'reweighted_mean: values and vbias of one shape, [samples] or [trajectories, chains], expected; got {o.shape}, {vb.shape}')
    wgt = np.exp(vb - vb.max())
    num, den = wgt * o, wgt
    if o.ndim == 2:
        num, den = num.sum(axis=0), den.sum(axis=0)
    nb = max(1, min(int(n_block), num.size))
    nums = np.array([c.sum() for c in np.array_split(num, nb)])
    dens = np.array([c.sum() for c in np.array_split(den, nb)])
    mean = float(nums.sum() / dens.sum())
    if nb < 2:
        return mean, float('nan')
    jk = (nums.sum() - nums) / (dens.sum() - dens)
    return mean, float(np.sqrt((nb - 1) * np.mean((jk - jk.mean()) ** 2)))
