"""The torch float64 twin of metadynamics ftHMC and the cases the CPU and GPU tests share.

S_b(x) = -beta sum cos P(y) - log det J(x) + V(Q_m(y)), y = F(x): the flow and the unbiased action are oracle.ref_cpu's
(flow_forward, action), V is written as a differentiable torch expression of Q_m = sum sin P(y) / 2 pi -- which interval of the
table (or which wall) a chain sits on is decided on the detached Q_m with tests/meta_cases.Table's rule, inside V = V_i + f dV is
differentiable through f, on the wall the quadratic form -- and the force is autograd's.  The trajectory is
meta_cases.schedule's stages with that force, regularize at the end, accept by u < exp(-dH).

V' jumps at the nodes and at +-qmax, so the twin records for every force evaluation and energy of a chain min |t - round(t)| of the
lookup coordinate and the distance to +-qmax, and for the accept |u - exp(-dH)|.  A chain is LEFT OUT below T_MARGIN on the former
or below U_MARGIN exp(-dH) on the latter; on the committed seeds no chain is (tests/test_ft_meta.py asserts it with the twin alone)."""
import functools
import math

import numpy as np
import torch

import meta_cases as MC
from oracle import ref_cpu as R

T_MARGIN = MC.T_MARGIN
U_MARGIN = MC.U_MARGIN
DT = MC.DT
TWO_PI = 2.0 * math.pi
GEN_ARCH = ((4, 6, 5), 5, 3)        # hidden sizes, kernel size, mixture components of the generic-net case


def charge_m(y):
    return torch.sin(R.plaq(y)).flatten(1).sum(1) / TWO_PI


def bias(q, tab):
    """V(q) per chain as a differentiable expression of q [B] -> (V, margin): the interval / wall side from the detached q"""
    qd = q.detach().numpy()
    B = len(qd)
    r = tab.rows(B)
    inside, i, _, t, delta = tab.locate(qd, np.float64)
    V = torch.from_numpy(tab.V)
    rt, it = torch.from_numpy(r), torch.from_numpy(i)
    v0, v1 = V[rt, it], V[rt, torch.clamp(it + 1, max=tab.nb - 1)]
    f = (q + tab.qmax) / float(delta) - torch.from_numpy(np.floor(t))
    inner = v0 + f * (v1 - v0)
    d = q.abs() - tab.qmax
    edge = torch.where(torch.from_numpy(qd < 0), V[rt, 0], V[rt, -1])
    outer = edge + ((0.5 * tab.wall) * d) * d
    ins = torch.from_numpy(inside)
    margin = np.minimum(np.where(inside, np.abs(t - np.rint(t)), np.inf), np.abs(np.abs(qd) - tab.qmax))
    return torch.where(ins, inner, outer), margin


def biased_action(x, flow, beta, tab, act='silu'):
    """-> (S_b, logdet, Q_m, V, margin), differentiable in x"""
    y, logdet = R.flow_forward(x, flow, act)
    qm = charge_m(y)
    vb, margin = bias(qm, tab)
    return R.action(y, beta) - logdet + vb, logdet, qm, vb, margin


def force(x, flow, beta, tab, act='silu'):
    """dS_b / dx by autograd -> (F, margin)"""
    xg = x.detach().clone().requires_grad_(True)
    S, _, _, _, margin = biased_action(xg, flow, beta, tab, act)
    (g,) = torch.autograd.grad(S.sum(), xg)
    return g, margin


def hamiltonian(x, v, flow, beta, tab, act='silu'):
    with torch.no_grad():
        S, _, qm, vb, margin = biased_action(x, flow, beta, tab, act)
        y = R.flow_forward(x, flow, act)[0]
        return S + 0.5 * (v * v).flatten(1).sum(1), qm, vb, margin, R.plaq_mean(y, beta), R.charge(y)


def trajectory(x, v, u, flow, beta, dt_md, nstep, integrator, tab, act='silu'):
    """One biased flowed trajectory of every chain -> dict of numpy arrays (x_new, dH, acc, H0, H1, plaq, Q, qm, vbias, t_margin,
    u_margin, left_out); plaq, Q, qm, vbias: of F(x_new)"""
    b0, stages = MC.schedule(integrator, float(dt_md), int(nstep))
    h0, qm0, vb0, margin, pl0, Q0 = hamiltonian(x, v, flow, beta, tab, act)
    y = x + b0 * v
    p = v.clone()
    ye = y
    for kind, a, b in stages:
        F, m = force(ye, flow, beta, tab, act)
        margin = np.minimum(margin, m)
        if kind == 'shift':
            ye = y - a * F
        else:
            p = p - a * F
            y = y + b * p
            ye = y
    y = R.regularize(y)
    h1, qm1, vb1, m, pl1, Q1 = hamiltonian(y, p, flow, beta, tab, act)
    margin = np.minimum(margin, m)
    dH = (h1 - h0).numpy()
    e = np.exp(-dH)
    uu = np.asarray(u, dtype=np.float64)
    acc = uu < e
    u_margin = np.abs(uu - e)
    left_out = (margin < T_MARGIN) | (u_margin < U_MARGIN * e)
    pick = lambda new, old: np.where(acc, new.numpy(), old.numpy())
    return {'x_new': np.where(acc[:, None, None, None], y.numpy(), x.numpy()), 'dH': dH, 'acc': acc, 'H0': h0.numpy(), 'H1': h1.numpy(),
            'plaq': pick(pl1, pl0), 'Q': pick(Q1, Q0), 'qm': pick(qm1, qm0), 'vbias': pick(vb1, vb0), 't_margin': margin,
            'u_margin': u_margin, 'left_out': left_out}


# ---------------------------------------------------------------- the cases
# (B, L, n_layers, path): the smallest shape at which each code path can go wrong
ONE_LAUNCH = ((3, 8, 2), (2, 12, 3), (4, 16, 4))
SMALL_OFF = ((3, 8, 2), (4, 16, 4))
TILED = ((2, 20, 2), (2, 32, 2), (2, 64, 2))
VALU = ((2, 16, 2),)
GENERIC = ((2, 8, 2),)
NO_LAYERS = ((2, 8, 0),)
PATHS = (('one', ONE_LAUNCH), ('off', SMALL_OFF), ('tiled', TILED), ('valu', VALU), ('gen', GENERIC), ('nolayers', NO_LAYERS))
AMPS, BETAS, NSTEPS, INTEGRATORS, TABLES, SCALES = MC.AMPS, MC.BETAS, MC.NSTEPS, MC.INTEGRATORS, ('zero', 'quad', 'rough'), (1.0, 3.0)


def _cases():
    """every shape of every path with every table and both row layouts; amplitude, beta, nstep, integrator and the flow's steepness
    rotate so that each value meets each path and each table"""
    out = []
    for tk in TABLES:
        k = 0
        for path, shapes in PATHS:
            for B, L, nl in shapes:
                for G in (1, B):
                    out.append((path, B, L, nl, AMPS[k % 2], BETAS[(k // 2) % 2], NSTEPS[(k // 4) % 2], INTEGRATORS[k % 3], tk, G,
                                SCALES[(k // 3) % 2]))
                    k += 1
    return tuple(out)


CASES = _cases()          # (path, B, L, n_layers, amp, beta, nstep, integrator, table kind, G, weight scale)
SEED_SHIFT = {}           # case id -> shift of the seed, where the first seed left a chain out (none needed)


def case_id(c):
    path, B, L, nl, amp, beta, nstep, integ, tk, G, sc = c
    return f'{path}-B{B}-L{L}-n{nl}-a{amp:.1f}-b{beta:g}-s{nstep}-{integ}-{tk}-G{G}-w{sc:g}'


def case_seed(c):
    path, B, L, nl, amp, beta, nstep, integ, tk, G, sc = c
    return 9000 + 97 * L + 13 * B + 5 * TABLES.index(tk) + (G > 1) + 1000 * [p for p, _ in PATHS].index(path) + SEED_SHIFT.get(case_id(c), 0)


@functools.lru_cache(maxsize=None)
def flow_of(path, nl, scale, seed=11):
    """the case's flow as oracle.ref_cpu takes it (a list of weight tuples), default init times `scale`"""
    gen = torch.Generator().manual_seed(seed + nl)
    if path == 'gen':
        hidden, k, n_mix = GEN_ARCH
        flow = R.default_flow(nl, gen, hidden=hidden, n_mix=n_mix, k=k)
    else:
        flow = R.default_flow(nl, gen)
    return [tuple(w * scale for w in layer) for layer in flow]


def inputs(c):
    path, B, L, nl, amp, beta, nstep, integ, tk, G, sc = c
    seed = case_seed(c)
    x = torch.from_numpy(MC.links(B, L, seed, amp))
    v, u = MC.draws(B, L, seed + 1)
    return x, torch.from_numpy(v), u, MC.table(tk, G), flow_of(path, nl, sc)


@functools.lru_cache(maxsize=None)
def case(c):
    """-> (x, v, u, table, flow, the twin's trajectory) of case c; computed once and shared (treat as read-only)"""
    path, B, L, nl, amp, beta, nstep, integ, tk, G, sc = c
    x, v, u, tab, flow = inputs(c)
    return x, v, u, tab, flow, trajectory(x, v, u, flow, beta, DT, nstep, integ, tab)
