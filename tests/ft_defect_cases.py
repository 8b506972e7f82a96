"""The torch float64 twin of boundary-condition tempering through the flow and the cases the CPU and GPU tests share.

S(x) = -beta C(y) + (beta - g_b) Dsum(y) - log det J(x), y = F(x): the flow and the periodic action are oracle.ref_cpu's (flow_forward,
action), Dsum is the same cosines under tests/defect_cases.mask, the couplings and the defects are defect_cases' (couplings, defect_of),
and the force is autograd's.  The trajectory is meta_cases.schedule's stages with that force, regularize at the end, accept by
u < exp(-dH).

Nothing in S has a kink, so the one thing that cannot be compared to round-off is the accept: the twin keeps |u - exp(-dH)| per chain,
and a chain is LEFT OUT below U_MARGIN exp(-dH).  On the committed seeds no chain is (tests/test_ft_defect.py asserts it with the twin
alone): a test that left chains out could hide a failure."""
import functools

import numpy as np
import torch

import defect_cases as DC
import ft_meta_cases as FC
import meta_cases as MC
from oracle import ref_cpu as R

U_MARGIN = MC.U_MARGIN
DT = MC.DT
GEN_ARCH = FC.GEN_ARCH


def dsum(y, defect):
    """the cosines of the defect's plaquettes, R.action's order of the four links"""
    m = torch.from_numpy(DC.mask(y.shape[-1], defect))
    return (torch.cos(R._plaq_action_order(y)) * m).sum(dim=(1, 2))


def action(x, flow, beta, g, defect, act='silu'):
    """-> (S, logdet, C, Dsum, Q), differentiable in x; g: the couplings per chain (a tensor [B])"""
    y, logdet = R.flow_forward(x, flow, act)
    sw = R.action(y, beta)
    d = dsum(y, defect)
    return sw + (beta - g) * d - logdet, logdet, sw / (-beta), d, R.charge(y)


def force(x, flow, beta, g, defect, act='silu'):
    """dS / dx by autograd"""
    xg = x.detach().clone().requires_grad_(True)
    (gr,) = torch.autograd.grad(action(xg, flow, beta, g, defect, act)[0].sum(), xg)
    return gr


def hamiltonian(x, v, flow, beta, g, defect, act='silu'):
    with torch.no_grad():
        S, _, _, d, Q = action(x, flow, beta, g, defect, act)
        y = R.flow_forward(x, flow, act)[0]
        return S + 0.5 * (v * v).flatten(1).sum(1), d, R.plaq_mean(y, beta), Q


def trajectory(x, v, u, flow, beta, g, defect, dt_md, nstep, integrator, act='silu'):
    """One flowed trajectory of every chain under the defect -> dict of numpy arrays (x_new, dH, acc, H0, H1, plaq, Q, dsum, u_margin,
    left_out); plaq, Q, dsum: of F(x_new)"""
    b0, stages = MC.schedule(integrator, float(dt_md), int(nstep))
    g = torch.as_tensor(np.asarray(g, dtype=np.float64))
    h0, d0, pl0, Q0 = hamiltonian(x, v, flow, beta, g, defect, act)
    y = x + b0 * v
    p = v.clone()
    ye = y
    for kind, a, b in stages:
        F = force(ye, flow, beta, g, defect, act)
        if kind == 'shift':
            ye = y - a * F
        else:
            p = p - a * F
            y = y + b * p
            ye = y
    y = R.regularize(y)
    h1, d1, pl1, Q1 = hamiltonian(y, p, flow, beta, g, defect, act)
    dH = (h1 - h0).numpy()
    e = np.exp(-dH)
    uu = np.asarray(u, dtype=np.float64)
    acc = uu < e
    u_margin = np.abs(uu - e)
    pick = lambda new, old: np.where(acc, new.numpy(), old.numpy())
    return {'x_new': np.where(acc[:, None, None, None], y.numpy(), x.numpy()), 'dH': dH, 'acc': acc, 'H0': h0.numpy(), 'H1': h1.numpy(),
            'plaq': pick(pl1, pl0), 'Q': pick(Q1, Q0), 'dsum': pick(d1, d0), 'u_margin': u_margin, 'left_out': u_margin < U_MARGIN * e}


# ---------------------------------------------------------------- the cases
# ft_meta_cases.PATHS' shapes (B, L, n_layers): the smallest at which each path can go wrong
PATHS = FC.PATHS
DEFECTS = DC.DEFECTS
AMPS, BETAS, NSTEPS, INTEGRATORS, SCALES = MC.AMPS, MC.BETAS, MC.NSTEPS, MC.INTEGRATORS, FC.SCALES


def _cases():
    """every shape of every path with every defect; amplitude, beta, nstep, integrator and the flow's steepness rotate so that each
    value meets each path and each defect; the couplings are mixed out of {0, beta / 3, beta}, the mix rotating with the defect"""
    out = []
    for dk in DEFECTS:
        k = DEFECTS.index(dk)                                            # start the rotation elsewhere for every defect
        for path, shapes in PATHS:
            for B, L, nl in shapes:
                out.append((path, B, L, nl, AMPS[k % 2], BETAS[(k // 2) % 2], NSTEPS[(k // 4) % 2], INTEGRATORS[k % 3], dk, SCALES[(k // 3) % 2]))
                k += 1
    return tuple(out)


CASES = _cases()          # (path, B, L, n_layers, amp, beta, nstep, integrator, defect kind, weight scale)
SEED_SHIFT = {}           # case id -> shift of the seed, where the first seed left a chain out (none needed)


def case_id(c):
    path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
    return f'{path}-B{B}-L{L}-n{nl}-a{amp:.1f}-b{beta:g}-s{nstep}-{integ}-{dk}-w{sc:g}'


def case_seed(c):
    path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
    return 7000 + 97 * L + 13 * B + 5 * DEFECTS.index(dk) + 1000 * [p for p, _ in PATHS].index(path) + SEED_SHIFT.get(case_id(c), 0)


flow_of = FC.flow_of


def inputs(c):
    """-> (x, v, u, g [B] numpy, defect, flow)"""
    path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
    seed = case_seed(c)
    x = torch.from_numpy(MC.links(B, L, seed, amp))
    v, u = MC.draws(B, L, seed + 1)
    return x, torch.from_numpy(v), u, DC.couplings(B, beta, DEFECTS.index(dk)), DC.defect_of(dk, L), flow_of(path, nl, sc)


@functools.lru_cache(maxsize=None)
def case(c):
    """-> (x, v, u, g, defect, flow, the twin's trajectory) of case c; computed once and shared (treat as read-only)"""
    path, B, L, nl, amp, beta, nstep, integ, dk, sc = c
    x, v, u, g, df, flow = inputs(c)
    return x, v, u, g, df, flow, trajectory(x, v, u, flow, beta, g, df, DT, nstep, integ)
