"""The MD integrators on the CPU oracle: what tests/test_integrators.py and tests/test_integrators_gpu.py hold the library to.

The schedules are written out here a second time, independently of csrc/integrator.h (stage by stage, as the tables of the
papers give them, not in the library's periodic form): an initial drift x += b0 v and then stages, g = the gradient of the action,
    ('kick', a, b):   v -= a g(x*);  x += b v        x* = x, or the shifted field if a 'shift' stage came just before
    ('shift', c, 0):  x~ = x - c g(x)                the next stage evaluates g at x~; x and v are untouched
  leapfrog          b0 = dt/2;       nstep x kick(dt, dt), the last b = dt/2
  omelyan           2nd-order minimum norm, position version (Omelyan, Mryglod & Folk 2003), lambda = 0.1931833275037836:
                    b0 = lambda dt; per step kick(dt/2, (1 - 2 lambda) dt), kick(dt/2, 2 lambda dt); the very last b = lambda dt
  force_gradient    4th order, B A B_FG A B (Kennedy, Clark & Silva 2009) with the end kicks of neighbouring steps merged and the
                    force-gradient term as one shifted re-evaluation of the force (Yin & Mawhinney 2011):
                    b0 = 0; kick(dt/6, dt/2); per step shift(dt^2/24), kick(2dt/3, dt/2); between steps kick(dt/3, dt/2);
                    last kick(dt/6, 0)
The forces and actions are the oracle's (oracle/ref_cpu.py: autograd of the reference's action)."""
import math

import torch

from oracle import ref_cpu as R

LAMBDA = 0.1931833275037836
NAMES = ('leapfrog', 'omelyan', 'force_gradient')
CODES = {'leapfrog': 0, 'omelyan': 1, 'force_gradient': 2}


def forces(name, nstep):
    return {'leapfrog': nstep, 'omelyan': 2 * nstep, 'force_gradient': 3 * nstep + 1}[name]


def schedule(name, dt, nstep):
    """-> (b0, [(kind, a, b), ...])"""
    assert nstep >= 1
    if name == 'leapfrog':
        st = [('kick', dt, dt) for _ in range(nstep)]
        st[-1] = ('kick', dt, 0.5 * dt)
        return 0.5 * dt, st
    if name == 'omelyan':
        st = []
        for _ in range(nstep):
            st += [('kick', 0.5 * dt, (1.0 - 2.0 * LAMBDA) * dt), ('kick', 0.5 * dt, 2.0 * LAMBDA * dt)]
        st[-1] = ('kick', 0.5 * dt, LAMBDA * dt)
        return LAMBDA * dt, st
    if name == 'force_gradient':
        st = [('kick', dt / 6.0, 0.5 * dt)]
        for k in range(nstep):
            st += [('shift', dt * dt / 24.0, 0.0), ('kick', 2.0 * dt / 3.0, 0.5 * dt)]
            st.append(('kick', dt / 3.0, 0.5 * dt) if k + 1 < nstep else ('kick', dt / 6.0, 0.0))
        return 0.0, st
    raise ValueError(name)


def md(x, v, grad_fn, name, dt, nstep):
    """the MD of `name`: -> (x', v'); grad_fn(y) = the gradient of the action at y.  The arithmetic of R.leapfrog, stage by stage."""
    b0, stages = schedule(name, dt, nstep)
    x_ = x + b0 * v
    v_ = v
    at = x_
    for kind, a, b in stages:
        g = grad_fn(at)
        if kind == 'shift':
            at = x_ + (-a) * g
        else:
            v_ = v_ + (-a) * g
            x_ = x_ + b * v_
            at = x_
    return x_, v_


def plain_md(x, p, beta, name, dt, nstep):
    return md(x, p, lambda y: R.wilson_force(y, beta), name, dt, nstep)


def ft_md(x, v, flow, beta, name, dt, nstep, act='silu'):
    return md(x, v, lambda y: R.ft_force(y, flow, beta, act), name, dt, nstep)


def plain_hmc(x, v, u, beta, name, dt, nstep):
    """R.hmc (per chain) with the MD of `name` -> dict(dH, acc, newx, H0, H1)"""
    red = lambda t: t.flatten(1).sum(1)
    h0 = R.action(x, beta) + 0.5 * red(v * v)
    x_, v_ = plain_md(x, v, beta, name, dt, nstep)
    xr = R.regularize(x_)
    h1 = R.action(xr, beta) + 0.5 * red(v_ * v_)
    dH = h1 - h0
    acc = u < torch.exp(-dH)
    return {'dH': dH, 'acc': acc, 'newx': torch.where(acc[:, None, None, None], xr, x), 'H0': h0, 'H1': h1}


def ft_hmc(x, v, u, flow, beta, name, dt, nstep, act='silu'):
    """R.ft_hmc (mode 'md', per chain) with the MD of `name` -> dict(dH, acc, newx, H0, H1, plaq, Q, md_x, md_v)"""
    red = lambda t: t.flatten(1).sum(1)
    with torch.no_grad():
        h0 = R.ft_action(x, flow, beta, act) + 0.5 * red(v * v)
    x_, v_ = ft_md(x, v, flow, beta, name, dt, nstep, act)
    xr = R.regularize(x_)
    with torch.no_grad():
        h1 = R.ft_action(xr, flow, beta, act) + 0.5 * red(v_ * v_)
        dH = h1 - h0
        acc = u < torch.exp(-dH)
        newx = torch.where(acc[:, None, None, None], xr, x)
        y = R.flow_forward(newx, flow, act)[0]
        plaq, Q = R.plaq_mean(y, beta), R.charge(y)
    return {'dH': dH, 'acc': acc, 'newx': newx, 'H0': h0, 'H1': h1, 'plaq': plaq, 'Q': Q, 'md_x': x_, 'md_v': v_}


def accept_margin(res, u):
    """min over the chains of |u - exp(-dH)|: how far every accept decision is from flipping"""
    return float((u - torch.exp(-res['dH'])).abs().min())


def draw(seed, B, L):
    """seeded inputs of the GPU cases: uniform links in +-pi, normal momenta, accept uniforms"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, 2, L, L, generator=g, dtype=torch.float64) * 2 - 1) * math.pi
    v = torch.randn(B, 2, L, L, generator=g, dtype=torch.float64)
    u = torch.rand(B, generator=g, dtype=torch.float64)
    return x, v, u


def decided_case(seed, B, L, run, margin=1e-3, redraws=3):
    """Inputs whose accept decisions are decided on the oracle's numbers: |u - exp(-dH)| > margin for every chain.  If the draw of
    `seed` is not, the seed is redrawn by a fixed rule (seed + 1000, at most `redraws` times).  run(x, v, u) -> the oracle's result
    dict.  -> (seed used, x, v, u, result)"""
    for k in range(redraws + 1):
        s = seed + 1000 * k
        x, v, u = draw(s, B, L)
        res = run(x, v, u)
        if accept_margin(res, u) > margin:
            return s, x, v, u, res
    raise AssertionError(f'seed {seed}: no draw with every accept decided by more than {margin} in {redraws} redraws')
