"""CPU: the hard cases of tests/first_order_cases.py are fit to be held to 1e-9 per tensor and per chain, the oracle's two orders
agree with each other on them, and the oracle agrees with the reference itself on one of them.

Every case asserts the condition second_order_cases.py states, for the first-order quantities: the oracle at the inputs and at a
copy with every link and weight moved by one relative 2^-52 (three sets of signs) differ by at most 1e-12 on every parameter tensor
(training and one-layer weight gradients) and on every chain (force, one-layer link gradient, leapfrog step, the flowed links,
S_eff, log det, log q, log p, log J); pytest -s prints each case's figure and the spread of its tensors.
tests/golden/first_order_steep_L8.npz is the L = 8, 8-layer, scale-3 case from the reference itself
(tests/golden/make_golden_first_order_steep.py), on the inputs of second_order_steep_L8.npz, so that the hard cases do not rest on
the oracle alone."""
import os

import numpy as np
import pytest
import torch

import first_order_cases as FC
import second_order_cases as C
from conftest import ROOT, load_golden
from oracle import ref_cpu as R


@pytest.mark.parametrize('case', FC.CASES, ids=FC.IDS)
def test_reference_is_well_conditioned_at_the_case(case):
    inp, ref = FC.inputs(case), FC.oracle(case)
    errs = FC.sensitivity(inp, ref, 8000 + 10 * FC.CASES.index(case))
    name, e = FC.worst(errs)
    spread = FC.tensor_spread(ref['gw'])
    print(f'{case.name}: sensitivity {e:.1e} ({name}), smallest / largest tensor {spread:.1e}')
    assert all(torch.isfinite(ref[k]).all() for k in ('F', 'y', 'lf_x', 'lf_v', 'S_eff', 'logdet', 'logq', 'logp'))
    # every quantity the GPU file compares is among the entries held
    B, nl = case.B, case.nl
    assert len(errs) == 12 * nl + 9 * B + 2 * nl * B, len(errs)
    FC.hold(errs, FC.SENS_BOUND, case.name)
    # the inputs are the hard ones: links on the cut in chain 0, and the per-tensor measure is not the global one
    assert float(inp.x[0, 0, 0, 0]) == np.pi - 1e-9 and float(inp.x[0, 1, 0, 0]) == -np.pi + 1e-9
    assert spread < 0.5, spread


def test_cases_cover_what_they_are_for():
    """the cases of the second order with their inputs, and every lattice kind of the tuned first-order kernels: the smallest,
    ragged below and above the fast-wrap threshold, whole tiles with a ragged edge, every (mu, off) on exact tiles with a run-time
    activation, 16 tiles per chain; no case above 2 * 32^2 sites but L = 64 with one chain; inputs never modified"""
    assert FC.CASES[:len(C.CASES)] == C.CASES and all(FC.inputs(c) is C.inputs(c) for c in C.CASES)
    by_L = {c.L: c for c in FC.FIRST_ONLY}
    assert set(by_L) == {4, 20, 28, 36, 40, 64, 32}
    assert by_L[32].nl == 8 and by_L[32].act == 'relu' and by_L[4].nl == 8
    assert all(c.B * c.L ** 2 <= 2 * 32 ** 2 or (c.L, c.B) == (64, 1) for c in FC.CASES)
    assert all(c.arch is None and not c.tanh for c in FC.FIRST_ONLY)
    assert {c.act for c in FC.FIRST_ONLY} == {'silu', 'relu', 'leaky_relu'}
    assert len({c.name for c in FC.CASES}) == len(FC.CASES)
    c = FC.BY_NAME['L20_silu']
    assert FC.inputs(c) is FC.inputs(c) and FC.oracle(c) is FC.oracle(c)
    assert FC.inputs(FC.BY_NAME['L8_tanh']).act == 'silu+tanh'


@pytest.mark.parametrize('case', FC.CASES, ids=FC.IDS)
def test_training_gradient_is_the_action_vjp(case):
    """the two orders tied together: log q - log p = S_eff + a constant in the weights, so the oracle's training gradient (the mean
    over the chains) is its action VJP `aw` (second_order_cases.oracle_results) with gS = 1 / B and glogdet = 0"""
    inp = FC.inputs(case)
    B = case.B
    a = C.oracle_results(inp._replace(gS=torch.full((B,), 1.0 / B, dtype=torch.float64), glogdet=torch.zeros(B, dtype=torch.float64)))
    errs = FC.per_tensor(a['aw'], FC.oracle(case)['gw'], 'aw vs train gw')
    print(f'{case.name}: action VJP against the training gradient: worst %.1e (%s)' % FC.worst(errs)[::-1])
    FC.hold(errs, FC.SENS_BOUND, case.name)
    # ... and the force of the one is the force of the other
    FC.hold(FC.per_chain(a['F'], FC.oracle(case)['F'], 'F'), FC.SENS_BOUND, case.name)


def test_oracle_reproduces_the_steep_fixture():
    """the oracle against the reference's own ft_force, ft_action and train_step at the hard case, per tensor and per chain, at
    the conditioning bound of the cases: two fp64 implementations of the same graph"""
    path = os.path.join(ROOT, 'tests', 'golden', 'first_order_steep_L8.npz')
    assert os.path.getsize(path) < 512 * 1024
    g, inp, ref = FC.steep_fixture()
    assert (int(g['n_layers']), g['x'].shape, float(g['beta']), str(g['act'])) == (8, (2, 2, 8, 8), FC.BETA, 'silu')
    assert np.all(g['x'][0, 0, 0, :] == np.pi - 1e-9) and np.all(g['x'][0, 1, :, 0] == -np.pi + 1e-9)
    # the parameters are the scaled ones: three times the default init's range 1 / sqrt(fan_in)
    assert 2.0 / np.sqrt(18) < np.abs(g['w0_0']).max() <= 3.0 / np.sqrt(18)
    # the inputs are those of the second-order fixture, bit for bit: one hard case from the reference serves both orders
    g2 = load_golden('second_order_steep_L8')
    assert all(np.array_equal(g[k], g2[k]) for k in ['x'] + [f'w{li}_{pi}' for li in range(8) for pi in range(6)])
    t64 = lambda a: torch.as_tensor(a, dtype=torch.float64)
    FC.hold(FC.per_chain(t64(g['F']), t64(g2['F']), 'F, create_graph off / on'), FC.SENS_BOUND, 'the two fixtures')
    assert np.array_equal(g['S_eff'], g2['S_eff'])
    full = FC.oracle_results(inp)
    errs = FC.compare({k: full[k] for k in ref}, ref, inp.flow)
    assert len(errs) == 48 + 4 * 2
    name, e = FC.worst(errs)
    print(f'oracle vs the reference fixture: worst {e:.1e} ({name}); smallest / largest tensor {FC.tensor_spread(ref["gw"]):.1e}')
    FC.hold(errs, FC.SENS_BOUND, 'steep fixture')
    # loss_dkl is the mean of log q - log p, as recorded and in the oracle
    dkl = float(g['loss_dkl'])
    assert abs(float(R.calc_dkl(full['logp'], full['logq'])) - dkl) <= FC.SENS_BOUND * abs(dkl)
    assert abs(float((ref['logq'] - ref['logp']).mean()) - dkl) <= FC.SENS_BOUND * abs(dkl)
    # ... and the fixture's inputs meet the condition of the cases
    sens = FC.sensitivity(inp, full, 8900)
    print('steep fixture: sensitivity %.1e (%s)' % FC.worst(sens)[::-1])
    FC.hold(sens, FC.SENS_BOUND, 'steep fixture, conditioning')
    assert FC.tensor_spread(ref['gw']) < 0.5
