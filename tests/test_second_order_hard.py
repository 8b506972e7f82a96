"""CPU: the hard cases of tests/second_order_cases.py are fit to be held to 1e-9 per tensor, and the oracle agrees with the
reference's own autograd on one of them.

Every case asserts the condition second_order_cases.py states: the oracle's double backward at the inputs and at a copy with every
link and weight moved by one relative 2^-52 (three sets of signs) differ by at most 1e-12 on every parameter tensor and every
chain (pytest -s prints each case's figure and the spread of its tensors).  tests/golden/second_order_steep_L8.npz is the L = 8, 8-layer, scale-3 case
from the reference itself (tests/golden/make_golden_second_order.py), so that the hard cases do not rest on the oracle alone."""
import os

import numpy as np
import pytest
import torch

import second_order_cases as C
from conftest import ROOT


@pytest.mark.parametrize('case', C.CASES, ids=[c.name for c in C.CASES])
def test_reference_is_well_conditioned_at_the_case(case):
    inp, ref = C.inputs(case), C.oracle(case)
    errs = C.sensitivity(inp, ref, 7000 + 10 * C.CASES.index(case))
    name, e = C.worst(errs)
    spread = min(C.tensor_spread(ref[k]) for k in ('gw_force', 'gw_vjp', 'aw'))
    print(f'{case.name}: sensitivity {e:.1e} ({name}), smallest / largest tensor {spread:.1e}')
    assert all(torch.isfinite(t).all() for k in ('F', 'Hg', 'ax') for t in [ref[k]])
    C.hold(errs, C.SENS_BOUND, case.name)
    # the inputs are the hard ones: links on the cut in chain 0, and the per-tensor measure is not the global one (the smallest
    # tensor is well below the largest)
    assert float(inp.x[0, 0, 0, 0]) == np.pi - 1e-9 and float(inp.x[0, 1, 0, 0]) == -np.pi + 1e-9
    assert spread < 0.2, spread


def test_cases_cover_what_they_are_for():
    """every (mu, off) at L = 16, every activation, every lattice kind, no case above 2 * 32^2 sites, inputs never modified"""
    assert {c.act for c in C.CASES} == {'silu', 'relu', 'leaky_relu'}
    assert {c.L for c in C.CASES} >= {8, 12, 16, 24, 32} and all(c.B * c.L ** 2 <= 2 * 32 ** 2 for c in C.CASES)
    assert all(c.nl == 8 for c in C.CASES if c.L == 16) and C.BY_NAME['L8_silu'].nl == 8
    assert any(c.arch is not None for c in C.CASES) and any(c.tanh for c in C.CASES)
    a, b = C.inputs(C.CASES[0]), C.inputs(C.CASES[0])
    assert a is b and C.oracle(C.CASES[0]) is C.oracle(C.CASES[0])


def test_oracle_reproduces_the_steep_fixture():
    """the oracle's double backward against the reference's own autograd at the hard case, per tensor and per chain, at the
    conditioning bound of the cases: two fp64 implementations of the same graph"""
    path = os.path.join(ROOT, 'tests', 'golden', 'second_order_steep_L8.npz')
    assert os.path.getsize(path) < 512 * 1024
    g, inp, ref = C.steep_fixture()
    assert (int(g['n_layers']), g['x'].shape, float(g['beta'])) == (8, (2, 2, 8, 8), C.BETA)
    assert np.all(g['x'][0, 0, 0, :] == np.pi - 1e-9) and np.all(g['x'][0, 1, :, 0] == -np.pi + 1e-9)
    # the parameters are the scaled ones: three times the default init's range 1 / sqrt(fan_in)
    assert 2.0 / np.sqrt(18) < np.abs(g['w0_0']).max() <= 3.0 / np.sqrt(18)
    errs = C.compare(C.oracle_results(inp), ref, inp.flow)
    name, e = C.worst(errs)
    print(f'oracle vs the reference fixture: worst {e:.1e} ({name}); smallest / largest tensor {C.tensor_spread(ref["gw_force"]):.1e}')
    C.hold(errs, C.SENS_BOUND, 'steep fixture')
    # ... and the fixture's inputs meet the condition of the cases
    sens = C.sensitivity(inp, C.oracle_results(inp), 7900)
    print('steep fixture: sensitivity %.1e (%s)' % C.worst(sens)[::-1])
    C.hold(sens, C.SENS_BOUND, 'steep fixture, conditioning')
