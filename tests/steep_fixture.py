"""Readers of tests/golden/steep_inverse.npz (tests/golden/make_golden_steep.py) shared by test_steep_reference.py and
test_steep_inverse_gpu.py: numpy only, nothing here computes an expectation."""
import math
import os

import numpy as np

from conftest import GOLDEN

S0 = (2.0, 5.0, 10.0, 20.0)
TOL = 1e-13
ULP_PI = math.ulp(math.pi)


def load():
    return dict(np.load(os.path.join(GOLDEN, 'steep_inverse.npz'), allow_pickle=False))


def wrapdiff(a, b):
    return (np.asarray(a) - np.asarray(b) + math.pi) % (2 * math.pi) - math.pi


def active_mask(L, mu, off):
    """[L, L] bool: mu = 0 columns j % 4 == off, mu = 1 rows i % 4 == off (layers.py:213-292)"""
    sel = (np.arange(L) - off) % 4 == 0
    return np.broadcast_to(sel[None, :] if mu == 0 else sel[:, None], (L, L)).copy()


def case_weights(g, ci):
    """the six conv parameters (numpy) of weight case `ci`: the base draw with the last bias overwritten"""
    w = [g[f'w{pi}'].copy() for pi in range(6)]
    w[5][:2] = g['case_sign'][ci] * g['case_s0'][ci]
    w[5][2] = 0.7
    return w


def si_of(g, ci):
    return S0.index(float(g['case_s0'][ci]))


def plaq_combos(g, L):
    """-> [(row, case, si, mu, off)] of the plaquette-level table of lattice size L"""
    return [(r, int(c), si_of(g, int(c)), int(mu), int(off)) for r, (c, mu, off) in enumerate(g[f'combo_L{L}'])]
