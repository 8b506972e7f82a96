"""CPU-only: the 32-bit offset arithmetic of the tuned flow kernels against the shapes their launchers accept.

The MFMA coupling kernels address the activation stash and the fields through 32-bit quantities (flow_mfma_common.h):
  * plane BASES as 32-bit element offsets of uniform_at() / stash_view() (then widened to 64 bits for the pointer),
  * offsets INSIDE a plane as 32-bit byte offsets, idx * 8u (ldu / ldu_j / stu / stu2 / sts / sts2).
The launchers accept flow_shape_ok(B, L, off) and flow_stash_fits32(B, L, train) (kernels.h).  The model below restates, for one
chain b < B of one layer (n = L * L), the largest value of every such quantity; the tests check that every accepted shape keeps all
of them below 2^32 and that the refusals start where the first of them stops fitting.  It is the precondition for running the
kernels at their limit shapes at all.
"""
import os
import re

import pytest

from conftest import ROOT

U32 = 1 << 32
KERNELS_H = os.path.join(ROOT, 'fthmc_amd', 'csrc', 'kernels.h')
MFMA_H = os.path.join(ROOT, 'fthmc_amd', 'csrc', 'flow_mfma_common.h')


# ---- the launchers' limits, restated from kernels.h (checked against its text below)
def flow_shape_ok(B, L, off=0):
    return 0 < B <= (1 << 20) and 4 <= L <= 8192 and L % 4 == 0 and 0 <= off < 4


def flow_stash_doubles(B, L, train):
    return B * (35 if train else 19) * L * L


def flow_stash_fits32(B, L, train):
    return flow_stash_doubles(B, L, train) < U32


def test_the_restated_limits_are_the_ones_in_kernels_h():
    src = open(KERNELS_H).read()
    assert re.search(r'flow_shape_ok\(int B, int L, int off\) \{ return B > 0 && B <= \(1 << 20\) && L >= 4 && L <= 8192 && '
                     r'\(L & 3\) == 0 && off >= 0 && off < 4; \}', src)
    assert 'return (size_t)B * (train ? 35 : 19) * L * L;' in src
    assert 'return flow_stash_doubles(B, L, train) < ((size_t)1 << 32);' in src
    # the stash layout the model restates (struct Stash / stash_view): the plane bases, in doubles
    mf = open(MFMA_H).read()
    for line in ('v.d1 = base + (size_t)(8u * bn);', 'v.d2 = base + (size_t)(8u * (Bn + bn));',
                 'v.tc = base + (size_t)(16u * Bn + 2u * bn);', 'v.cs = base + (size_t)(18u * Bn + bn);',
                 'v.h1 = base + (size_t)(19u * Bn + 8u * bn);', 'v.h2 = base + (size_t)(27u * Bn + 8u * bn);'):
        assert line in mf, line


# ---- the model
def plane_bases(B, L, train):
    """Largest 32-bit ELEMENT offset of a plane base, formed in unsigned 32-bit arithmetic, at b = B - 1:
      stash_view (flow_mfma_common.h), flow_bwd_gather.hip:117-119,248, flow_bwd_train.hip:270-300,324, flow_fwd.hip:196:
        d1 8 b n, d2 8 (B n + b n), tc 16 B n + 2 b n, cs 18 B n + b n; with h1 / h2 (training only) 19 B n + 8 b n, 27 B n + 8 b n
      the fields: flow_fwd.hip:107,511,593 (x, y: 2 b n), flow_bwd_gather.hip:171-174 (up_gp b n, up_link 2 b n + mu n),
        flow_bwd_gather.hip:537 / flow_bwd_train.hip:588 (gp_out b n)"""
    n, b = L * L, B - 1
    Bn, bn = B * n, b * n
    v = {'d1': 8 * bn, 'd2': 8 * (Bn + bn), 'tc': 16 * Bn + 2 * bn, 'cs': 18 * Bn + bn,
         'x': 2 * bn, 'up_link': 2 * bn + n, 'gp': bn}
    if train:
        v.update(h1=19 * Bn + 8 * bn, h2=27 * Bn + 8 * bn)
    return v


def plane_bytes(L, train):
    """Largest 32-bit BYTE offset inside one plane, idx * 8u:
      d1 [n][8]: 8 (n - 1) + 7 (flow_fwd.hip:278-313, flow_bwd_* through ldu);  d2 compact [3n/4][8]: 8 (3n/4 - 1) + 7 (:353);
      tc [n/4][4] of one mixture component: 4 (n/4 - 1) + 3 (:551-553);  cs [2][n/2]: n/2 + n/2 - 1 (:198);
      y [2][n]: n + n - 1 (:513, 595);  fields and gradient planes [n]: n - 1;  h1, h2 [n][8] (training): as d1"""
    n = L * L
    e = {'d1': 8 * n - 1, 'd2': 6 * n - 1, 'tc': n - 1, 'cs': n - 1, 'y': 2 * n - 1, 'field': n - 1}
    if train:
        e.update(h1=8 * n - 1, h2=8 * n - 1)
    return {k: 8 * v for k, v in e.items()}


def fits(B, L, train):
    return max(plane_bases(B, L, train).values()) < U32 and max(plane_bytes(L, train).values()) < U32


LS = list(range(4, 8192 + 4, 4))


def b_max_accepted(L, train):
    B = min(1 << 20, (U32 - 1) // flow_stash_doubles(1, L, train))
    assert flow_stash_fits32(B, L, train) and (B == 1 << 20 or not flow_stash_fits32(B + 1, L, train))
    return B


@pytest.mark.parametrize('train', [False, True])
def test_every_accepted_shape_fits_32_bits(train):
    """both quantities grow with B and L: the largest accepted B of every accepted L is the worst case of that L"""
    for L in LS:
        B = b_max_accepted(L, train)
        assert flow_shape_ok(B, L) and fits(B, L, train), (L, B, plane_bases(B, L, train), plane_bytes(L, train))


def test_the_lattice_limit_is_the_last_size_whose_planes_fit():
    """L = 8192: the act'(z1) plane's last byte offset is 64 n - 8 = 2^32 - 8; at L = 8196 (the first size flow_shape_ok refuses)
    it is past 2^32 -- the limit is exact, for the force and the training stash alike"""
    for train in (False, True):
        assert max(plane_bytes(8192, train).values()) == U32 - 8
        assert max(plane_bytes(8196, train).values()) >= U32
        assert flow_shape_ok(1, 8192) and not flow_shape_ok(1, 8196) and fits(1, 8192, train) and not fits(1, 8196, train)


@pytest.mark.parametrize('train', [False, True])
def test_the_chain_limit_is_the_stash_size_within_one_chain(train):
    """flow_stash_fits32 bounds the whole layer region (19 / 35 B n doubles); the largest base actually formed is that of the
    last plane of the last chain, 8 n (training: h2) or n (force: cs) doubles short of the region's end.  So the first B it
    refuses is the first that overflows, or one chain count below it; it never accepts one that overflows."""
    exact = 0
    for L in LS:
        B = b_max_accepted(L, train)
        if B == 1 << 20:
            continue
        first_bad = B + 1
        while fits(first_bad, L, train):
            first_bad += 1
        assert first_bad - (B + 1) in (0, 1), (L, B, first_bad)
        exact += first_bad == B + 1
    assert exact > len(LS) // 2


def test_stash_bases_of_the_accepted_training_shapes_at_the_headline_lattice():
    """L = 256, the training stash: 1872 chains fit (35 B n < 2^32), 1873 do not (27 B n + 8 (B - 1) n >= 2^32)"""
    assert b_max_accepted(256, True) == 1872
    assert fits(1872, 256, True) and not fits(1873, 256, True)


def test_plain_lattice_entry_points_refuse_shapes_past_their_limits():
    """FTHMC_MAX_L / FTHMC_MAX_B (include/fthmc_hip.h): the smallest refused shapes end in FTHMC_ERR_ARG before anything is
    enqueued (the pointers are never dereferenced)"""
    import ctypes
    from fthmc_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'fthmc_hip.h')).read()
    LMAX = int(re.search(r'#define FTHMC_MAX_L (\d+)', hdr).group(1))
    BMAX = int(re.search(r'#define FTHMC_MAX_B (\d+)', hdr).group(1))
    # the int arithmetic the limits restate: 2 L^2 in launch_kinetic / k_leap_rows, launch_metropolis's (2 L^2 + 2047) / 2048
    # and k_metropolis's walk s < 2 L^2, s += gy * 256 with gy clamped to 16 (wilson.hip launch_metropolis)
    src = open(os.path.join(ROOT, 'fthmc_amd', 'csrc', 'wilson.hip')).read()
    assert 'int gy = (2 * L * L + 2047) / 2048;' in src and 'if (gy > 16) gy = 16;' in src

    def int_ok(L):
        n2 = 2 * L * L
        gy = min((n2 + 2047) // 2048, 16)
        return n2 + 2047 < 1 << 31 and n2 + gy * 256 <= 1 << 31

    assert int_ok(LMAX) and not int_ok(LMAX + 4) and LMAX % 4 == 0
    assert BMAX * 1024 < U32 <= (BMAX + 1) * 1024
    lib = _lib.load()
    p = ctypes.c_void_p(64)
    for B, L in ((BMAX + 1, 4), (1, LMAX + 4), (1, 2), (0, 4), (1, 6)):
        assert lib.fthmc_plaquettes(p, p, B, L, None) == -1, (B, L)
        assert lib.fthmc_wilson_action_charge(p, B, L, 1.0, p, p, p, None) == -1, (B, L)
        assert lib.fthmc_wilson_force(p, B, L, 1.0, p, None) == -1, (B, L)
        assert lib.fthmc_kinetic(p, B, L, p, None) == -1, (B, L)
        assert lib.fthmc_leapfrog(p, p, B, L, 1.0, 0.1, 1, p, p, p, 1 << 40, None) == -1, (B, L)
        assert lib.fthmc_hmc_trajectory(p, p, p, B, L, 1.0, 0.1, 1, p, p, p, p, p, p, 1 << 40, None) == -1, (B, L)
    # fthmc_random_momenta takes (B, n_per_chain): at most a field of the largest lattice
    assert lib.fthmc_random_momenta(p, BMAX + 1, 32, p, p, None) == -1
    assert lib.fthmc_random_momenta(p, 1, 2 * LMAX * LMAX + 1, p, p, None) == -1
    assert lib.fthmc_random_momenta(p, 1, 2 ** 31 - 1, p, p, None) == -1


def test_flow_entry_points_refuse_the_first_chain_count_past_their_limit():
    """B = 2^20 + 1 with the default net (flow_shape_ok; include/fthmc_hip.h: B <= 2^20, else FTHMC_ERR_ARG): every flow entry
    point refuses before anything is enqueued, the weight expansion included (the pointers are never dereferenced; on a machine
    without a device a launch would be FTHMC_ERR_LAUNCH).  tests/test_limits_gpu.py runs B = 2^20."""
    import ctypes
    from fthmc_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)
    B, L, nl, big = (1 << 20) + 1, 4, 2, 1 << 50
    assert flow_shape_ok(B - 1, L) and not flow_shape_ok(B, L) and flow_stash_fits32(B, L, True)
    assert 'B <= 2^20, else FTHMC_ERR_ARG' in open(os.path.join(ROOT, 'include', 'fthmc_hip.h')).read()
    assert lib.fthmc_flow_layer_fwd(p, p, None, B, L, 0, 0, 0, p, p, p, big, None) == -1
    assert lib.fthmc_flow_layer_rev(p, p, None, B, L, 0, 0, 0, 1e-12, p, p, p, big, None) == -1
    assert lib.fthmc_flow_layer_bwd(p, p, None, p, p, B, L, 0, 0, 0, p, p, p, big, None) == -1
    assert lib.fthmc_flow_forward(p, p, None, nl, B, L, 0, p, p, p, big, None) == -1
    assert lib.fthmc_flow_reverse(p, p, None, nl, B, L, 0, 1e-12, p, p, p, big, None) == -1
    assert lib.fthmc_ft_action(p, p, None, nl, B, L, 0, 1.0, p, p, p, p, p, big, None) == -1
    assert lib.fthmc_ft_force(p, p, None, nl, B, L, 0, 1.0, p, p, big, None) == -1
    assert lib.fthmc_ft_leapfrog(p, p, p, None, nl, B, L, 0, 1.0, 0.1, 1, p, p, p, big, None) == -1
    assert lib.fthmc_train_grad(p, p, None, nl, B, L, 0, 1.0, p, p, p, p, p, big, None) == -1
