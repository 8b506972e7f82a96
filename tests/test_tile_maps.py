"""Tile maps of the coupling-layer forward with aligned tile origins (fthmc_amd/csrc/flow_fwd.hip, the EXACT instances), on
the CPU: the line counts that motivate the alignment, from the stripe formula alone, and a Python model of the kernel's
stage-0 / conv1 / conv2 maps (the same index arithmetic, lane by lane) showing that every (line, position) a later stage
reads is produced exactly once and that nothing outside the LDS planes is addressed."""
import itertools

import pytest

T = 16                      # tile edge
TOFF = 1                    # residue mod 4 of the active lines in tile coordinates: tile origin = off + 3 (mod 4)
R0, R1, R2 = T + 6, T + 4, T + 2                   # input / h1 / h2 window ALONG the stripe lines (flow_mfma_common.h Geom)
X0, X1 = R0 - 2, R1 - 2                            # ... and ACROSS them with aligned origins: 20 input lines, 18 h1 lines
NW = 8


def ps_round16(n):
    return (n - 16 + 31) // 32 * 32 + 16


def ps_round(n):
    return (n - 18 + 31) // 32 * 32 + 18


def geom(mu):
    """(rows, row stride) of the input window, (rows, row stride) of the h1 window, plane strides: Geom<16, 16, MU, true>"""
    r0r, r0c = (R0, X0) if mu == 0 else (X0, R0)
    r1r, r1c = (R1, X1) if mu == 0 else (X1, R1)
    rs1 = r1c + 1
    assert rs1 % 2 == 1
    return r0r, r0c, r1r, rs1, ps_round16(r0r * r0c), ps_round16(r1r * rs1)


PS2 = ps_round(R2 * R2)


def test_lds_plan():
    for mu in (0, 1):
        r0r, r0c, r1r, rs1, ps0, ps1 = geom(mu)
        assert ps0 % 32 == 16 and ps1 % 32 == 16 and PS2 % 32 == 18 and ps0 >= r0r * r0c and ps1 >= r1r * rs1
        IN = max(8 * ps1, 8 * PS2)
        size = IN + max(2 * ps0 + 352, 8 * 3 * 64 + 2 * 2 * 64) + r0r * r0c + 980      # SmemF: LF_P1_SIZE = 352, LF_SIZE = 980
        assert size * 8 == 51296
        assert 3 * ((size * 8 + 1279) // 1280 * 1280) <= 160 * 1024                     # three workgroups per CU


# ---------------------------------------------------------------- line counts from the stripe formula
def fwd_lines(t0, off):
    """lines ACROSS the stripe direction that a force-sweep tile t0 .. t0 + 15 must produce (active lines g % 4 == off)"""
    own = range(t0, t0 + T)
    act = [g for g in own if (g - off) % 4 == 0]
    h2 = {g + d for g in act for d in (-1, 0, 1)} | {g for g in own if (g - off) % 4 != 2}
    h1 = {g + d for g in h2 for d in (-1, 0, 1)} | set(own)
    frozen = {g + d for g in h1 for d in (-1, 0, 1) if (g + d - off) % 4 in (1, 2)}
    live_today = {g for g in range(t0 - 1, t0 + T + 1) if (g - off) % 4 != 2}
    return h2, h1, frozen, live_today


def bwd_lines(t0, off):
    own = range(t0, t0 + T)
    fro = {g for g in own if (g - off) % 4 in (1, 2)}
    gz1 = {g + d for g in fro for d in (-1, 0, 1)}
    gz2 = {g + d for g in gz1 for d in (-1, 0, 1) if (g + d - off) % 4 != 2}
    active = {g + d for g in gz2 for d in (-1, 0, 1) if (g + d - off) % 4 == 0}
    return gz1, gz2, active


@pytest.mark.parametrize('off', range(4))
def test_forward_line_counts(off):
    want = {0: (14, 13, 19, 11), 1: (14, 13, 19, 10), 2: (13, 12, 17, 10), 3: (13, 12, 17, 10)}
    for t0 in range(0, 64):
        h2, h1, frozen, live_today = fwd_lines(t0, off)
        assert (len(live_today), len(h2), len(h1), len(frozen)) == want[(t0 - off) % 4], (t0, off)
    # at the phases 2, 3 conv3 reads exactly the tile's own live lines: conv2 has no halo across the lines
    for ph in (2, 3):
        t0 = 16 + off + ph
        h2 = fwd_lines(t0, off)[0]
        assert h2 == {g for g in range(t0, t0 + T) if (g - off) % 4 != 2}


@pytest.mark.parametrize('off', range(4))
def test_backward_line_counts(off):
    # gz1 lines, live gz2 lines, active lines a tile needs for its own frozen sites (the kernel walks 18 / 15 / 6 at any phase)
    want = {0: (16, 14, 5), 1: (16, 14, 5), 2: (18, 15, 6), 3: (16, 14, 5)}
    for t0 in range(0, 64):
        gz1, gz2, active = bwd_lines(t0, off)
        assert (len(gz1), len(gz2), len(active)) == want[(t0 - off) % 4], (t0, off)


def test_shift_gives_the_tile_residue():
    for off, L, t in itertools.product(range(4), (16, 32, 64, 8192), range(4)):
        origin = (16 * t + (off + 3) % 4) % L
        assert (off - origin) % 4 == TOFF
        # the forward phase of the issue's table: 3
        assert (origin - off) % 4 == 3


# ---------------------------------------------------------------- the kernel's maps, lane by lane
# window coordinates: input window line w = tile line + 3, h1 window = tile + 2, h2 window = tile + 1
ACT_T = [TOFF + 4 * m for m in range(4)]                               # active tile lines
LIVE_T = [t for t in range(T) if (t - TOFF) % 4 != 2]                  # the tile's own live lines


def needed():
    h2 = sorted({a + d for a in ACT_T for d in (-1, 0, 1)} | set(LIVE_T))          # tile lines
    h1 = sorted({t + d for t in h2 for d in (-1, 0, 1)} | set(range(T)))
    fz = sorted({t + d for t in h1 for d in (-1, 0, 1) if (t + d - TOFF) % 4 in (1, 2)})
    return h2, h1, fz


def test_needed_lines_are_the_tiles_own():
    h2, h1, fz = needed()
    assert h2 == LIVE_T and len(h2) == 12
    assert h1 == list(range(-1, 16)) and len(fz) == 10
    assert fz == [w - 3 for w in (1, 2, 5, 6, 9, 10, 13, 14, 17, 18)]


def site(mu, across, along):
    """(row, column) of a window site given its line across the stripe direction and its position along"""
    return (along, across) if mu == 0 else (across, along)


@pytest.mark.parametrize('mu', (0, 1))
def test_stage0_map(mu):
    NFL, NA, NCC = 10, 64, 12
    NFT = R0 * NFL
    assert NFT + NA + NCC <= 512
    r0r, r0c, _, _, PS0, _ = geom(mu)
    frozen, active, const = {}, {}, {}
    for tid in range(512):
        if tid < NFT:
            a, k = divmod(tid, NFL)
            x = TOFF + 4 * (k >> 1) + (k & 1)
            assert 0 <= x < X0
            rc = site(mu, x, a)
            assert rc not in frozen
            frozen[rc] = tid
        elif tid < NFT + NA:
            a = tid - NFT
            r = 3 + (a // 4 if mu == 0 else TOFF + 4 * (a // T))
            c = 3 + (TOFF + 4 * (a % 4) if mu == 0 else a % T)
            assert (r, c) not in active
            active[(r, c)] = tid
            # the three scratch slots on the following lines stay inside the window
            st = 1 if mu == 0 else r0c
            assert r < r0r and c + (3 if mu == 0 else 0) < r0c and r * r0c + c + 3 * st < r0r * r0c
        elif tid < NFT + NA + NCC:
            k = tid - NFT - NA
            rc = site(mu, 16 + 3 * (k & 1), 16 + (k >> 1))
            assert rc not in const and rc not in frozen
            const[rc] = tid
    for (r, c) in list(frozen) + list(const):
        assert 0 <= r < r0r and 0 <= c < r0c and r * r0c + c < PS0
    # frozen: the 10 lines conv1 reads, every position along; active: the tile's own active sites
    fz = needed()[2]
    assert set(frozen) == {site(mu, t + 3, a) for t in fz for a in range(R0)}
    assert set(active) == {site(mu, t + 3, a + 3) for t in ACT_T for a in range(T)}
    # the constant (1, 0): what the leftover pairs (h1 window lines 16, 17 across, 16 .. 19 along, all 18 taps) read off the frozen lines
    reads = {site(mu, x + dx, v + dv) for x in (16, 17) for v in range(16, 20) for dx in range(3) for dv in range(3)}
    assert {rc for rc in reads if rc not in frozen} == set(const)


def conv1_map(mu):
    """-> {(across, along) in h1 window coordinates: how often produced}, and the input lines each MFMA pair reads"""
    NU1, NREMP = 9, 4
    made, reads = {}, set()
    r0r, r0c, r1r, RS1, _, PS1 = geom(mu)

    def tile(u, v, par):
        assert par == u & 1 and 0 <= u < NU1 and 0 <= v < R1
        s4 = (0 + 2 * par) & 3
        for g in range(4):
            fl = ((g >> 1) + 1 - s4) & 3                                # the lane group's frozen line of the pair window
            for t in range(3):
                x, a = 2 * u + fl, v + t                                # input window line across, position along
                assert (x - 3 - TOFF) % 4 in (1, 2), 'an MFMA operand line must be frozen'
                r, c = site(mu, x, a)
                assert 0 <= r < r0r and 0 <= c < r0c
                reads.add((x, a))
        for dd in range(2):
            key = (2 * u + dd, v)
            made[key] = made.get(key, 0) + 1
            r, c = site(mu, *key)
            assert 0 <= r < r1r and 0 <= c < RS1 - 1 and r * RS1 + c < PS1

    for wave in range(NW):
        for i in range(16):
            tile(wave, i, wave & 1)
            Tn = wave + NW
            if Tn < NU1:
                tile(Tn, i, Tn & 1)
            elif Tn < NU1 + 2:
                tile(2 * (i >> 2) + (Tn - NU1), 16 + (i & 3), Tn - NU1)
    nrem = 0
    for idx in range(2 * NREMP * 8):                                    # leftover threads: (site, output channel)
        s, co = idx >> 3, idx & 7
        pair, sd = s >> 1, s & 1
        assert pair < NREMP
        v, u = R1 - NREMP + pair, NU1 - 1
        if co == 0:
            made[(2 * u + sd, v)] = made.get((2 * u + sd, v), 0) + 1
        nrem += 1
    assert nrem == 64
    return made, reads


@pytest.mark.parametrize('mu', (0, 1))
def test_conv1_map(mu):
    made, reads = conv1_map(mu)
    # 18 lines across (window 0 .. 17 = tile -2 .. 15) x 20 along, each exactly once: 11 tiles + 4 leftover pairs
    assert set(made) == {(x, v) for x in range(18) for v in range(R1)} and set(made.values()) == {1}
    assert len(made) == 2 * (11 * 16 + 4)
    h1 = needed()[1]
    assert {t + 2 for t in h1} <= {x for x, _ in made}
    # the MFMA tiles read frozen lines that stage 0 wrote
    assert {x for x, _ in reads} <= {1, 2, 5, 6, 9, 10, 13, 14, 17, 18}


def conv2_map(mu):
    NPL, NL2, NT2 = R2 // 2, 12, 7
    assert NT2 == (NPL * NL2 + 15) // 16
    made, h1_reads = {}, set()
    _, _, r1r, RS1, _, PS1 = geom(mu)
    for wave in range(NT2):
        for i in range(16):
            p = 16 * wave + i
            if p >= NPL * NL2:
                continue
            pl, l = divmod(p, NL2)
            wl = 1 + l + l // 3
            for dd in range(2):
                key = (wl, 2 * pl + dd)                                 # (line across, position along), h2 window coordinates
                made[key] = made.get(key, 0) + 1
                r, c = site(mu, *key)
                assert 0 <= r < R2 and 0 <= c < R2 and r * R2 + c < PS2
            # operand window in h1 coordinates: lines wl .. wl + 2 across, positions 2 pl .. 2 pl + 3 along
            for dx in range(3):
                for da in range(4):
                    r, c = site(mu, wl + dx, 2 * pl + da)
                    assert 0 <= r < r1r and 0 <= c < RS1 - 1 and r * RS1 + c < PS1
                    h1_reads.add((wl + dx, 2 * pl + da))
    return made, h1_reads


@pytest.mark.parametrize('mu', (0, 1))
def test_conv2_map(mu):
    made, h1_reads = conv2_map(mu)
    live_w = [t + 1 for t in LIVE_T]
    assert set(made) == {(x, a) for x in live_w for a in range(R2)} and set(made.values()) == {1}
    assert len(made) == 2 * 108
    # everything conv2 reads was produced by conv1
    assert h1_reads <= set(conv1_map(mu)[0])
    # everything conv3 reads (3 x 3 around the tile's active sites, h2 window = tile + 1) was produced by conv2
    conv3 = {(t + 1 + dx, a + 1 + da) for t in ACT_T for a in range(T) for dx in (-1, 0, 1) for da in (-1, 0, 1)}
    assert conv3 <= set(made)
    # and the act'(z2) stash of the tile's own live sites
    assert {(t + 1, a + 1) for t in LIVE_T for a in range(T)} <= set(made)


@pytest.mark.parametrize('L', (16, 32, 64, 8192))
def test_own_sites_cover_the_lattice_once(L):
    """with wrapped global lines the tiles of a layer still partition the lattice lines, for every off"""
    for off in range(4):
        shift = (off + 3) % 4
        lines = [(16 * t + shift + r) & (L - 1) for t in range(L // 16) for r in range(16)]
        assert sorted(lines) == list(range(L))
        for t in range(L // 16):
            for r in range(16):
                g = (16 * t + shift + r) & (L - 1)
                assert ((g - off) % 4 == 0) == (r % 4 == TOFF)
