// Stand-alone walk of the replica-exchange entry points (fthmc_ft_trajectory_pb_v, fthmc_hmc_trajectory_pb, fthmc_replica_swap,
// fthmc_ladder_init) for tests/test_tempering.py: built with AddressSanitizer + UBSan by `make -f san.mk san_tempering` against
// the host-side sanitizer build of the library (launches, copies and memsets are no-ops there) and run as a program of its own.
// Every refusal the header lists, then legal sizes up to K M = 2^20 and every branch of the two trajectory calls.  Device
// pointers are never dereferenced by the host side, so they are stand-in addresses; the one HOST array (the ladder handed to
// fthmc_ladder_init) is a heap block of exactly K doubles, so a read past it is a heap overflow the sanitizer reports.
#include "walk.h"

#include <math.h>

static int fail(const char* what, long a, long b, int rc) {
    fprintf(stderr, "tempering_walk: %s (%ld, %ld) -> %d\n", what, a, b, rc);
    return 1;
}
static int32_t* devi(int k) { return (int32_t*)dev(k); }
static int want(int rc, int code, const char* what, long a, long b) { return answered(rc, code) ? 0 : fail(what, a, b, rc); }

static int swap_call(int K, int M, int parity, int null_at) {
    const double* p[3] = {dev(0), dev(1), dev(2)};
    double* bb = dev(3); int32_t *rg = devi(4), *co = devi(5);
    if (null_at >= 0 && null_at < 3) p[null_at] = NULL;
    if (null_at == 3) bb = NULL;
    if (null_at == 4) rg = NULL;
    if (null_at == 5) co = NULL;
    return fthmc_replica_swap(p[0], K, M, parity, p[1], p[2], bb, rg, co, null_at == 6 ? NULL : dev(6), null_at == 7 ? NULL : dev(7), NULL);
}
static int init_call(const double* host, int K, int M, int null_at) {
    return fthmc_ladder_init(host, K, M, null_at == 0 ? NULL : dev(0), null_at == 1 ? NULL : dev(1), null_at == 2 ? NULL : devi(2),
                             null_at == 3 ? NULL : devi(3), NULL);
}
static double* ladder(int K) {
    double* h = (double*)malloc(sizeof(double) * (size_t)K);
    if (h) for (int k = 0; k < K; ++k) h[k] = 1.0 + 0.5 * k;
    return h;
}
static int ft_call(int B, int L, int nl, const fthmc_arch_t* arch, int integ, int mode, int nstep, const double* beta_b, size_t ws_bytes,
                   const double* state_in) {
    return fthmc_ft_trajectory_pb_v(dev(0), dev(1), dev(2), nl ? dev(3) : NULL, arch, nl, B, L, 0, beta_b, 0.1, nstep, mode, dev(4), dev(5),
                                    dev(6), NULL, NULL, dev(7), dev(8), state_in, dev(9), dev(10), ws_bytes, NULL, integ, 0);
}
static int hmc_call(int B, int L, int integ, int nstep, const double* beta_b, size_t ws_bytes, int inplace) {
    return fthmc_hmc_trajectory_pb(dev(0), dev(1), dev(2), B, L, beta_b, 0.1, nstep, integ, inplace ? dev(0) : dev(4), dev(5), dev(6), NULL,
                                   NULL, dev(10), ws_bytes, NULL);
}

int main() {
    // ---- fthmc_replica_swap / fthmc_ladder_init: the refusals
    for (int K = -1; K < 2; ++K) WANT(swap_call(K, 3, 0, -1), FTHMC_ERR_ARG, "swap: K < 2 not refused", K, 3);
    for (int M = -1; M < 1; ++M) WANT(swap_call(3, M, 0, -1), FTHMC_ERR_ARG, "swap: M < 1 not refused", 3, M);
    WANT(swap_call(2, FTHMC_MAX_B / 2 + 1, 0, -1), FTHMC_ERR_ARG, "swap: K M > FTHMC_MAX_B not refused", 2, FTHMC_MAX_B / 2 + 1);
    WANT(swap_call(65536, 65536, 0, -1), FTHMC_ERR_ARG, "swap: K M beyond int not refused", 65536, 65536);
    WANT(swap_call(2147483647, 2147483647, 1, -1), FTHMC_ERR_ARG, "swap: K M beyond int not refused", 2147483647, 2147483647);
    for (int parity = -2; parity <= 3; ++parity)
        if (parity != 0 && parity != 1) WANT(swap_call(4, 2, parity, -1), FTHMC_ERR_ARG, "swap: parity not refused", parity, 0);
    for (int at = 0; at < 6; ++at) WANT(swap_call(4, 2, 0, at), FTHMC_ERR_ARG, "swap: null pointer not refused", at, 0);
    for (int at = 6; at < 8; ++at) WANT(swap_call(4, 2, 1, at), FTHMC_OK, "swap: an optional output refused", at, 0);
    {
        double* h = ladder(4);
        if (!h) return fail("out of memory", 4, 0, 0);
        for (int K = -1; K < 2; ++K) WANT(init_call(h, K, 3, -1), FTHMC_ERR_ARG, "init: K < 2 not refused", K, 3);
        for (int M = -1; M < 1; ++M) WANT(init_call(h, 4, M, -1), FTHMC_ERR_ARG, "init: M < 1 not refused", 4, M);
        WANT(init_call(h, 4, FTHMC_MAX_B / 4 + 1, -1), FTHMC_ERR_ARG, "init: K M > FTHMC_MAX_B not refused", 4, FTHMC_MAX_B / 4 + 1);
        WANT(init_call(NULL, 4, 2, -1), FTHMC_ERR_ARG, "init: null host ladder not refused", 0, 0);
        for (int at = 0; at < 4; ++at) WANT(init_call(h, 4, 2, at), FTHMC_ERR_ARG, "init: null pointer not refused", at, 0);
        WANT(init_call(h, 4, 2, -1), FTHMC_OK, "init: a legal ladder refused", 4, 2);
        h[2] = h[1];
        WANT(init_call(h, 4, 2, -1), FTHMC_ERR_ARG, "init: equal neighbours not refused", 4, 2);
        h[2] = 0.5;
        WANT(init_call(h, 4, 2, -1), FTHMC_ERR_ARG, "init: a decreasing ladder not refused", 4, 2);
        h[2] = 2.0; h[3] = nan("");
        WANT(init_call(h, 4, 2, -1), FTHMC_ERR_ARG, "init: a NaN rung not refused", 4, 2);
        free(h);
    }
    // ---- legal sizes up to K M = 2^20 (and the largest the header allows)
    for (int lk = 1; lk <= 20; ++lk)
        for (int lm = 0; lk + lm <= 20; lm += (lm < 4 ? 1 : 3)) {
            const int Ks[3] = {1 << lk, (1 << lk) + 1, (1 << lk) - 1};
            for (int i = 0; i < 3; ++i) {
                const int K = Ks[i], M = (1 << lm) + (i == 1 ? 0 : (lm > 1));
                if (K < 2 || (long long)K * M > (1ll << 20)) continue;
                double* h = ladder(K);
                if (!h) return fail("out of memory", K, M, 0);
                WANT(init_call(h, K, M, -1), FTHMC_OK, "init: a legal size refused", K, M);
                free(h);
                WANT(swap_call(K, M, 0, -1), FTHMC_OK, "swap: a legal size refused", K, M);
                WANT(swap_call(K, M, 1, -1), FTHMC_OK, "swap: a legal size refused", K, M);
            }
        }
    WANT(swap_call(2, FTHMC_MAX_B / 2, 1, -1), FTHMC_OK, "swap: the largest batch refused", 2, FTHMC_MAX_B / 2);
    WANT(swap_call(FTHMC_MAX_B, 1, 0, -1), FTHMC_OK, "swap: the longest ladder refused", FTHMC_MAX_B, 1);

    // ---- the two trajectory calls: refusals, then every branch
    const size_t big = (size_t)1 << 62;
    WANT(ft_call(6, 8, 2, NULL, 0, FTHMC_MODE_MD, 3, NULL, big, NULL), FTHMC_ERR_ARG, "ft: null beta_b not refused", 0, 0);
    WANT(ft_call(0, 8, 2, NULL, 0, FTHMC_MODE_MD, 3, dev(11), big, NULL), FTHMC_ERR_ARG, "ft: B = 0 not refused", 0, 0);
    WANT(ft_call(6, 10, 2, NULL, 0, FTHMC_MODE_MD, 3, dev(11), big, NULL), FTHMC_ERR_ARG, "ft: L % 4 != 0 not refused", 0, 0);
    WANT(ft_call(6, 8, 2, NULL, 0, FTHMC_MODE_MD, 0, dev(11), big, NULL), FTHMC_ERR_ARG, "ft: nstep = 0 not refused", 0, 0);
    WANT(ft_call(6, 8, 2, NULL, 0, FTHMC_MODE_LITERAL, 3, dev(11), big, NULL), FTHMC_ERR_UNSUPPORTED, "ft: literal mode not refused", 0, 0);
    WANT(ft_call(6, 8, 2, NULL, 3, FTHMC_MODE_MD, 3, dev(11), big, NULL), FTHMC_ERR_UNSUPPORTED, "ft: unknown integrator not refused", 0, 0);
    WANT(ft_call(6, 8, 2, NULL, 0, FTHMC_MODE_MD, 3, dev(11), 8, NULL), FTHMC_ERR_WS, "ft: a short workspace not refused", 0, 0);
    WANT(hmc_call(6, 8, 0, 3, NULL, big, 0), FTHMC_ERR_ARG, "hmc: null beta_b not refused", 0, 0);
    WANT(hmc_call(6, 8, 0, 0, dev(11), big, 0), FTHMC_ERR_ARG, "hmc: nstep = 0 not refused", 0, 0);
    WANT(hmc_call(6, 6, 0, 3, dev(11), big, 0), FTHMC_ERR_ARG, "hmc: L % 4 != 0 not refused", 0, 0);
    WANT(hmc_call(6, 8, -1, 3, dev(11), big, 0), FTHMC_ERR_UNSUPPORTED, "hmc: unknown integrator not refused", 0, 0);
    WANT(hmc_call(6, 128, 1, 3, dev(11), 8, 0), FTHMC_ERR_WS, "hmc: a short workspace not refused", 0, 0);
    fthmc_arch_t gen = {1, {4, 0, 0, 0, 0, 0, 0, 0}, 3, 1, 0};
    const int Ls[7] = {8, 12, 16, 20, 32, 64, 128};
    for (int variant = 1; variant >= 0; --variant) {
        if (fthmc_set_variant(variant) != FTHMC_OK) return fail("fthmc_set_variant", variant, 0, 0);
        for (int small = 1; small >= 0; --small) {
            if (fthmc_set_small_path(small) != FTHMC_OK) return fail("fthmc_set_small_path", small, 0, 0);
            for (int li = 0; li < 7; ++li)
                for (int integ = 0; integ < 3; ++integ)
                    for (int nl = 0; nl <= 3; ++nl)
                        for (int g = 0; g < 2; ++g) {
                            const int L = Ls[li], B = li < 4 ? 6 : (li == 6 ? 2 : 4);
                            const fthmc_arch_t* arch = g ? &gen : NULL;
                            const size_t need = fthmc_ws_bytes(arch, B, L, nl);
                            if (!need) return fail("fthmc_ws_bytes = 0", B, L, 0);
                            for (int st = 0; st < 2; ++st)
                                WANT(ft_call(B, L, nl, arch, integ, FTHMC_MODE_MD, 1 + integ, dev(11), need, st ? dev(12) : NULL), FTHMC_OK,
                                     "ft: a legal call refused", L, nl);
                            WANT(ft_call(B, L, nl, arch, integ, FTHMC_MODE_MD, 2, dev(11), need - 8, NULL), FTHMC_ERR_WS,
                                 "ft: a workspace one double short not refused", L, nl);
                            if (nl == 0 && g == 0) {
                                const size_t n0 = fthmc_ws_bytes(NULL, B, L, 0);
                                WANT(hmc_call(B, L, integ, 2, dev(11), n0, 0), FTHMC_OK, "hmc: a legal call refused", L, integ);
                                WANT(hmc_call(B, L, integ, 2, dev(11), n0, 1), FTHMC_OK, "hmc: an in-place call refused", L, integ);
                            }
                        }
        }
    }
    WANT(ft_call(1 << 20, 8, 1, NULL, 0, FTHMC_MODE_MD, 1, dev(11), big, NULL), FTHMC_OK, "ft: B = 2^20 refused", 1 << 20, 8);
    WANT(hmc_call(1 << 20, 8, 2, 1, dev(11), big, 0), FTHMC_OK, "hmc: B = 2^20 refused", 1 << 20, 8);
    return walked();
}
