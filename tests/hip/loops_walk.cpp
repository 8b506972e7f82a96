// Stand-alone walk of the Wilson-loop entry points (fthmc_wilson_loops_ws_bytes, fthmc_wilson_loops) for
// tests/test_wilson_loops.py: built with AddressSanitizer + UBSan by `make -f san.mk san_loops` against the host-side sanitizer
// build of the library (launches are no-ops there) and run as a program of its own.  Every refusal the header lists, the smallest
// refused shapes, legal sizes up to B = 2^20 and L = FTHMC_MAX_L, workspace sizes monotone in every argument.  Device pointers are
// never dereferenced by the host side, so they are stand-in addresses.
#include "walk.h"

static int fail(const char* what, long a, long b, long c, long d, long rc) {
    fprintf(stderr, "loops_walk: %s (B %ld, L %ld, Rmax %ld, Tmax %ld) -> %ld\n", what, a, b, c, d, rc);
    return 1;
}

static int loops_call(int B, int L, int Rmax, int Tmax, int null_at, size_t ws_bytes) {
    return fthmc_wilson_loops(null_at == 0 ? NULL : dev(0), B, L, Rmax, Tmax, null_at == 1 ? NULL : dev(1), null_at == 2 ? NULL : dev(2),
                              null_at == 3 ? NULL : dev(3), ws_bytes, NULL);
}

static int want(int rc, int code, const char* what, long B, long L, long R, long T) { return answered(rc, code) ? 0 : fail(what, B, L, R, T, rc); }

int main() {
    const size_t big = (size_t)1 << 62;
    // ---- the refusals: pointers, B, L, Rmax, Tmax (FTHMC_ERR_ARG before anything else), then the workspace
    for (int at = 0; at < 2; ++at) WANT(loops_call(2, 8, 3, 3, at, big), FTHMC_ERR_ARG, "a null x / W not refused", 2, 8, 3, 3);
    WANT(loops_call(2, 8, 3, 3, 2, big), FTHMC_OK, "a null Wmean (optional) refused", 2, 8, 3, 3);
    WANT(loops_call(2, 8, 3, 3, 3, big), FTHMC_ERR_WS, "a null workspace not refused", 2, 8, 3, 3);
    const int badB[4] = {-1, 0, FTHMC_MAX_B + 1, 2147483647};
    for (int k = 0; k < 4; ++k) {
        WANT(loops_call(badB[k], 8, 3, 3, -1, big), FTHMC_ERR_ARG, "B out of range not refused", badB[k], 8, 3, 3);
        if (fthmc_wilson_loops_ws_bytes(badB[k], 8, 3, 3) != 0) return fail("ws_bytes of a refused B not 0", badB[k], 8, 3, 3, -1);
    }
    const int badL[11] = {-4, 0, 1, 2, 3, 5, 6, 7, 10, FTHMC_MAX_L + 4, 2147483644};
    for (int k = 0; k < 11; ++k) {
        WANT(loops_call(2, badL[k], 1, 1, -1, big), FTHMC_ERR_ARG, "L out of range not refused", 2, badL[k], 1, 1);
        if (fthmc_wilson_loops_ws_bytes(2, badL[k], 1, 1) != 0) return fail("ws_bytes of a refused L not 0", 2, badL[k], 1, 1, -1);
    }
    const int Ls[8] = {4, 8, 12, 20, 64, 1024, 1028, FTHMC_MAX_L};
    for (int li = 0; li < 8; ++li) {
        const int L = Ls[li];
        const int bad[5] = {-2147483647 - 1, -1, 0, L + 1, 2147483647};
        for (int k = 0; k < 5; ++k) {
            WANT(loops_call(1, L, bad[k], 1, -1, big), FTHMC_ERR_ARG, "Rmax outside [1, L] not refused", 1, L, bad[k], 1);
            WANT(loops_call(1, L, 1, bad[k], -1, big), FTHMC_ERR_ARG, "Tmax outside [1, L] not refused", 1, L, 1, bad[k]);
            if (fthmc_wilson_loops_ws_bytes(1, L, bad[k], 1) != 0 || fthmc_wilson_loops_ws_bytes(1, L, 1, bad[k]) != 0)
                return fail("ws_bytes of a refused table not 0", 1, L, bad[k], bad[k], -1);
        }
        // the legal corners of this L, each with its exact workspace, one double less, and none
        const int ext[3] = {1, L / 2 + 1, L};
        for (int r = 0; r < 3; ++r)
            for (int t = 0; t < 3; ++t)
                for (int bi = 0; bi < 3; ++bi) {
                    const int B = bi == 0 ? 1 : (bi == 1 ? 130 : 1 << 20), R = ext[r], T = ext[t];
                    const size_t need = fthmc_wilson_loops_ws_bytes(B, L, R, T);
                    if (need == 0) {                                      // a size beyond size_t: no workspace is long enough
                        WANT(loops_call(B, L, R, T, -1, big), FTHMC_ERR_WS, "a size beyond size_t not refused", B, L, R, T);
                        continue;
                    }
                    if (need % sizeof(double)) return fail("ws_bytes not a whole number of doubles", B, L, R, T, (long)need);
                    WANT(loops_call(B, L, R, T, -1, need), FTHMC_OK, "a legal call refused", B, L, R, T);
                    WANT(loops_call(B, L, R, T, 2, need), FTHMC_OK, "a legal call without Wmean refused", B, L, R, T);
                    WANT(loops_call(B, L, R, T, -1, need - 8), FTHMC_ERR_WS, "a workspace one double short not refused", B, L, R, T);
                    WANT(loops_call(B, L, R, T, -1, 0), FTHMC_ERR_WS, "an empty workspace not refused", B, L, R, T);
                }
    }
    WANT(loops_call(FTHMC_MAX_B, 4, 4, 4, -1, fthmc_wilson_loops_ws_bytes(FTHMC_MAX_B, 4, 4, 4)), FTHMC_OK, "the largest batch refused",
         FTHMC_MAX_B, 4, 4, 4);
    WANT(loops_call(1 << 20, FTHMC_MAX_L, 1, 1, -1, big), FTHMC_OK, "B = 2^20 at the largest L refused", 1 << 20, FTHMC_MAX_L, 1, 1);
    // ---- workspace sizes: monotone in B, L, Rmax and Tmax (a refused size, 0, only beyond every accepted one)
    size_t prevL = 0;
    for (int L = 4; L <= FTHMC_MAX_L; L += (L < 2100 ? 4 : 1020)) {
        const size_t nL = fthmc_wilson_loops_ws_bytes(3, L, 2, 3);
        if (nL == 0 || nL < prevL) return fail("ws_bytes not monotone in L", 3, L, 2, 3, (long)nL);
        prevL = nL;
        size_t prevB = 0;
        for (int lb = 0; lb <= 20; lb += 5) {
            const size_t nB = fthmc_wilson_loops_ws_bytes(1 << lb, L, 2, 3);
            if (nB == 0 || nB < prevB) return fail("ws_bytes not monotone in B", 1 << lb, L, 2, 3, (long)nB);
            prevB = nB;
        }
        size_t prevR = 0, prevT = 0;
        for (int R = 1; R <= L; R += 1 + L / 7) {
            const size_t nR = fthmc_wilson_loops_ws_bytes(2, L, R, 2), nT = fthmc_wilson_loops_ws_bytes(2, L, 2, R);
            if (nR == 0 || nR < prevR) return fail("ws_bytes not monotone in Rmax", 2, L, R, 2, (long)nR);
            if (nT == 0 || nT < prevT) return fail("ws_bytes not monotone in Tmax", 2, L, 2, R, (long)nT);
            prevR = nR; prevT = nT;
        }
    }
    return walked();
}
