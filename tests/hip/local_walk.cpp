// Stand-alone walk of the local-update entry point (fthmc_local_update) for tests/test_local_update.py: built with AddressSanitizer +
// UBSan by `make -f san.mk san_local` against the host-side sanitizer build of the library (launches are no-ops there) and run as a
// program of its own.  Every refusal the header lists and the counter arithmetic at its edges; legal calls on both paths
// (fthmc_set_small_path 1 / 0) from the smallest to the largest shapes, every class mask, aliased and separate outputs, scalar and
// per-chain beta, which take the host code through its geometry and its loops over sweeps and classes.  The launches themselves are
// empty here: how many there are and in what order is what the device tests of the compositions see, not this program.  Device pointers are never dereferenced by the host side: stand-in addresses.
#include "walk.h"

struct Call {
    int B = 2, L = 8, n_hb = 1, n_or = 1, nsweep = 1, classes = 15;
    int64_t sweep0 = 0;
    bool null_x = false, null_out = false, null_seeds = false, pb = false, alias = false;
    int run() const {
        return fthmc_local_update(null_x ? NULL : dev(0), B, L, 2.0, pb ? dev(2) : NULL, null_seeds ? NULL : seeds(), n_hb, n_or, nsweep, sweep0,
                                  classes, null_out ? NULL : (alias ? dev(0) : dev(1)), NULL);
    }
};

static int want(const Call& c, int code, const char* what) {
    const int rc = c.run();
    if (answered(rc, code)) return 0;
    fprintf(stderr, "local_walk: %s (B %d, L %d, n_hb %d, n_or %d, nsweep %d, sweep0 %lld, classes %d) -> %d, expected %d\n", what, c.B, c.L,
            c.n_hb, c.n_or, c.nsweep, (long long)c.sweep0, c.classes, rc, code);
    return 1;
}

int main() {
    const int64_t two32 = (int64_t)1 << 32;
    for (int path = 1; path >= 0; --path) {
        if (fthmc_set_small_path(path) != FTHMC_OK || fthmc_get_small_path() != path) { fprintf(stderr, "local_walk: set_small_path\n"); return 1; }
        // ---- the refusals
        { Call c; c.null_x = true; WANT(c, FTHMC_ERR_ARG, "a null x not refused"); }
        { Call c; c.null_out = true; WANT(c, FTHMC_ERR_ARG, "a null x_out not refused"); }
        { Call c; c.null_seeds = true; WANT(c, FTHMC_ERR_ARG, "null seeds with heatbath sweeps not refused"); }
        { Call c; c.null_seeds = true; c.n_hb = 0; WANT(c, FTHMC_OK, "null seeds without heatbath sweeps refused"); }
        const int badB[4] = {-1, 0, FTHMC_MAX_B + 1, 2147483647};
        for (int k = 0; k < 4; ++k) { Call c; c.B = badB[k]; WANT(c, FTHMC_ERR_ARG, "B out of range not refused"); }
        const int badL[11] = {-4, 0, 1, 2, 3, 5, 6, 7, 10, FTHMC_MAX_L + 4, 2147483644};
        for (int k = 0; k < 11; ++k) { Call c; c.L = badL[k]; WANT(c, FTHMC_ERR_ARG, "L out of range not refused"); }
        const int neg[3] = {-1, -2147483647 - 1, -65536};
        for (int k = 0; k < 3; ++k) {
            { Call c; c.n_hb = neg[k]; WANT(c, FTHMC_ERR_ARG, "a negative n_hb not refused"); }
            { Call c; c.n_or = neg[k]; WANT(c, FTHMC_ERR_ARG, "a negative n_or not refused"); }
            { Call c; c.nsweep = neg[k]; WANT(c, FTHMC_ERR_ARG, "a negative nsweep not refused"); }
            { Call c; c.sweep0 = neg[k]; WANT(c, FTHMC_ERR_ARG, "a negative sweep0 not refused"); }
        }
        { Call c; c.sweep0 = INT64_MIN; WANT(c, FTHMC_ERR_ARG, "sweep0 = INT64_MIN not refused"); }
        const int badC[6] = {0, 16, -1, 255, 2147483647, -2147483647 - 1};
        for (int k = 0; k < 6; ++k) { Call c; c.classes = badC[k]; WANT(c, FTHMC_ERR_ARG, "classes outside 1 .. 15 not refused"); }
        // ---- the counter field: sweep0 + nsweep n_hb <= 2^32, in arithmetic that cannot overflow
        { Call c; c.sweep0 = two32 - 1; c.n_or = 0; WANT(c, FTHMC_OK, "the last sweep index refused"); }
        { Call c; c.sweep0 = two32; c.n_hb = 0; WANT(c, FTHMC_OK, "sweep0 = 2^32 without a heatbath sweep refused"); }
        { Call c; c.sweep0 = two32; WANT(c, FTHMC_ERR_ARG, "a sweep index of 2^32 not refused"); }
        { Call c; c.sweep0 = two32 - 1; c.nsweep = 2; WANT(c, FTHMC_ERR_ARG, "a sweep index of 2^32 not refused (second sweep)"); }
        { Call c; c.sweep0 = two32 - 6; c.nsweep = 2; c.n_hb = 3; c.n_or = 0; WANT(c, FTHMC_OK, "the last six sweep indices refused"); }
        { Call c; c.sweep0 = two32 - 5; c.nsweep = 2; c.n_hb = 3; WANT(c, FTHMC_ERR_ARG, "one sweep index too many not refused"); }
        { Call c; c.sweep0 = two32 + 1; c.n_hb = 0; WANT(c, FTHMC_ERR_ARG, "sweep0 beyond the counter field not refused"); }
        { Call c; c.sweep0 = INT64_MAX; WANT(c, FTHMC_ERR_ARG, "sweep0 = INT64_MAX not refused"); }
        { Call c; c.sweep0 = INT64_MAX; c.n_hb = 2147483647; c.nsweep = 2147483647; WANT(c, FTHMC_ERR_ARG, "the largest arguments not refused"); }
        { Call c; c.n_hb = 2147483647; c.nsweep = 2147483647; WANT(c, FTHMC_ERR_ARG, "2^62 heatbath sweeps not refused"); }
        { Call c; c.n_hb = 65536; c.nsweep = 65537; WANT(c, FTHMC_ERR_ARG, "2^32 + 2^16 heatbath sweeps not refused"); }
        // ---- legal calls: every mask, both betas, aliased and not, the shapes where the path or the launch geometry changes
        const int Ls[9] = {4, 8, 12, 20, 64, 68, 128, 1024, FTHMC_MAX_L};
        const int Bs[4] = {1, 130, 66000, FTHMC_MAX_B};
        for (int li = 0; li < 9; ++li)
            for (int bi = 0; bi < 4; ++bi)
                for (int v = 0; v < 4; ++v) {
                    Call c; c.L = Ls[li]; c.B = Bs[bi]; c.pb = v & 1; c.alias = v & 2; c.n_hb = 1 + (v & 1); c.n_or = v; c.nsweep = 1 + bi;
                    WANT(c, FTHMC_OK, "a legal call refused");
                }
        for (int m = 1; m <= 15; ++m) { Call c; c.classes = m; c.alias = m & 1; WANT(c, FTHMC_OK, "a legal class mask refused"); }
        { Call c; c.n_hb = 0; c.n_or = 0; WANT(c, FTHMC_OK, "a call without sweeps refused"); }
        { Call c; c.nsweep = 0; WANT(c, FTHMC_OK, "a call with nsweep = 0 refused"); }
        { Call c; c.nsweep = 2000; c.n_hb = 2; c.n_or = 3; c.L = 68; WANT(c, FTHMC_OK, "a long call refused"); }
    }
    if (fthmc_set_small_path(1) != FTHMC_OK) return 1;
    return walked();
}
