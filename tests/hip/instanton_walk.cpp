// Stand-alone walk of the instanton-hit entry points (fthmc_instanton_hit, fthmc_instanton_ws_bytes) and of the integer reductions the
// kernels form their angles from (csrc/topo_int.h) for tests/test_instanton.py: built with AddressSanitizer + UBSan by
// `make -f san.mk san_instanton` against the host-side sanitizer build of the library (launches are no-ops there) and run as a program
// of its own.  Every refusal the header lists, the hit0 arithmetic at 2^32 and at the INT64 extremes, the workspace rule, legal calls
// on both paths from the smallest to the largest shapes; then the reductions for k = +-1024 at L = 4 and L = FTHMC_MAX_L: every result
// in its range and congruent to the unreduced product, no signed overflow on the way.  Device pointers are never dereferenced by
// the host side: stand-in addresses.
#include "walk.h"
#include "../../fthmc_amd/csrc/topo_int.h"

static long reductions = 0;

struct Call {
    int B = 2, L = 8, n_hit = 1, path = 1;
    int64_t hit0 = 0;
    bool null_x = false, null_out = false, null_seeds = false, pb = false, alias = false, outs = false, null_ws = false;
    long long ws_short = 0;                       // bytes taken off the workspace size the library asks for
    int run() const {
        const size_t need = fthmc_instanton_ws_bytes(B, L, path);
        return fthmc_instanton_hit(null_x ? NULL : dev(0), B, L, 2.0, pb ? dev(2) : NULL, null_seeds ? NULL : seeds(), n_hit, hit0, path,
                                   null_out ? NULL : (alias ? dev(0) : dev(1)), outs ? ints(0) : NULL, outs ? ints(1) : NULL,
                                   outs ? dev(3) : NULL, null_ws ? NULL : wsp(), need - (size_t)ws_short, NULL);
    }
};

static int want(const Call& c, int code, const char* what) {
    const int rc = c.run();
    if (answered(rc, code)) return 0;
    fprintf(stderr, "instanton_walk: %s (B %d, L %d, n_hit %d, hit0 %lld, path %d) -> %d, expected %d\n", what, c.B, c.L, c.n_hit,
            (long long)c.hit0, c.path, rc, code);
    return 1;
}

static int reduce_walk(int L) {
    using namespace fthmc;
    const int64_t V = (int64_t)L * L;
    const int ks[6] = {IT_MAX_HITS, -IT_MAX_HITS, IT_MAX_HITS - 1, -IT_MAX_HITS + 1, 1, -1};
    for (int q = 0; q < 6; ++q) {
        const int k = ks[q];
        for (int i = 0; i < L; ++i) {
            const int64_t a = it_shift_num_x1(k, i, L), b = it_shift_num_seam(k, i, L);
            const __int128 p = (__int128)k * i;
            if (a < 0 || a >= V || (p - a) % V != 0 || b < 0 || b >= L || (p - b) % L != 0) {
                fprintf(stderr, "instanton_walk: reduction of k i = %d * %d at L = %d: %lld, %lld\n", k, i, L, (long long)a, (long long)b);
                return 1;
            }
            reductions += 2;
        }
        for (int s = -1; s <= 1; s += 2) {
            const int64_t t = it_theta_num(k, s, L);
            if (t < 0 || t >= 2 * V || ((__int128)2 * k + s - t) % (2 * V) != 0) {
                fprintf(stderr, "instanton_walk: theta of k = %d, s = %d at L = %d: %lld\n", k, s, L, (long long)t);
                return 1;
            }
            ++reductions;
        }
    }
    if (it_mod(INT64_MIN + 1, 3) != (int64_t)((((__int128)INT64_MIN + 1) % 3 + 3) % 3) || it_mod(INT64_MAX, INT64_MAX) != 0 || it_mod(-1, INT64_MAX) != INT64_MAX - 1) {
        fprintf(stderr, "instanton_walk: it_mod at the extremes\n");
        return 1;
    }
    return 0;
}

int main() {
    const int64_t two32 = (int64_t)1 << 32;
    for (int path = 0; path <= 2; ++path) {
        // ---- the refusals
        { Call c; c.path = path; c.null_x = true; WANT(c, FTHMC_ERR_ARG, "a null x not refused"); }
        { Call c; c.path = path; c.null_out = true; WANT(c, FTHMC_ERR_ARG, "a null x_out not refused"); }
        { Call c; c.path = path; c.null_seeds = true; WANT(c, FTHMC_ERR_ARG, "null seeds with a hit not refused"); }
        { Call c; c.path = path; c.null_seeds = true; c.n_hit = 0; WANT(c, FTHMC_OK, "null seeds without a hit refused"); }
        const int badB[4] = {-1, 0, FTHMC_MAX_B + 1, 2147483647};
        for (int k = 0; k < 4; ++k) { Call c; c.path = path; c.B = badB[k]; WANT(c, FTHMC_ERR_ARG, "B out of range not refused"); }
        const int badL[11] = {-4, 0, 1, 2, 3, 5, 6, 7, 10, FTHMC_MAX_L + 4, 2147483644};
        for (int k = 0; k < 11; ++k) { Call c; c.path = path; c.L = badL[k]; WANT(c, FTHMC_ERR_ARG, "L out of range not refused"); }
        const int badN[5] = {-1, 1025, 65536, 2147483647, -2147483647 - 1};
        for (int k = 0; k < 5; ++k) { Call c; c.path = path; c.n_hit = badN[k]; WANT(c, FTHMC_ERR_ARG, "n_hit outside 0 .. 1024 not refused"); }
        // ---- the counter field: hit0 + n_hit <= 2^32, in arithmetic that cannot overflow
        { Call c; c.path = path; c.hit0 = -1; WANT(c, FTHMC_ERR_ARG, "a negative hit0 not refused"); }
        { Call c; c.path = path; c.hit0 = INT64_MIN; WANT(c, FTHMC_ERR_ARG, "hit0 = INT64_MIN not refused"); }
        { Call c; c.path = path; c.hit0 = INT64_MIN; c.n_hit = 1024; WANT(c, FTHMC_ERR_ARG, "hit0 = INT64_MIN with 1024 hits not refused"); }
        { Call c; c.path = path; c.hit0 = INT64_MAX; WANT(c, FTHMC_ERR_ARG, "hit0 = INT64_MAX not refused"); }
        { Call c; c.path = path; c.hit0 = INT64_MAX; c.n_hit = 1024; WANT(c, FTHMC_ERR_ARG, "hit0 = INT64_MAX with 1024 hits not refused"); }
        { Call c; c.path = path; c.hit0 = INT64_MAX; c.n_hit = 0; WANT(c, FTHMC_ERR_ARG, "hit0 = INT64_MAX without a hit not refused"); }
        { Call c; c.path = path; c.hit0 = two32 - 1; WANT(c, FTHMC_OK, "the last hit index refused"); }
        { Call c; c.path = path; c.hit0 = two32; WANT(c, FTHMC_ERR_ARG, "a hit index of 2^32 not refused"); }
        { Call c; c.path = path; c.hit0 = two32; c.n_hit = 0; WANT(c, FTHMC_OK, "hit0 = 2^32 without a hit refused"); }
        { Call c; c.path = path; c.hit0 = two32 + 1; c.n_hit = 0; WANT(c, FTHMC_ERR_ARG, "hit0 beyond the counter field not refused"); }
        { Call c; c.path = path; c.hit0 = two32 - 1024; c.n_hit = 1024; WANT(c, FTHMC_OK, "the last 1024 hit indices refused"); }
        { Call c; c.path = path; c.hit0 = two32 - 1023; c.n_hit = 1024; WANT(c, FTHMC_ERR_ARG, "one hit index too many not refused"); }
        { Call c; c.path = path; c.hit0 = two32 - 64; c.n_hit = 64; c.outs = true; WANT(c, FTHMC_OK, "the last 64 hit indices refused"); }
    }
    const int badP[5] = {-1, 3, 255, 2147483647, -2147483647 - 1};
    for (int k = 0; k < 5; ++k) { Call c; c.path = badP[k]; WANT(c, FTHMC_ERR_ARG, "path outside 0 .. 2 not refused"); }
    // ---- the workspace rule (sizes are rounded up to a multiple of 256 bytes, like every workspace size of the header)
    auto up256 = [](size_t n) { return (n + 255) / 256 * 256; };
    if (fthmc_instanton_ws_bytes(2, 8, 1) != 0 || fthmc_instanton_ws_bytes(2, 8, 0) != 0 || fthmc_instanton_ws_bytes(64, 128, 0) != 0 ||
        fthmc_instanton_ws_bytes(63, 128, 0) == 0 || fthmc_instanton_ws_bytes(63, 128, 0) != fthmc_instanton_ws_bytes(63, 128, 2) ||
        fthmc_instanton_ws_bytes(2, 8, 2) != up256(2 * 4 * 2 * sizeof(double) + 8) || fthmc_instanton_ws_bytes(0, 8, 2) != 0 ||
        fthmc_instanton_ws_bytes(2, 8, 3) != 0 || fthmc_instanton_ws_bytes(FTHMC_MAX_B, FTHMC_MAX_L, 2) != up256((size_t)FTHMC_MAX_B * 16 * 2 * 8 + ((size_t)FTHMC_MAX_B * 4 + 7) / 8 * 8)) {
        fprintf(stderr, "instanton_walk: fthmc_instanton_ws_bytes\n");
        return 1;
    }
    calls += 9;
    { Call c; c.path = 2; c.null_ws = true; WANT(c, FTHMC_ERR_WS, "a null workspace not refused"); }
    { Call c; c.path = 2; c.ws_short = 1; WANT(c, FTHMC_ERR_WS, "a short workspace not refused"); }
    { Call c; c.path = 2; c.ws_short = 136; WANT(c, FTHMC_ERR_WS, "an empty workspace not refused"); }
    { Call c; c.path = 0; c.B = 3; c.L = 128; c.ws_short = 8; WANT(c, FTHMC_ERR_WS, "a short workspace not refused (path 0)"); }
    { Call c; c.path = 1; c.null_ws = true; WANT(c, FTHMC_OK, "a null workspace refused where none is needed"); }
    { Call c; c.path = 0; c.null_ws = true; WANT(c, FTHMC_OK, "a null workspace refused where none is needed (path 0)"); }
    // ---- legal calls: both paths and the library's choice, both betas, aliased and not, optional outputs, the shapes where the launch
    // geometry changes
    const int Ls[10] = {4, 8, 12, 20, 28, 32, 64, 68, 128, FTHMC_MAX_L};
    const int Bs[5] = {1, 63, 130, 66000, FTHMC_MAX_B};
    for (int li = 0; li < 10; ++li)
        for (int bi = 0; bi < 5; ++bi)
            for (int v = 0; v < 4; ++v)
                for (int path = 0; path <= 2; ++path) {
                    Call c; c.L = Ls[li]; c.B = Bs[bi]; c.path = path; c.pb = v & 1; c.alias = v & 2; c.outs = v == 1 || v == 2;
                    c.n_hit = v == 0 ? 0 : (v == 3 ? 1024 : 1 + bi);
                    WANT(c, FTHMC_OK, "a legal call refused");
                }
    if (reduce_walk(4) || reduce_walk(FTHMC_MAX_L)) return 1;
    printf("{\"calls\": %ld, \"refusals\": %ld, \"reductions\": %ld}\n", calls, refusals, reductions);
    return 0;
}
