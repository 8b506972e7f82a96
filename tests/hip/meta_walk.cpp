// Stand-alone walk of the metadynamics entry points (fthmc_meta_ws_bytes, fthmc_meta_trajectory, fthmc_meta_deposit, fthmc_meta_force,
// fthmc_meta_action) for tests/test_meta.py: built with AddressSanitizer + UBSan by `make -f san.mk san_meta` against the host-side
// sanitizer build of the library (launches are no-ops there) and run as a program of its own.  Every refusal the header lists and
// their precedence, the workspace rule, legal calls on both paths and the library's choice from the smallest to the largest shapes
// and at the edges of the table's arguments.  Device pointers are never dereferenced by the host side: stand-in addresses.
#include "walk.h"

#include <math.h>

struct Call {
    int B = 4, L = 8, nstep = 2, integrator = 0, G = 2, nb = 11, path = 1;
    double qmax = 2.0, wall = 1.0, w = 0.1;
    bool null_x = false, null_v = false, null_u = false, null_out = false, null_tab = false, alias = false, outs = false, null_ws = false;
    long long ws_short = 0;                       // bytes taken off the workspace size the library asks for
    int trajectory() const {
        const size_t need = fthmc_meta_ws_bytes(B, L, path);
        return fthmc_meta_trajectory(null_x ? NULL : dev(0), null_v ? NULL : dev(1), null_u ? NULL : dev(2), B, L, 2.0, 0.1, nstep, integrator,
                                     null_tab ? NULL : dev(3), G, nb, qmax, wall, path, null_out ? NULL : (alias ? dev(0) : dev(4)),
                                     outs ? dev(5) : NULL, outs ? dev(6) : NULL, outs ? dev(7) : NULL, outs ? dev(8) : NULL,
                                     outs ? dev(9) : NULL, outs ? dev(10) : NULL, null_ws ? NULL : wsp(), need - (size_t)ws_short, NULL);
    }
    int deposit() const { return fthmc_meta_deposit(null_x ? NULL : dev(0), B, G, nb, qmax, w, null_tab ? NULL : dev(3), NULL); }
    int force() const { return fthmc_meta_force(null_x ? NULL : dev(0), B, L, 2.0, null_tab ? NULL : dev(3), G, nb, qmax, wall, null_out ? NULL : dev(4), NULL); }
    int action() const {
        return fthmc_meta_action(null_x ? NULL : dev(0), B, L, 2.0, null_tab ? NULL : dev(3), G, nb, qmax, wall, outs ? dev(5) : NULL,
                                 outs ? dev(6) : NULL, outs ? dev(7) : NULL, NULL);
    }
    int run(int entry) const { return entry == 0 ? trajectory() : (entry == 1 ? deposit() : (entry == 2 ? force() : action())); }
};
static const char* const ENTRY[4] = {"fthmc_meta_trajectory", "fthmc_meta_deposit", "fthmc_meta_force", "fthmc_meta_action"};

static int want(const Call& c, int entry, int code, const char* what) {
    const int rc = c.run(entry);
    if (answered(rc, code)) return 0;
    fprintf(stderr, "meta_walk: %s: %s (B %d, L %d, G %d, nb %d, qmax %g, wall %g, w %g, nstep %d, integrator %d, path %d) -> %d, expected %d\n",
            ENTRY[entry], what, c.B, c.L, c.G, c.nb, c.qmax, c.wall, c.w, c.nstep, c.integrator, c.path, rc, code);
    return 1;
}

int main() {
    const double inf = INFINITY, nan_ = NAN;
    for (int e = 0; e < 4; ++e) {
        // ---- the refusals every entry point shares
        { Call c; c.null_x = true; WANT(c, e, FTHMC_ERR_ARG, "a null x / qm not refused"); }
        { Call c; c.null_tab = true; WANT(c, e, FTHMC_ERR_ARG, "a null table not refused"); }
        const int badB[4] = {-1, 0, FTHMC_MAX_B + 1, 2147483647};
        for (int k = 0; k < 4; ++k) { Call c; c.B = badB[k]; c.G = 1; WANT(c, e, FTHMC_ERR_ARG, "B out of range not refused"); }
        const int badG[6] = {0, -1, 3, 8, 2147483647, -2147483647 - 1};
        for (int k = 0; k < 6; ++k) { Call c; c.G = badG[k]; WANT(c, e, FTHMC_ERR_ARG, "G < 1 or B % G != 0 not refused"); }
        const int badNb[6] = {1, 0, -1, 65537, 2147483647, -2147483647 - 1};
        for (int k = 0; k < 6; ++k) { Call c; c.nb = badNb[k]; WANT(c, e, FTHMC_ERR_ARG, "nb outside 2 .. 65536 not refused"); }
        const double badQ[6] = {0.0, -0.0, -2.0, inf, -inf, nan_};
        for (int k = 0; k < 6; ++k) { Call c; c.qmax = badQ[k]; WANT(c, e, FTHMC_ERR_ARG, "a qmax that is not finite and positive not refused"); }
        const double badW[4] = {-1.0, -1e-300, inf, nan_};
        for (int k = 0; k < 4; ++k) { Call c; c.wall = badW[k]; c.w = badW[k]; WANT(c, e, FTHMC_ERR_ARG, "a wall / w that is not finite and >= 0 not refused"); }
        if (e != 1) {
            const int badL[11] = {-4, 0, 1, 2, 3, 5, 6, 7, 10, FTHMC_MAX_L + 4, 2147483644};
            for (int k = 0; k < 11; ++k) { Call c; c.L = badL[k]; WANT(c, e, FTHMC_ERR_ARG, "L out of range not refused"); }
        }
        // ---- the legal edges of the table's arguments
        { Call c; c.nb = 2; WANT(c, e, FTHMC_OK, "nb = 2 refused"); }
        { Call c; c.nb = 65536; WANT(c, e, FTHMC_OK, "nb = 65536 refused"); }
        { Call c; c.G = 1; WANT(c, e, FTHMC_OK, "G = 1 refused"); }
        { Call c; c.G = 4; WANT(c, e, FTHMC_OK, "G = B refused"); }
        { Call c; c.wall = 0.0; c.w = 0.0; WANT(c, e, FTHMC_OK, "wall = 0 / w = 0 refused"); }
        { Call c; c.qmax = 1e-300; WANT(c, e, FTHMC_OK, "a tiny qmax refused"); }
        { Call c; c.qmax = 1e300; WANT(c, e, FTHMC_OK, "a huge qmax refused"); }
        { Call c; c.outs = true; WANT(c, e, FTHMC_OK, "the optional outputs refused"); }
    }
    { Call c; c.null_out = true; WANT(c, 2, FTHMC_ERR_ARG, "a null F not refused"); }
    // ---- the trajectory's own
    for (int path = 0; path <= 2; ++path) {
        { Call c; c.path = path; c.null_v = true; WANT(c, 0, FTHMC_ERR_ARG, "a null v not refused"); }
        { Call c; c.path = path; c.null_u = true; WANT(c, 0, FTHMC_ERR_ARG, "a null u not refused"); }
        { Call c; c.path = path; c.null_out = true; WANT(c, 0, FTHMC_ERR_ARG, "a null x_new not refused"); }
        const int badN[4] = {0, -1, -2147483647 - 1, -7};
        for (int k = 0; k < 4; ++k) { Call c; c.path = path; c.nstep = badN[k]; WANT(c, 0, FTHMC_ERR_ARG, "nstep < 1 not refused"); }
        const int badI[4] = {3, -1, 255, 2147483647};
        for (int k = 0; k < 4; ++k) {
            Call c; c.path = path; c.integrator = badI[k]; WANT(c, 0, FTHMC_ERR_UNSUPPORTED, "an unknown integrator not refused");
            c.nstep = 0; WANT(c, 0, FTHMC_ERR_ARG, "the arguments do not come before the integrator");
            c.nstep = 2; c.null_ws = true; WANT(c, 0, FTHMC_ERR_UNSUPPORTED, "the integrator does not come before the workspace");
        }
        // a step count whose stage count leaves int: refused as an argument
        { Call c; c.path = path; c.integrator = 2; c.nstep = 2147483647; WANT(c, 0, FTHMC_ERR_ARG, "a stage count beyond int not refused"); }
    }
    const int badP[5] = {-1, 3, 255, 2147483647, -2147483647 - 1};
    for (int k = 0; k < 5; ++k) { Call c; c.path = badP[k]; WANT(c, 0, FTHMC_ERR_ARG, "path outside 0 .. 2 not refused"); }
    { Call c; c.path = 1; c.L = 68; WANT(c, 0, FTHMC_ERR_ARG, "path 1 at L > 64 not refused"); }
    { Call c; c.path = 1; c.alias = true; WANT(c, 0, FTHMC_ERR_ARG, "path 1 with x_new == x not refused"); }
    // ---- the workspace rule (sizes are multiples of 256 bytes, like every workspace size of the header)
    if (fthmc_meta_ws_bytes(4, 8, 1) != 0 || fthmc_meta_ws_bytes(4, 128, 1) != 0 || fthmc_meta_ws_bytes(4, 8, 0) == 0 ||
        fthmc_meta_ws_bytes(4, 8, 0) != fthmc_meta_ws_bytes(4, 8, 2) || fthmc_meta_ws_bytes(4, 8, 2) % 256 != 0 ||
        fthmc_meta_ws_bytes(4, 8, 2) <= fthmc_ws_bytes(NULL, 4, 8, 0) || fthmc_meta_ws_bytes(0, 8, 2) != 0 || fthmc_meta_ws_bytes(2, 6, 2) != 0 ||
        fthmc_meta_ws_bytes(2, 8, 3) != 0 || fthmc_meta_ws_bytes(2, 8, -1) != 0 || fthmc_meta_ws_bytes(65535, FTHMC_MAX_L, 2) == 0 ||
        fthmc_meta_ws_bytes(1, FTHMC_MAX_L, 2) == 0 || fthmc_meta_ws_bytes(65536, 4, 2) != 0 || fthmc_meta_ws_bytes(FTHMC_MAX_B, 4, 0) != 0) {
        fprintf(stderr, "meta_walk: fthmc_meta_ws_bytes\n");
        return 1;
    }
    calls += 14;
    { Call c; c.path = 2; c.null_ws = true; WANT(c, 0, FTHMC_ERR_WS, "a null workspace not refused"); }
    { Call c; c.path = 2; c.ws_short = 1; WANT(c, 0, FTHMC_ERR_WS, "a short workspace not refused"); }
    { Call c; c.path = 2; c.ws_short = 256; WANT(c, 0, FTHMC_ERR_WS, "a workspace one region short not refused"); }
    { Call c; c.path = 0; c.alias = true; c.ws_short = 8; WANT(c, 0, FTHMC_ERR_WS, "a short workspace not refused (path 0, aliased)"); }
    { Call c; c.path = 0; c.L = 68; c.null_ws = true; WANT(c, 0, FTHMC_ERR_WS, "a null workspace not refused (path 0, L > 64)"); }
    { Call c; c.path = 1; c.null_ws = true; WANT(c, 0, FTHMC_OK, "a null workspace refused where none is needed"); }
    { Call c; c.path = 0; c.null_ws = true; WANT(c, 0, FTHMC_OK, "a null workspace refused where none is needed (path 0)"); }
    // ---- legal calls: both paths and the library's choice, every integrator, aliased and not, optional outputs, G = 1 and G = B, the
    // shapes where the launch geometry changes
    const int Ls[10] = {4, 8, 12, 20, 28, 32, 64, 68, 128, FTHMC_MAX_L};
    const int Bs[6] = {1, 63, 130, 65535, 66000, FTHMC_MAX_B};
    for (int li = 0; li < 10; ++li)
        for (int bi = 0; bi < 6; ++bi) {
            for (int v = 0; v < 4; ++v)
                for (int path = 0; path <= 2; ++path) {
                    Call c; c.L = Ls[li]; c.B = Bs[bi]; c.path = path; c.integrator = v % 3; c.nstep = 1 + v; c.outs = v & 1;
                    c.G = (v & 2) ? c.B : 1; c.nb = v == 3 ? 65536 : 41;
                    c.alias = path != 1 && (v & 1);
                    if (path == 1 && c.L > 64) continue;
                    // the sequenced path serves B <= 65535: beyond, unsupported -- behind the arguments, before the workspace
                    const bool seq = path == 2 || (path == 0 && (c.L > 64 || c.alias));
                    if (seq && c.B > 65535) {
                        c.null_ws = true;
                        WANT(c, 0, FTHMC_ERR_UNSUPPORTED, "more chains than the sequenced path serves not refused");
                        c.nstep = 0;
                        WANT(c, 0, FTHMC_ERR_ARG, "the arguments do not come before the sequenced path's chain count");
                        c.nstep = 1; c.null_ws = false;
                    } else WANT(c, 0, FTHMC_OK, "a legal call refused");
                    if (path == 0) { WANT(c, 1, FTHMC_OK, "a legal deposit refused"); WANT(c, 2, FTHMC_OK, "a legal force call refused"); WANT(c, 3, FTHMC_OK, "a legal action call refused"); }
                }
        }
    return walked();
}
