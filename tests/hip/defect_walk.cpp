// Stand-alone walk of the boundary-condition tempering entry points (fthmc_defect_ws_bytes, fthmc_defect_trajectory, fthmc_defect_force,
// fthmc_defect_action, fthmc_defect_translate) for tests/test_defect.py: built with AddressSanitizer + UBSan by `make -f san.mk san_defect`
// against the host-side sanitizer build of the library (launches are no-ops there) and run as a program of its own.  Every refusal the
// header lists and their precedence, the workspace rule, legal calls on every path and at the edges of the defect's arguments (Ld = 0
// and L, B = 1 and 65535) from the smallest to the largest shapes.  Device pointers are never dereferenced by the host side: stand-in
// addresses.
#include "walk.h"

#include <math.h>

struct Call {
    int B = 4, L = 8, nstep = 2, integrator = 0, path = 1, i0 = 1, j0 = 2, Ld = 3, top = 3;
    double beta = 2.0;
    bool null_x = false, null_v = false, null_u = false, null_out = false, null_g = false, alias = false, outs = false, null_ws = false,
         null_rung = false, null_shift = false;
    long long ws_short = 0;                       // bytes taken off the workspace size the library asks for
    int trajectory() const {
        const size_t need = fthmc_defect_ws_bytes(B, L, path);
        return fthmc_defect_trajectory(null_x ? NULL : dev(0), null_v ? NULL : dev(1), null_u ? NULL : dev(2), B, L, beta, null_g ? NULL : dev(3),
                                       i0, j0, Ld, 0.1, nstep, integrator, path, null_out ? NULL : (alias ? dev(0) : dev(4)),
                                       outs ? dev(5) : NULL, outs ? dev(6) : NULL, outs ? dev(7) : NULL, outs ? dev(8) : NULL,
                                       outs ? dev(9) : NULL, outs ? dev(10) : NULL, outs ? dev(11) : NULL, null_ws ? NULL : wsp(),
                                       need - (size_t)ws_short, NULL);
    }
    int force() const {
        return fthmc_defect_force(null_x ? NULL : dev(0), B, L, beta, null_g ? NULL : dev(3), i0, j0, Ld, null_out ? NULL : dev(4), NULL);
    }
    int action() const {
        return fthmc_defect_action(null_x ? NULL : dev(0), B, L, beta, null_g ? NULL : dev(3), i0, j0, Ld, outs ? dev(5) : NULL,
                                   outs ? dev(6) : NULL, outs ? dev(7) : NULL, outs ? dev(8) : NULL, NULL);
    }
    int translate() const {
        return fthmc_defect_translate(null_x ? NULL : dev(0), B, L, null_rung ? NULL : ints(0), top, null_shift ? NULL : ints(1),
                                      null_out ? NULL : (alias ? dev(0) : dev(4)), NULL);
    }
    int run(int entry) const { return entry == 0 ? trajectory() : (entry == 1 ? force() : (entry == 2 ? action() : translate())); }
};
static const char* const ENTRY[4] = {"fthmc_defect_trajectory", "fthmc_defect_force", "fthmc_defect_action", "fthmc_defect_translate"};

static int want(const Call& c, int entry, int code, const char* what) {
    const int rc = c.run(entry);
    if (answered(rc, code)) return 0;
    fprintf(stderr, "defect_walk: %s: %s (B %d, L %d, defect (%d, %d, %d), beta %g, nstep %d, integrator %d, path %d) -> %d, expected %d\n",
            ENTRY[entry], what, c.B, c.L, c.i0, c.j0, c.Ld, c.beta, c.nstep, c.integrator, c.path, rc, code);
    return 1;
}

int main() {
    const double inf = INFINITY, nan_ = NAN;
    const int imin = -2147483647 - 1, imax = 2147483647;
    for (int e = 0; e < 4; ++e) {
        // ---- the refusals every entry point shares
        { Call c; c.null_x = true; WANT(c, e, FTHMC_ERR_ARG, "a null x not refused"); }
        const int badB[4] = {-1, 0, FTHMC_MAX_B + 1, imax};
        for (int k = 0; k < 4; ++k) { Call c; c.B = badB[k]; WANT(c, e, FTHMC_ERR_ARG, "B out of range not refused"); }
        const int badL[11] = {-4, 0, 1, 2, 3, 5, 6, 7, 10, FTHMC_MAX_L + 4, 2147483644};
        for (int k = 0; k < 11; ++k) { Call c; c.L = badL[k]; c.i0 = c.j0 = c.Ld = 0; WANT(c, e, FTHMC_ERR_ARG, "L out of range not refused"); }
        if (e == 3) continue;
        // ---- the defect and the couplings
        { Call c; c.null_g = true; WANT(c, e, FTHMC_ERR_ARG, "a null g_b not refused"); }
        const int badLd[5] = {-1, 9, imax, imin, 65536};
        for (int k = 0; k < 5; ++k) { Call c; c.Ld = badLd[k]; WANT(c, e, FTHMC_ERR_ARG, "Ld outside [0, L] not refused"); }
        const int badI[5] = {-1, 8, imax, imin, 9};
        for (int k = 0; k < 5; ++k) {
            { Call c; c.i0 = badI[k]; WANT(c, e, FTHMC_ERR_ARG, "i0 outside [0, L) not refused"); }
            { Call c; c.j0 = badI[k]; WANT(c, e, FTHMC_ERR_ARG, "j0 outside [0, L) not refused"); }
        }
        const double badBeta[3] = {inf, -inf, nan_};
        for (int k = 0; k < 3; ++k) { Call c; c.beta = badBeta[k]; WANT(c, e, FTHMC_ERR_ARG, "a beta that is not finite not refused"); }
        // ---- the legal edges of the defect
        { Call c; c.Ld = 0; WANT(c, e, FTHMC_OK, "Ld = 0 refused"); }
        { Call c; c.Ld = 8; WANT(c, e, FTHMC_OK, "Ld = L refused"); }
        { Call c; c.i0 = 7; c.j0 = 7; c.Ld = 4; WANT(c, e, FTHMC_OK, "a row that wraps refused"); }
        { Call c; c.i0 = 0; c.j0 = 0; WANT(c, e, FTHMC_OK, "i0 = j0 = 0 refused"); }
        { Call c; c.beta = 0.0; WANT(c, e, FTHMC_OK, "beta = 0 refused"); }
        { Call c; c.outs = true; WANT(c, e, FTHMC_OK, "the optional outputs refused"); }
    }
    { Call c; c.null_out = true; WANT(c, 1, FTHMC_ERR_ARG, "a null F not refused"); }
    // ---- the translation's own
    { Call c; c.null_out = true; WANT(c, 3, FTHMC_ERR_ARG, "a null x_out not refused"); }
    { Call c; c.alias = true; WANT(c, 3, FTHMC_ERR_ARG, "x_out == x not refused"); }
    { Call c; c.null_rung = true; WANT(c, 3, FTHMC_ERR_ARG, "a null rung not refused"); }
    { Call c; c.null_shift = true; WANT(c, 3, FTHMC_ERR_ARG, "a null shift not refused"); }
    const int tops[5] = {0, 3, -1, imax, imin};                   // any rung may be named: one no chain sits on translates nothing
    for (int k = 0; k < 5; ++k) { Call c; c.top = tops[k]; WANT(c, 3, FTHMC_OK, "a legal translation refused"); }
    // ---- the trajectory's own
    for (int path = 0; path <= 2; ++path) {
        { Call c; c.path = path; c.null_v = true; WANT(c, 0, FTHMC_ERR_ARG, "a null v not refused"); }
        { Call c; c.path = path; c.null_u = true; WANT(c, 0, FTHMC_ERR_ARG, "a null u not refused"); }
        { Call c; c.path = path; c.null_out = true; WANT(c, 0, FTHMC_ERR_ARG, "a null x_new not refused"); }
        const int badN[4] = {0, -1, imin, -7};
        for (int k = 0; k < 4; ++k) { Call c; c.path = path; c.nstep = badN[k]; WANT(c, 0, FTHMC_ERR_ARG, "nstep < 1 not refused"); }
        const int badInt[4] = {3, -1, 255, imax};
        for (int k = 0; k < 4; ++k) {
            Call c; c.path = path; c.integrator = badInt[k]; WANT(c, 0, FTHMC_ERR_UNSUPPORTED, "an unknown integrator not refused");
            c.nstep = 0; WANT(c, 0, FTHMC_ERR_ARG, "the arguments do not come before the integrator");
            c.nstep = 2; c.Ld = 9; WANT(c, 0, FTHMC_ERR_ARG, "the defect does not come before the integrator");
            c.Ld = 3; c.null_ws = true; WANT(c, 0, FTHMC_ERR_UNSUPPORTED, "the integrator does not come before the workspace");
        }
        // a step count whose stage count leaves int: refused as an argument
        { Call c; c.path = path; c.integrator = 2; c.nstep = imax; WANT(c, 0, FTHMC_ERR_ARG, "a stage count beyond int not refused"); }
    }
    const int badP[5] = {-1, 3, 255, imax, imin};
    for (int k = 0; k < 5; ++k) { Call c; c.path = badP[k]; WANT(c, 0, FTHMC_ERR_ARG, "path outside 0 .. 2 not refused"); }
    { Call c; c.path = 1; c.L = 68; WANT(c, 0, FTHMC_ERR_ARG, "path 1 at L > 64 not refused"); }
    { Call c; c.path = 1; c.alias = true; WANT(c, 0, FTHMC_ERR_ARG, "path 1 with x_new == x not refused"); }
    // ---- the workspace rule (sizes are multiples of 256 bytes, like every workspace size of the header)
    if (fthmc_defect_ws_bytes(4, 8, 1) != 0 || fthmc_defect_ws_bytes(4, 128, 1) != 0 || fthmc_defect_ws_bytes(4, 8, 0) == 0 ||
        fthmc_defect_ws_bytes(4, 8, 0) != fthmc_defect_ws_bytes(4, 8, 2) || fthmc_defect_ws_bytes(4, 8, 2) % 256 != 0 ||
        fthmc_defect_ws_bytes(4, 8, 2) <= fthmc_ws_bytes(NULL, 4, 8, 0) || fthmc_defect_ws_bytes(0, 8, 2) != 0 || fthmc_defect_ws_bytes(2, 6, 2) != 0 ||
        fthmc_defect_ws_bytes(2, 8, 3) != 0 || fthmc_defect_ws_bytes(2, 8, -1) != 0 || fthmc_defect_ws_bytes(65535, FTHMC_MAX_L, 2) == 0 ||
        fthmc_defect_ws_bytes(1, FTHMC_MAX_L, 2) == 0 || fthmc_defect_ws_bytes(65536, 4, 2) != 0 || fthmc_defect_ws_bytes(FTHMC_MAX_B, 4, 0) != 0) {
        fprintf(stderr, "defect_walk: fthmc_defect_ws_bytes\n");
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
    // ---- legal calls: every path and the library's choice, every integrator, aliased and not, optional outputs, Ld = 0 and L, the shapes
    // where the launch geometry changes
    const int Ls[10] = {4, 8, 12, 20, 28, 32, 64, 68, 128, FTHMC_MAX_L};
    const int Bs[6] = {1, 63, 130, 65535, 66000, FTHMC_MAX_B};
    for (int li = 0; li < 10; ++li)
        for (int bi = 0; bi < 6; ++bi) {
            for (int v = 0; v < 4; ++v)
                for (int path = 0; path <= 2; ++path) {
                    Call c; c.L = Ls[li]; c.B = Bs[bi]; c.path = path; c.integrator = v % 3; c.nstep = 1 + v; c.outs = v & 1;
                    c.Ld = v == 0 ? 0 : (v == 1 ? c.L : (v == 2 ? 1 : 4));
                    c.i0 = v == 3 ? c.L - 2 : 0; c.j0 = (v & 1) ? c.L - 1 : 0;
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
                    if (path == 0) {
                        c.alias = false;
                        WANT(c, 1, FTHMC_OK, "a legal force call refused"); WANT(c, 2, FTHMC_OK, "a legal action call refused");
                        c.top = v; WANT(c, 3, FTHMC_OK, "a legal translation refused");
                    }
                }
        }
    return walked();
}
