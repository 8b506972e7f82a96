// Stand-alone walk of the entry points of boundary-condition tempering through the flow (fthmc_ft_defect_ws_bytes,
// fthmc_ft_defect_trajectory_v, fthmc_ft_defect_force_v, fthmc_ft_defect_action_v) for tests/test_ft_defect.py: built with
// AddressSanitizer + UBSan by `make -f san.mk san_ft_defect` against the host-side sanitizer build of the library (launches are no-ops
// there) and run as a program of its own.  Every refusal the header lists and their precedence, the workspace rule, legal calls on
// every branch of the sequencer (small path on and off, the default and a generic net, 0 to 66 layers, every
// edge of the defect, the three integrators, carried state and optional outputs) up to the largest shapes.  Device pointers are never
// dereferenced by the host side: stand-in addresses.
#include "walk.h"

#include <math.h>

static const fthmc_arch_t GEN = {3, {4, 6, 5, 0, 0, 0, 0, 0}, 5, 3, 0};
static const fthmc_arch_t BAD = {9, {4, 4, 4, 4, 4, 4, 4, 4}, 3, 2, 0};                                    // n_hidden > 8

struct Call {
    int B = 4, L = 8, nl = 2, act = 0, nstep = 2, integrator = 0, i0 = 6, j0 = 7, Ld = 4;
    double beta = 2.0;
    const fthmc_arch_t* arch = NULL;
    bool null_x = false, null_v = false, null_u = false, null_out = false, null_g = false, null_w = false, outs = false, null_ws = false,
         state = false;
    long long ws_short = 0;                       // bytes taken off the workspace size the library asks for
    uint64_t wver = 0;
    size_t need() const { return fthmc_ft_defect_ws_bytes(arch, B, L, nl); }
    int trajectory() const {
        return fthmc_ft_defect_trajectory_v(null_x ? NULL : dev(0), null_v ? NULL : dev(1), null_u ? NULL : dev(2), null_w ? NULL : dev(11), arch,
                                            nl, B, L, act, beta, null_g ? NULL : dev(3), i0, j0, Ld, 0.1, nstep, integrator,
                                            null_out ? NULL : dev(4), outs ? dev(5) : NULL, outs ? dev(6) : NULL, outs ? dev(7) : NULL,
                                            outs ? dev(8) : NULL, outs ? dev(9) : NULL, outs ? dev(10) : NULL, outs ? dev(12) : NULL,
                                            state ? dev(14) : NULL, state ? dev(15) : NULL, null_ws ? NULL : wsp(), need() - (size_t)ws_short,
                                            NULL, wver);
    }
    int force() const {
        return fthmc_ft_defect_force_v(null_x ? NULL : dev(0), null_w ? NULL : dev(11), arch, nl, B, L, act, beta, null_g ? NULL : dev(3), i0, j0,
                                       Ld, null_out ? NULL : dev(4), null_ws ? NULL : wsp(), need() - (size_t)ws_short, NULL, wver);
    }
    int action() const {
        return fthmc_ft_defect_action_v(null_x ? NULL : dev(0), null_w ? NULL : dev(11), arch, nl, B, L, act, beta, null_g ? NULL : dev(3), i0, j0,
                                        Ld, outs ? dev(5) : NULL, outs ? dev(6) : NULL, outs ? dev(7) : NULL, outs ? dev(8) : NULL,
                                        outs ? dev(9) : NULL, null_ws ? NULL : wsp(), need() - (size_t)ws_short, NULL, wver);
    }
    int run(int entry) const { return entry == 0 ? trajectory() : (entry == 1 ? force() : action()); }
};
static const char* const ENTRY[3] = {"fthmc_ft_defect_trajectory_v", "fthmc_ft_defect_force_v", "fthmc_ft_defect_action_v"};

static int want(const Call& c, int entry, int code, const char* what) {
    const int rc = c.run(entry);
    if (answered(rc, code)) return 0;
    fprintf(stderr, "ft_defect_walk: %s: %s (B %d, L %d, layers %d, act %d, beta %g, defect (%d, %d, %d), nstep %d, integrator %d, small %d, "
            "arch %s) -> %d, expected %d\n", ENTRY[entry], what, c.B, c.L, c.nl, c.act, c.beta, c.i0, c.j0, c.Ld, c.nstep, c.integrator,
            fthmc_get_small_path(), c.arch == NULL ? "default" : (c.arch == &GEN ? "generic" : "refused"), rc, code);
    return 1;
}

int main() {
    const double inf = INFINITY, nan_ = NAN;
    for (int small = 1; small >= 0; --small) {
        if (fthmc_set_small_path(small) != FTHMC_OK) return 1;
        for (int e = 0; e < 3; ++e) {
            // ---- FTHMC_ERR_ARG
            { Call c; c.null_x = true; WANT(c, e, FTHMC_ERR_ARG, "a null x not refused"); }
            { Call c; c.null_g = true; WANT(c, e, FTHMC_ERR_ARG, "null couplings not refused"); }
            { Call c; c.null_w = true; WANT(c, e, FTHMC_ERR_ARG, "null weights with layers not refused"); }
            { Call c; c.nl = -1; WANT(c, e, FTHMC_ERR_ARG, "a negative layer count not refused"); }
            const int badB[4] = {-1, 0, FTHMC_MAX_B + 1, 2147483647};
            for (int k = 0; k < 4; ++k) { Call c; c.B = badB[k]; WANT(c, e, FTHMC_ERR_ARG, "B out of range not refused"); }
            const int badL[11] = {-4, 0, 1, 2, 3, 5, 6, 7, 10, FTHMC_MAX_L + 4, 2147483644};
            for (int k = 0; k < 11; ++k) { Call c; c.L = badL[k]; c.i0 = c.j0 = 0; c.Ld = 0; WANT(c, e, FTHMC_ERR_ARG, "L out of range not refused"); }
            const int badLd[5] = {-1, 9, 2147483647, -2147483647 - 1, 16};
            for (int k = 0; k < 5; ++k) { Call c; c.Ld = badLd[k]; WANT(c, e, FTHMC_ERR_ARG, "Ld outside [0, L] not refused"); }
            const int badI[5] = {-1, 8, 2147483647, -2147483647 - 1, 9};
            for (int k = 0; k < 5; ++k) {
                { Call c; c.i0 = badI[k]; WANT(c, e, FTHMC_ERR_ARG, "i0 outside [0, L) not refused"); }
                { Call c; c.j0 = badI[k]; WANT(c, e, FTHMC_ERR_ARG, "j0 outside [0, L) not refused"); }
            }
            const double badBeta[3] = {inf, -inf, nan_};
            for (int k = 0; k < 3; ++k) { Call c; c.beta = badBeta[k]; WANT(c, e, FTHMC_ERR_ARG, "a beta that is not finite not refused"); }
            // ---- FTHMC_ERR_UNSUPPORTED, behind every FTHMC_ERR_ARG and before the workspace
            const int badA[3] = {-1, 3, 2147483647};
            for (int k = 0; k < 3; ++k) {
                Call c; c.act = badA[k]; c.null_ws = true; WANT(c, e, FTHMC_ERR_UNSUPPORTED, "an unknown activation not refused");
                c.Ld = 9; WANT(c, e, FTHMC_ERR_ARG, "the arguments do not come before the activation");
            }
            { Call c; c.arch = &BAD; c.null_ws = true; WANT(c, e, FTHMC_ERR_UNSUPPORTED, "a refused arch not refused");
              c.beta = nan_; WANT(c, e, FTHMC_ERR_ARG, "the arguments do not come before the arch"); }
            // the sequenced kernels put the chain on grid y: the force and action entry points always, the trajectory where it is sequenced
            { Call c; c.B = 65536; c.null_ws = true;
              WANT(c, e, (e == 0 && small) ? FTHMC_ERR_WS : FTHMC_ERR_UNSUPPORTED, "more chains than the sequenced kernels serve");
              c.L = 20; WANT(c, e, FTHMC_ERR_UNSUPPORTED, "more chains than the sequenced kernels serve not refused (L = 20)");
              c.j0 = -1; WANT(c, e, FTHMC_ERR_ARG, "the arguments do not come before the chain count"); }
            // ---- the workspace, behind both
            { Call c; c.null_ws = true; WANT(c, e, FTHMC_ERR_WS, "a null workspace not refused"); }
            { Call c; c.ws_short = 1; WANT(c, e, FTHMC_ERR_WS, "a short workspace not refused"); }
            { Call c; c.ws_short = 256; WANT(c, e, FTHMC_ERR_WS, "a workspace one region short not refused"); }
            { Call c; c.nl = 0; c.null_w = true; c.ws_short = 8; WANT(c, e, FTHMC_ERR_WS, "a short workspace not refused (no layers)"); }
            // ---- the legal edges
            { Call c; c.Ld = 0; WANT(c, e, FTHMC_OK, "Ld = 0 refused"); }
            { Call c; c.Ld = 8; WANT(c, e, FTHMC_OK, "Ld = L refused"); }
            { Call c; c.i0 = c.j0 = 0; WANT(c, e, FTHMC_OK, "a defect at the origin refused"); }
            { Call c; c.i0 = c.j0 = 7; c.Ld = 8; WANT(c, e, FTHMC_OK, "a defect that wraps from the last site refused"); }
            { Call c; c.beta = 0.0; WANT(c, e, FTHMC_OK, "beta = 0 refused"); }
            { Call c; c.beta = -1e300; WANT(c, e, FTHMC_OK, "a huge negative beta refused"); }
            { Call c; c.outs = true; c.state = true; c.wver = 77; WANT(c, e, FTHMC_OK, "the optional outputs, the carried state or a weights version refused"); }
            { Call c; c.nl = 0; c.null_w = true; WANT(c, e, FTHMC_OK, "no layers without weights refused"); }
        }
        { Call c; c.null_out = true; WANT(c, 1, FTHMC_ERR_ARG, "a null F not refused"); }
        // ---- the trajectory's own
        { Call c; c.null_v = true; WANT(c, 0, FTHMC_ERR_ARG, "a null v not refused"); }
        { Call c; c.null_u = true; WANT(c, 0, FTHMC_ERR_ARG, "a null u not refused"); }
        { Call c; c.null_out = true; WANT(c, 0, FTHMC_ERR_ARG, "a null x_new not refused"); }
        const int badN[4] = {0, -1, -2147483647 - 1, -7};
        for (int k = 0; k < 4; ++k) { Call c; c.nstep = badN[k]; WANT(c, 0, FTHMC_ERR_ARG, "nstep < 1 not refused"); }
        const int badI[4] = {3, -1, 255, 2147483647};
        for (int k = 0; k < 4; ++k) {
            Call c; c.integrator = badI[k]; WANT(c, 0, FTHMC_ERR_UNSUPPORTED, "an unknown integrator not refused");
            c.nstep = 0; WANT(c, 0, FTHMC_ERR_ARG, "the arguments do not come before the integrator");
            c.nstep = 2; c.null_ws = true; WANT(c, 0, FTHMC_ERR_UNSUPPORTED, "the integrator does not come before the workspace");
        }
        { Call c; c.integrator = 2; c.nstep = 2147483647; WANT(c, 0, FTHMC_ERR_ARG, "a stage count beyond int not refused"); }
        // ---- legal calls on every branch: the one-launch sizes and the tiled ones, ragged, the generic net, 0 .. 66 layers
        const int Ls[8] = {4, 8, 12, 16, 20, 32, 64, 128};
        const int Bs[4] = {1, 3, 130, 65535};
        const int NLs[4] = {0, 1, 8, 66};
        for (int li = 0; li < 8; ++li)
            for (int bi = 0; bi < 4; ++bi)
                for (int ni = 0; ni < 4; ++ni)
                    for (int v = 0; v < 4; ++v) {
                        Call c; c.L = Ls[li]; c.B = Bs[bi]; c.nl = NLs[ni]; c.integrator = v % 3; c.nstep = 1 + v; c.outs = v & 1; c.state = v & 2;
                        c.i0 = v == 0 ? 0 : c.L - 1; c.j0 = v == 3 ? 0 : c.L - 1; c.Ld = v == 0 ? 0 : (v == 1 ? c.L : 3);
                        c.act = v % 3; c.arch = (v == 1) ? &GEN : NULL;
                        if (c.arch && c.B == 65535 && c.L >= 64) continue;                  // (a generic workspace of terabytes: nothing new to walk)
                        // the tuned kernels address a layer's stash with 32-bit offsets (fthmc_hip.h): B * 35 * L * L < 2^32, refused beyond
                        if (!c.arch && c.nl > 0 && (unsigned long long)c.B * 35ull * c.L * c.L >= (1ull << 32)) continue;
                        for (int e = 0; e < 3; ++e) WANT(c, e, FTHMC_OK, "a legal call refused");
                    }
        // the largest shapes: no layers (the plain kernels' limits) and the sequenced kernels' chain count
        { Call c; c.L = FTHMC_MAX_L; c.B = 1; c.nl = 0; c.i0 = c.j0 = FTHMC_MAX_L - 1; c.Ld = FTHMC_MAX_L;
          for (int e = 0; e < 3; ++e) WANT(c, e, FTHMC_OK, "the largest lattice refused"); }
        { Call c; c.L = 4; c.B = 65535; c.nl = 0; c.i0 = c.j0 = 3; for (int e = 0; e < 3; ++e) WANT(c, e, FTHMC_OK, "the sequenced kernels' largest batch refused"); }
        { Call c; c.L = 4; c.B = FTHMC_MAX_B; c.nl = 0; c.i0 = c.j0 = 3; for (int e = 0; e < 3; ++e) WANT(c, e, FTHMC_ERR_UNSUPPORTED, "FTHMC_MAX_B chains on the sequenced kernels not refused"); }
        { Call c; c.L = 8; c.B = 66000; c.nl = 2;
          WANT(c, 0, small ? FTHMC_OK : FTHMC_ERR_UNSUPPORTED, "66000 chains: the one-launch kernel takes them, the sequenced kernels do not"); }
    }
    // ---- the workspace rule: fthmc_ws_bytes and the three rows of chain sums behind it, rounded to 256 bytes
    const int shapes[6][3] = {{4, 8, 2}, {3, 20, 2}, {1, 4, 0}, {130, 16, 4}, {65535, 4, 0}, {16, 64, 8}};
    for (int k = 0; k < 6; ++k)
        for (int g = 0; g < 2; ++g) {
            const fthmc_arch_t* a = g ? &GEN : NULL;
            const int B = shapes[k][0], L = shapes[k][1], nl = shapes[k][2];
            const size_t base = fthmc_ws_bytes(a, B, L, nl), rows = ((size_t)3 * B * sizeof(double) + 255) / 256 * 256;
            if (base == 0 || fthmc_ft_defect_ws_bytes(a, B, L, nl) != base + rows || base % 256 != 0) {
                fprintf(stderr, "ft_defect_walk: fthmc_ft_defect_ws_bytes(%s, %d, %d, %d)\n", g ? "generic" : "default", B, L, nl);
                return 1;
            }
            ++calls;
        }
    if (fthmc_ft_defect_ws_bytes(NULL, 0, 8, 2) != 0 || fthmc_ft_defect_ws_bytes(NULL, 4, 0, 2) != 0 || fthmc_ft_defect_ws_bytes(NULL, 4, 8, -1) != 0 ||
        fthmc_ft_defect_ws_bytes(&BAD, 4, 8, 2) != 0) {
        fprintf(stderr, "ft_defect_walk: fthmc_ft_defect_ws_bytes of refused arguments\n");
        return 1;
    }
    calls += 4;
    if (fthmc_set_small_path(1) != FTHMC_OK) return 1;
    return walked();
}
