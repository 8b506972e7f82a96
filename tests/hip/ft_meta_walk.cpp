// Stand-alone walk of the metadynamics-through-the-flow entry points (fthmc_ft_meta_ws_bytes, fthmc_ft_meta_trajectory_v,
// fthmc_ft_meta_force_v, fthmc_ft_meta_action_v) for tests/test_ft_meta.py: built with AddressSanitizer + UBSan by
// `make -f san.mk san_ft_meta` against the host-side sanitizer build of the library (launches are no-ops there) and run as a program
// of its own.  Every refusal the header lists and their precedence, the workspace rule, legal calls on every branch of the sequencer
// (small path on and off, the default and a generic net, 0 to 66 layers, G = 1 and B, nb = 2 and 65536, the three integrators, carried
// state and optional outputs) up to the largest shapes.  Device pointers are never dereferenced by the host side: stand-in addresses.
#include "walk.h"

#include <math.h>

static const fthmc_arch_t GEN = {3, {4, 6, 5, 0, 0, 0, 0, 0}, 5, 3, 0};
static const fthmc_arch_t BAD = {9, {4, 4, 4, 4, 4, 4, 4, 4}, 3, 2, 0};                                    // n_hidden > 8

struct Call {
    int B = 4, L = 8, nl = 2, act = 0, nstep = 2, integrator = 0, G = 2, nb = 11;
    double qmax = 2.0, wall = 1.0;
    const fthmc_arch_t* arch = NULL;
    bool null_x = false, null_v = false, null_u = false, null_out = false, null_tab = false, null_w = false, outs = false, null_ws = false,
         state = false;
    long long ws_short = 0;                       // bytes taken off the workspace size the library asks for
    uint64_t wver = 0;
    size_t need() const { return fthmc_ft_meta_ws_bytes(arch, B, L, nl); }
    int trajectory() const {
        return fthmc_ft_meta_trajectory_v(null_x ? NULL : dev(0), null_v ? NULL : dev(1), null_u ? NULL : dev(2), null_w ? NULL : dev(11), arch,
                                          nl, B, L, act, 2.0, 0.1, nstep, integrator, null_tab ? NULL : dev(3), G, nb, qmax, wall,
                                          null_out ? NULL : dev(4), outs ? dev(5) : NULL, outs ? dev(6) : NULL, outs ? dev(7) : NULL,
                                          outs ? dev(8) : NULL, outs ? dev(9) : NULL, outs ? dev(10) : NULL, outs ? dev(12) : NULL,
                                          outs ? dev(13) : NULL, state ? dev(14) : NULL, state ? dev(15) : NULL, null_ws ? NULL : wsp(),
                                          need() - (size_t)ws_short, NULL, wver);
    }
    int force() const {
        return fthmc_ft_meta_force_v(null_x ? NULL : dev(0), null_w ? NULL : dev(11), arch, nl, B, L, act, 2.0, null_tab ? NULL : dev(3), G, nb,
                                     qmax, wall, null_out ? NULL : dev(4), null_ws ? NULL : wsp(), need() - (size_t)ws_short, NULL, wver);
    }
    int action() const {
        return fthmc_ft_meta_action_v(null_x ? NULL : dev(0), null_w ? NULL : dev(11), arch, nl, B, L, act, 2.0, null_tab ? NULL : dev(3), G, nb,
                                      qmax, wall, outs ? dev(5) : NULL, outs ? dev(6) : NULL, outs ? dev(7) : NULL, outs ? dev(8) : NULL,
                                      null_ws ? NULL : wsp(), need() - (size_t)ws_short, NULL, wver);
    }
    int run(int entry) const { return entry == 0 ? trajectory() : (entry == 1 ? force() : action()); }
};
static const char* const ENTRY[3] = {"fthmc_ft_meta_trajectory_v", "fthmc_ft_meta_force_v", "fthmc_ft_meta_action_v"};

static int want(const Call& c, int entry, int code, const char* what) {
    const int rc = c.run(entry);
    if (answered(rc, code)) return 0;
    fprintf(stderr, "ft_meta_walk: %s: %s (B %d, L %d, layers %d, act %d, G %d, nb %d, qmax %g, wall %g, nstep %d, integrator %d, small %d, "
            "arch %s) -> %d, expected %d\n", ENTRY[entry], what, c.B, c.L, c.nl, c.act, c.G, c.nb, c.qmax, c.wall, c.nstep, c.integrator,
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
            { Call c; c.null_tab = true; WANT(c, e, FTHMC_ERR_ARG, "a null table not refused"); }
            { Call c; c.null_w = true; WANT(c, e, FTHMC_ERR_ARG, "null weights with layers not refused"); }
            { Call c; c.nl = -1; WANT(c, e, FTHMC_ERR_ARG, "a negative layer count not refused"); }
            const int badB[4] = {-1, 0, FTHMC_MAX_B + 1, 2147483647};
            for (int k = 0; k < 4; ++k) { Call c; c.B = badB[k]; c.G = 1; WANT(c, e, FTHMC_ERR_ARG, "B out of range not refused"); }
            const int badL[11] = {-4, 0, 1, 2, 3, 5, 6, 7, 10, FTHMC_MAX_L + 4, 2147483644};
            for (int k = 0; k < 11; ++k) { Call c; c.L = badL[k]; WANT(c, e, FTHMC_ERR_ARG, "L out of range not refused"); }
            const int badG[6] = {0, -1, 3, 8, 2147483647, -2147483647 - 1};
            for (int k = 0; k < 6; ++k) { Call c; c.G = badG[k]; WANT(c, e, FTHMC_ERR_ARG, "G < 1 or B % G != 0 not refused"); }
            const int badNb[6] = {1, 0, -1, 65537, 2147483647, -2147483647 - 1};
            for (int k = 0; k < 6; ++k) { Call c; c.nb = badNb[k]; WANT(c, e, FTHMC_ERR_ARG, "nb outside 2 .. 65536 not refused"); }
            const double badQ[6] = {0.0, -0.0, -2.0, inf, -inf, nan_};
            for (int k = 0; k < 6; ++k) { Call c; c.qmax = badQ[k]; WANT(c, e, FTHMC_ERR_ARG, "a qmax that is not finite and positive not refused"); }
            const double badW[4] = {-1.0, -1e-300, inf, nan_};
            for (int k = 0; k < 4; ++k) { Call c; c.wall = badW[k]; WANT(c, e, FTHMC_ERR_ARG, "a wall that is not finite and >= 0 not refused"); }
            // ---- FTHMC_ERR_UNSUPPORTED, behind every FTHMC_ERR_ARG and before the workspace
            const int badA[3] = {-1, 3, 2147483647};
            for (int k = 0; k < 3; ++k) {
                Call c; c.act = badA[k]; c.null_ws = true; WANT(c, e, FTHMC_ERR_UNSUPPORTED, "an unknown activation not refused");
                c.nb = 1; WANT(c, e, FTHMC_ERR_ARG, "the arguments do not come before the activation");
            }
            { Call c; c.arch = &BAD; c.null_ws = true; WANT(c, e, FTHMC_ERR_UNSUPPORTED, "a refused arch not refused");
              c.qmax = nan_; WANT(c, e, FTHMC_ERR_ARG, "the arguments do not come before the arch"); }
            // the sequenced kernels put the chain on grid y: the force and action entry points always, the trajectory where it is sequenced
            { Call c; c.B = 65536; c.G = 1; c.null_ws = true;
              WANT(c, e, (e == 0 && small) ? FTHMC_ERR_WS : FTHMC_ERR_UNSUPPORTED, "more chains than the sequenced kernels serve");
              c.L = 20; WANT(c, e, FTHMC_ERR_UNSUPPORTED, "more chains than the sequenced kernels serve not refused (L = 20)");
              c.wall = -1.0; WANT(c, e, FTHMC_ERR_ARG, "the arguments do not come before the chain count"); }
            // ---- the workspace, behind both
            { Call c; c.null_ws = true; WANT(c, e, FTHMC_ERR_WS, "a null workspace not refused"); }
            { Call c; c.ws_short = 1; WANT(c, e, FTHMC_ERR_WS, "a short workspace not refused"); }
            { Call c; c.ws_short = 256; WANT(c, e, FTHMC_ERR_WS, "a workspace one region short not refused"); }
            { Call c; c.nl = 0; c.null_w = true; c.ws_short = 8; WANT(c, e, FTHMC_ERR_WS, "a short workspace not refused (no layers)"); }
            // ---- the legal edges
            { Call c; c.nb = 2; WANT(c, e, FTHMC_OK, "nb = 2 refused"); }
            { Call c; c.nb = 65536; WANT(c, e, FTHMC_OK, "nb = 65536 refused"); }
            { Call c; c.G = 1; WANT(c, e, FTHMC_OK, "G = 1 refused"); }
            { Call c; c.G = 4; WANT(c, e, FTHMC_OK, "G = B refused"); }
            { Call c; c.wall = 0.0; WANT(c, e, FTHMC_OK, "wall = 0 refused"); }
            { Call c; c.qmax = 1e-300; WANT(c, e, FTHMC_OK, "a tiny qmax refused"); }
            { Call c; c.qmax = 1e300; WANT(c, e, FTHMC_OK, "a huge qmax refused"); }
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
                        c.G = (v & 2) ? c.B : 1; c.nb = v == 3 ? 65536 : (v == 0 ? 2 : 41); c.act = v % 3; c.arch = (v == 1) ? &GEN : NULL;
                        if (c.arch && c.B == 65535 && c.L >= 64) continue;                  // (a generic workspace of terabytes: nothing new to walk)
                        // the tuned kernels address a layer's stash with 32-bit offsets (fthmc_hip.h): B * 35 * L * L < 2^32, refused beyond
                        if (!c.arch && c.nl > 0 && (unsigned long long)c.B * 35ull * c.L * c.L >= (1ull << 32)) continue;
                        for (int e = 0; e < 3; ++e) WANT(c, e, FTHMC_OK, "a legal call refused");
                    }
        // the largest shapes: no layers (the plain kernels' limits) and the one-launch kernel's chain count
        { Call c; c.L = FTHMC_MAX_L; c.B = 1; c.G = 1; c.nl = 0; for (int e = 0; e < 3; ++e) WANT(c, e, FTHMC_OK, "the largest lattice refused"); }
        { Call c; c.L = 4; c.B = 65535; c.G = 65535; c.nl = 0; for (int e = 0; e < 3; ++e) WANT(c, e, FTHMC_OK, "the sequenced kernels' largest batch refused"); }
        { Call c; c.L = 4; c.B = FTHMC_MAX_B; c.G = 1; c.nl = 0; for (int e = 0; e < 3; ++e) WANT(c, e, FTHMC_ERR_UNSUPPORTED, "FTHMC_MAX_B chains on the sequenced kernels not refused"); }
        { Call c; c.L = 8; c.B = 66000; c.G = 66000; c.nl = 2;
          WANT(c, 0, small ? FTHMC_OK : FTHMC_ERR_UNSUPPORTED, "66000 chains: the one-launch kernel takes them, the sequenced kernels do not"); }
    }
    // ---- the workspace rule: fthmc_ws_bytes and the two rows of chain sums behind it, rounded to 256 bytes
    const int shapes[6][3] = {{4, 8, 2}, {3, 20, 2}, {1, 4, 0}, {130, 16, 4}, {65535, 4, 0}, {16, 64, 8}};
    for (int k = 0; k < 6; ++k)
        for (int g = 0; g < 2; ++g) {
            const fthmc_arch_t* a = g ? &GEN : NULL;
            const int B = shapes[k][0], L = shapes[k][1], nl = shapes[k][2];
            const size_t base = fthmc_ws_bytes(a, B, L, nl), rows = ((size_t)2 * B * sizeof(double) + 255) / 256 * 256;
            if (base == 0 || fthmc_ft_meta_ws_bytes(a, B, L, nl) != base + rows || base % 256 != 0) {
                fprintf(stderr, "ft_meta_walk: fthmc_ft_meta_ws_bytes(%s, %d, %d, %d)\n", g ? "generic" : "default", B, L, nl);
                return 1;
            }
            ++calls;
        }
    if (fthmc_ft_meta_ws_bytes(NULL, 0, 8, 2) != 0 || fthmc_ft_meta_ws_bytes(NULL, 4, 0, 2) != 0 || fthmc_ft_meta_ws_bytes(NULL, 4, 8, -1) != 0 ||
        fthmc_ft_meta_ws_bytes(&BAD, 4, 8, 2) != 0) {
        fprintf(stderr, "ft_meta_walk: fthmc_ft_meta_ws_bytes of refused arguments\n");
        return 1;
    }
    calls += 4;
    if (fthmc_set_small_path(1) != FTHMC_OK) return 1;
    return walked();
}
