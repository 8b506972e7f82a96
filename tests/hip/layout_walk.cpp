// Stand-alone walk of the three workspace layouts of csrc/api_call.h (ws_layout, vjp_layout, force_layout) under
// AddressSanitizer + UBSan with the unsigned-overflow check (csrc/san.mk: san_layout; run by tests/test_ws_sizes.py): over the
// grid of tests/golden/make_ws_sizes.py, with a base pointer (never dereferenced) the regions lie in their documented order,
// 256-byte aligned, each behind the end of the one before, and end inside `total`; with a null base every pointer is null and
// `total` is the same; `total` in bytes is what the public size query answers; at the edge of size_t `total` is the last size
// that fits and 0 beyond it, with no signed or unsigned wrap on the way.  Last line of output: a JSON summary.
#include "api_call.h"

#include <limits.h>
#include <stdio.h>

namespace {

long n_layouts = 0, n_regions = 0, n_queries = 0, n_overflows = 0, n_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (n_failed++ < 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

double* const BASE = reinterpret_cast<double*>((uintptr_t)1 << 20);       // 256-byte aligned; no region is ever read or written
struct Shape { FlowArch A; int ia, B, L, nl; bool based; };      // based: small enough for a scratch at BASE to exist

// p[i]: the regions in their documented order, size[i]: doubles region i holds at least (0: not restated here), start: where
// the first one lies
void check_regions(const char* what, const Shape& s, bool with_base, const void* const* p, const size_t* size, int n, size_t start, size_t total) {
    ++n_layouts;
    size_t end = start;
    for (int i = 0; i < n; ++i, ++n_regions) {
        if (!with_base) { CHECK(p[i] == nullptr, "%s arch %d B %d L %d nl %d region %d", what, s.ia, s.B, s.L, s.nl, i); continue; }
        const size_t o = (size_t)(static_cast<const double*>(p[i]) - BASE);
        CHECK(p[i] && o % ALIGN == 0 && o >= end && (i > 0 || o == start), "%s arch %d B %d L %d nl %d region %d at %zu, end of the last %zu",
              what, s.ia, s.B, s.L, s.nl, i, o, end);
        end = o + size[i];
    }
    CHECK(total % ALIGN == 0 && total >= end && total > 0, "%s arch %d B %d L %d nl %d total %zu end %zu", what, s.ia, s.B, s.L, s.nl, total, end);
}

// a carver over a scratch of `total` doubles at BASE (as a caller with exactly the queried size has it), or the sizing one
Carver carver(bool with_base, size_t total) { return with_base ? Carver(BASE, total * sizeof(double)) : Carver(); }

size_t check_ws(const Shape& s, bool train, bool with_base, const WS& w) {
    const size_t n1 = (size_t)s.B * s.L * s.L, n2 = 2 * n1;
    const void* p[] = {w.wint, w.X, w.gp, w.gp2, w.gp_part, w.lj_part, w.scal, w.act_part, w.xa, w.va, w.xb, w.vb, w.gw_part, w.gw_tmp,
                       w.stash, w.gz, w.hbuf, w.gbuf};
    const size_t size[] = {(size_t)FLOW_WHEAD_LAYERS * FLOW_WINT, (size_t)s.nl * n2, n1, s.nl > 0 ? n1 : 0, 0, 0, (size_t)SC_N * s.B,
                           (size_t)32 * s.B, n2, n2, n2, n2, w.gw_rows * FLOW_GW_STRIDE, w.gw_tmp_rows * FLOW_GW_STRIDE, 0, 0, 0, 0};
    check_regions(train ? "train_ws" : "ws", s, with_base, p, size, 18, 0, w.total);
    CHECK(w.n2 == n2, "n2");
    return w.total;
}
size_t check_vjp(const char* what, const Shape& s, bool with_base, const VWS& v, size_t start) {
    const size_t n1 = (size_t)s.B * s.L * s.L, n2 = 2 * n1;
    const void* p[] = {v.xd, v.X, v.stash, v.hbuf, v.gbuf, v.gp, v.gp2, v.gw, v.glj};
    const size_t size[] = {2 * n2, 2 * (size_t)s.nl * n2, 0, 0, 0, 2 * n1, 2 * n1, 2 * (size_t)s.nl * s.A.params(), (size_t)s.B};
    check_regions(what, s, with_base, p, size, 9, start, v.total);
    return v.total;
}
// each layout twice: sized with a null base, then carved in a scratch of exactly that size
size_t walk_ws(const Shape& s, bool train) {
    size_t total[2] = {0, 0};
    for (int with_base = 0; with_base <= (s.based ? 1 : 0); ++with_base) {
        Carver c = carver(with_base, total[0]);
        total[with_base] = check_ws(s, train, with_base, ws_layout(s.A, c, s.B, s.L, s.nl, train));
    }
    CHECK(total[0] == total[1] || !s.based, "ws, null base: arch %d B %d L %d nl %d", s.ia, s.B, s.L, s.nl);
    // a scratch of half the size: the same total, and no pointer behind the scratch's end
    if (!s.based) return total[0];
    Carver c = carver(true, total[0] / 2);
    const WS w = ws_layout(s.A, c, s.B, s.L, s.nl, train);
    CHECK(w.total == total[0] && w.wint == BASE && (!w.gbuf || (size_t)(w.gbuf - BASE) <= total[0] / 2), "ws, short scratch: arch %d B %d L %d nl %d", s.ia, s.B, s.L, s.nl);
    return total[0];
}
size_t walk_vjp(const Shape& s) {
    size_t total[2] = {0, 0};
    for (int with_base = 0; with_base <= (s.based ? 1 : 0); ++with_base) {
        Carver c = carver(with_base, total[0]);
        total[with_base] = check_vjp("vjp", s, with_base, vjp_layout(s.A, c, s.B, s.L, s.nl), Carver().up((size_t)FLOW_WHEAD_LAYERS * FLOW_WINT));
    }
    CHECK(total[0] == total[1] || !s.based, "vjp, null base: arch %d B %d L %d nl %d", s.ia, s.B, s.L, s.nl);
    return total[0];
}
size_t walk_force(const Shape& s, int tile, size_t ws_total) {
    const size_t n1 = (size_t)s.B * s.L * s.L, n2 = 2 * n1;
    size_t total[2] = {0, 0};
    for (int with_base = 0; with_base <= (s.based ? 1 : 0); ++with_base) {
        Carver c = carver(with_base, total[0]), c0 = c;
        const FWS w = force_layout(s.A, c, s.B, s.L, s.nl, tile);
        total[with_base] = w.total;
        CHECK(w.first == ws_total && w.first == check_ws(s, false, with_base, ws_layout(s.A, c0, s.B, s.L, s.nl)), "force: the first-order workspace in front");
        if (tile < 0) {
            const void* p[] = {w.F};
            const size_t size[] = {n2};
            check_regions("force F", s, with_base, p, size, 1, w.first, w.total);
            check_vjp("force plain", s, with_base, w.V, w.first + Carver().up(n2));
            continue;
        }
        const void* p[] = {w.F, w.xd, w.X, w.gp, w.gpp, w.gwp, w.gwt};
        const size_t size[] = {n2, 2 * n2, 2 * (size_t)s.nl * n2, 2 * n1, 0, 0, s.nl > 0 ? (size_t)FLOW_REDUCE_GROUPS * FLOW_GW_STRIDE : 0};
        check_regions("force fused", s, with_base, p, size, 7, w.first, w.total);
    }
    CHECK(total[0] == total[1] || !s.based, "force tile %d, null base: arch %d B %d L %d nl %d", tile, s.ia, s.B, s.L, s.nl);
    return total[0];
}

// every layout of a shape against the public queries
void walk_shape(const Shape& s, const fthmc_arch_t* arch) {
    const size_t ws = walk_ws(s, false), tws = walk_ws(s, true), vws = walk_vjp(s);
    const bool second = !bad_shape(s.B, s.L) && pad_fits(s.A, s.L, s.nl);          // what the second-order queries refuse first
    CHECK(fthmc_ws_bytes(arch, s.B, s.L, s.nl) == ws * 8 && fthmc_train_ws_bytes(arch, s.B, s.L, s.nl) == tws * 8 &&
          fthmc_vjp_ws_bytes(arch, s.B, s.L, s.nl) == (second ? vws * 8 : 0), "queries: arch %d B %d L %d nl %d", s.ia, s.B, s.L, s.nl);
    n_queries += 3;
    for (int tile = -1; tile <= 1; ++tile) {
        if (tile >= 0 && !(s.A.is_default() && flow_dual_shape(s.B, s.L, tile))) continue;
        const size_t fws = walk_force(s, tile, ws);
        for (int path = 0; path <= 3; ++path) {
            if (force_dual_tile(s.A, s.B, s.L, path) != tile) continue;
            fthmc_set_dual_path(path);
            CHECK(fthmc_train_force_ws_bytes(arch, s.B, s.L, s.nl) == (second ? fws * 8 : 0), "force query, path %d: arch %d B %d L %d nl %d",
                  path, s.ia, s.B, s.L, s.nl);
            ++n_queries;
        }
    }
    fthmc_set_dual_path(1);
}

// no layout: total = 0 from all three, whatever the base
void walk_refused(const Shape& s, const fthmc_arch_t* arch) {
    for (int with_base = 0; with_base <= 1; ++with_base) {
        Carver c[6];
        if (with_base) for (Carver& k : c) k = Carver(BASE, (size_t)1 << 40);
        const size_t t[] = {ws_layout(s.A, c[0], s.B, s.L, s.nl).total, ws_layout(s.A, c[1], s.B, s.L, s.nl, true).total,
                            vjp_layout(s.A, c[2], s.B, s.L, s.nl).total, force_layout(s.A, c[3], s.B, s.L, s.nl, -1).total,
                            force_layout(s.A, c[4], s.B, s.L, s.nl, 0).total, force_layout(s.A, c[5], s.B, s.L, s.nl, 1).total};
        for (size_t v : t) CHECK(v == 0, "beyond the edge: arch %d B %d L %d nl %d answers %zu", s.ia, s.B, s.L, s.nl, v);
    }
    CHECK(fthmc_ws_bytes(arch, s.B, s.L, s.nl) == 0 && fthmc_train_ws_bytes(arch, s.B, s.L, s.nl) == 0 && fthmc_vjp_ws_bytes(arch, s.B, s.L, s.nl) == 0 &&
          fthmc_train_force_ws_bytes(arch, s.B, s.L, s.nl) == 0, "queries beyond the edge: arch %d B %d L %d nl %d", s.ia, s.B, s.L, s.nl);
    n_queries += 4;
    ++n_overflows;
}

}  // namespace

int main() {
    // the default net and the net shapes of tests/net_shape_cases.py
    const fthmc_arch_t archs[] = {{2, {8, 8}, 3, 2, 0},   {1, {4}, 9, 2, 0},         {0, {0}, 5, 2, 0},  {1, {3}, 15, 3, 0},
                                  {2, {8, 8}, 1, 2, 0},   {2, {256, 256}, 3, 2, 0},  {1, {1}, 3, 64, 0}, {3, {3, 17, 2}, 3, 1, 0},
                                  {8, {2, 2, 2, 2, 2, 2, 2, 2}, 3, 2, 0}, {1, {5}, 5, 3, 1}, {1, {6}, 7, 2, 0}, {1, {32}, 3, 2, 0}};
    const int Bs[] = {1, 3, 64, 65, 1 << 20}, Ls[] = {4, 8, 16, 20, 64, 68, 132, 256}, nls[] = {0, 1, 8, 64, 65, 66};
    // shapes no layout holds: sizes beyond size_t inside the limits of the ABI, B or L beyond those limits, non-positive counts
    const int edge[][3] = {{FTHMC_MAX_B, FTHMC_MAX_L, 64}, {1 << 20, FTHMC_MAX_L, 1 << 20}, {1, FTHMC_MAX_L, INT_MAX}, {FTHMC_MAX_B, 64, INT_MAX},
                           {FTHMC_MAX_B, FTHMC_MAX_L, INT_MAX}, {FTHMC_MAX_B + 1, 8, 1}, {1, FTHMC_MAX_L + 4, 1}, {INT_MAX, INT_MAX, INT_MAX},
                           {INT_MAX, 4, 0}, {1, INT_MAX, 0}, {0, 8, 1}, {1, 0, 1}, {1, 8, -1}, {-1, -4, 1}};
    for (int ia = 0; ia < 12; ++ia) {
        const fthmc_arch_t* arch = ia == 0 ? nullptr : &archs[ia];
        Shape s{};
        s.ia = ia;
        if (make_flow_arch(archs[ia].n_hidden, archs[ia].hidden, archs[ia].kernel_size, archs[ia].n_mix, archs[ia].final_tanh, &s.A) != FTHMC_OK ||
            s.A.is_default() != (ia == 0)) { printf("arch %d refused\n", ia); return 1; }
        s.based = true;
        for (int B : Bs) for (int L : Ls) for (int nl : nls) { s.B = B; s.L = L; s.nl = nl; walk_shape(s, arch); }
        for (const int* e : edge) { s.B = e[0]; s.L = e[1]; s.nl = e[2]; walk_refused(s, arch); }
        // the edge itself: the deepest flow whose layouts fit size_t at 2^20 chains (64 of the largest lattice), by bisection over
        // the layer count; one layer more and the largest of the layouts, force training's, has none
        for (int L : {64, 256, FTHMC_MAX_L}) {
            s.B = L == FTHMC_MAX_L ? 64 : 1 << 20; s.L = L;                // one layer fits for every net shape of the list
            int lo = 1, hi = INT_MAX;                                  // lo fits, hi does not
            auto fits = [&](int nl) { Carver c; return force_layout(s.A, c, s.B, s.L, nl, -1).total != 0; };
            while (hi - lo > 1) {
                const int mid = lo + (hi - lo) / 2;
                if (fits(mid)) lo = mid; else hi = mid;
            }
            s.based = false;                                           // 2^64 bytes at BASE would wrap the address space: sized only
            s.nl = lo; walk_shape(s, arch);                            // every layout fits here (force_layout holds the other two)
            CHECK(fits(lo) && !fits(hi) && fthmc_train_force_ws_bytes(arch, s.B, s.L, hi) == 0, "the edge: arch %d L %d nl %d", ia, L, lo);
            ++n_overflows;
        }
    }
    printf("{\"layouts\": %ld, \"regions\": %ld, \"queries\": %ld, \"overflows\": %ld, \"failed\": %ld}\n", n_layouts, n_regions, n_queries,
           n_overflows, n_failed);
    return n_failed ? 1 : 0;
}
