// gillespie_mixed.hpp -- the exact event loop for MIXED batches (include/gillespie_mixed.h, include/gillespie_mixed_many.h):
// every system of the launch refers to one of V variants, a variant being an interaction range (its weight table) and a
// blocking table.  Included by gillespie_hip.hip (the batch kernel: gilx_view) and gillespie_big_hip.hip (the large-system
// kernel: gilxm_select); the host code that checks the variants and builds their tables is here once for both.  The device
// code here is instantiated by the kernels that have the compile-time property MX; the others keep the launch-wide values
// of their arguments and are the code they were before it existed.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "gillespie_mixed.h"
#include "aps_common.hpp"

namespace {

struct GilxVariant { int32_t offset, tlen, field_mode, reserved; };   // of one variant: first double of its table, its length, sigma_grid > 0

struct GilxArgs {
    const int32_t *order;              // [n_systems] the system a workgroup takes: a permutation
    const int32_t *variant_of_system;  // [n_systems]
    const GilxVariant *variants;       // [n_variants]; the tables lie back to back in GilArgs::table,
    int has_block;                     //   the blocking tables, (K+1)^2 bytes each, in GilArgs::block_table when has_block
    const uint64_t *seed;              // [n_systems] Philox key of a system
    const int32_t *stream;             // [n_systems] Philox counter word 2 of a system
};

// What one workgroup of a mixed launch runs with: the system's own values, where the other launches read the launch's from
// their arguments.  Without MX nothing is read and the view stays empty.
struct GilxView {
    int sys, tlen, chunk, nslots, field_mode;
    const double *table;
    const uint8_t *block_table;
    uint32_t seed_lo, seed_hi, stream;
};

template <bool MX, int NT, class Args>
__device__ __forceinline__ GilxView gilx_view(const Args &a) {
    GilxView v{};
    if constexpr (MX) {
        v.sys = a.mx.order[blockIdx.x];
        const int n = a.n0[v.sys], K1 = a.m.K + 1;
        const int var = a.mx.variant_of_system[v.sys];
        const GilxVariant gv = a.mx.variants[var];
        v.tlen = gv.tlen; v.field_mode = gv.field_mode; v.table = a.table + gv.offset;
        v.block_table = a.mx.has_block ? a.block_table + (size_t)var * K1 * K1 : nullptr;
        v.nslots = n; v.chunk = (n + NT - 1) / NT;           // the system's own slots: none is added during a run
        const uint64_t key = a.mx.seed[v.sys];
        v.seed_lo = (uint32_t)key; v.seed_hi = (uint32_t)(key >> 32); v.stream = (uint32_t)a.mx.stream[v.sys];
    }
    return v;
}

// The large-system kernel's counterpart: `a` is the workgroup's copy of the arguments, already narrowed to system `sys`
// (select_system); the launch-wide table, its length, whether it lies in LDS (up to tab_lds_max entries), the field mode, the
// blocking table and the Philox key are replaced by the system's own.  Returns the system's stream (Philox counter word 2).
// `sys` is uniform over the workgroup, so every value here is loaded and kept as a scalar.
template <class Args>
__device__ __forceinline__ uint32_t gilxm_select(Args &a, const GilxArgs &mx, int sys, int tab_lds_max) {
    const int var = mx.variant_of_system[sys], K1 = a.m.K + 1;
    const GilxVariant gv = mx.variants[var];
    a.table += gv.offset; a.tlen = gv.tlen; a.tab_in_lds = gv.tlen + 1 <= tab_lds_max ? 1 : 0;
    a.m.field_mode = gv.field_mode;
    a.block_table = mx.has_block ? a.block_table + (size_t)var * K1 * K1 : nullptr;
    const uint64_t key = mx.seed[sys];
    a.m.seed_lo = (uint32_t)key; a.m.seed_hi = (uint32_t)(key >> 32);
    return (uint32_t)mx.stream[sys];
}

// ---- host side, shared by gilx_decide (gillespie_hip.hip) and gilxm_decide (gillespie_big_hip.hip)

// the V weight tables of a mixed batch, back to back, each as weight_table gives it for that sigma_grid alone
struct GilxTables { std::vector<double> table; std::vector<GilxVariant> var; int max_tlen = 0; };

// empty when the variants of `v` are acceptable for p->n_systems systems, else the text of the complaint, naming the value:
// the number of variants, every sigma_grid, every variant index and the order (the last two where given)
inline std::string gilx_check_variants(const gil_params *p, const gilx_variants *v) {
    const int V = v->n_variants, S = p->n_systems;
    if (V < 1 || V > GILX_MAX_VARIANTS) return "n_variants = " + std::to_string(V) + " is outside [1, " + std::to_string(GILX_MAX_VARIANTS) + "]";
    if (!v->sigma_grid) return "null sigma_grid";
    for (int i = 0; i < V; ++i)
        if (!std::isfinite(v->sigma_grid[i]) || v->sigma_grid[i] < 0.0)
            return "sigma_grid = " + std::to_string(v->sigma_grid[i]) + " of variant " + std::to_string(i) + " must be finite and not negative";
    if (v->variant_of_system)
        for (int s = 0; s < S; ++s) {
            const int i = v->variant_of_system[s];
            if (i < 0 || i >= V) return "variant index " + std::to_string(i) + " of system " + std::to_string(s) + " is outside [0, n_variants = " + std::to_string(V) + ")";
        }
    if (v->order) {
        std::vector<uint8_t> seen((size_t)S, 0);
        for (int b = 0; b < S; ++b) {
            const int s = v->order[b];
            if (s < 0 || s >= S) return "order is not a permutation: order[" + std::to_string(b) + "] = " + std::to_string(s) + " is outside [0, n_systems = " + std::to_string(S) + ")";
            if (seen[(size_t)s]++) return "order is not a permutation: system " + std::to_string(s) + " appears twice (second time at " + std::to_string(b) + ")";
        }
    }
    return "";
}

// the tables of checked variants: one weight_table call per variant, so a table's bits are those of a single-variant launch
inline void gilx_build_tables(const gil_params *p, const gilx_variants *v, GilxTables &tb) {
    const int V = v->n_variants;
    tb = GilxTables{};
    tb.var.resize((size_t)V);
    std::vector<double> one;
    for (int i = 0; i < V; ++i) {
        int tlen = 0, q = 0;
        weight_table(v->sigma_grid[i], p->L, p->K, p->periodic != 0, one, tlen, q);
        tb.var[(size_t)i] = GilxVariant{(int32_t)tb.table.size(), tlen, v->sigma_grid[i] > 0.0 ? 1 : 0, 0};
        tb.table.insert(tb.table.end(), one.begin(), one.end());   // tlen taps and the closing zero
        tb.max_tlen = std::max(tb.max_tlen, tlen);
    }
}

}  // namespace
