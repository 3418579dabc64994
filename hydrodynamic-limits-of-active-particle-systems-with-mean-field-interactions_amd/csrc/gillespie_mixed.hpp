// gillespie_mixed.hpp -- the batch kernel of the exact event loop for MIXED batches (include/gillespie_mixed.h): every
// system of the launch refers to one of V variants, a variant being an interaction range (its weight table) and a blocking
// table.  Included by gillespie_hip.hip only.  The code here is instantiated by the kernels that have the compile-time
// property MX; the others keep the launch-wide values of their arguments and are the code they were before it existed.
#pragma once

#include <cstdint>

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

}  // namespace
