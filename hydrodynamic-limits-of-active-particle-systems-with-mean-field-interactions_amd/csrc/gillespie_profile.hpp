// gillespie_profile.hpp -- device side of include/gillespie_profile.h: the ensemble density and field profiles of
// PARTICLE_solver_CLASS.py:205-213, :517-536 (rho_plus_list, rho_minus_list, m_local_list) taken inside the exact event loop.
// One device function, called at an observation by the profile instantiations of both loop kernels (gillespie_hip.hip: the
// system in LDS, 64 or 256 threads; gillespie_big_hip.hip: the state in global memory, 1024 threads):
//   1. the workgroup forms its system's bin counts completely in its profile slots in LDS -- a pass over the particle slots
//      (the bound count needs them) with LDS integer atomics, dead slots skipped; with the field a pass over the sites, a lane
//      per site, llrint(m * 2^32) added to the bin's 64-bit slot;
//   2. a lane per bin then adds n+, n-, n_bound, n+^2, n-^2, n+ n- and the field sum to the row of the system's group with
//      64-bit integer global atomics whose result nobody reads (no-return atomics); zeros are not sent.  Bins are the innermost
//      index of a row, so the lanes of one such instruction touch contiguous words.  Integer addition is exact: the sums do
//      not depend on the order in which the systems arrive.
// The event loop holds no register for any of it, and no workgroup waits on another.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>

#include "gillespie.h"

// What gilp_run hands to the drivers of the two kernels (host side; the two sources are linked into one library)
struct GilpCall {
    const int32_t *group_of_system;            // [S] or nullptr (all in group 0)
    int n_groups, n_bins, first_obs, want_field;
    int64_t *ensemble_sums;                    // [G][n_obs][7][n_bins]
    int32_t *members, *profile_obs;            // [G][n_obs]; [S][n_obs][3][n_bins] or nullptr
};

// bytes of the profile slots of one workgroup: three int counts per bin, rounded up to 8, and a 64-bit field sum per bin
constexpr size_t gilp_lds_bytes(int n_bins, bool want_field) {
    return 8 * (((size_t)3 * n_bins + 1) / 2) + (want_field ? (size_t)8 * n_bins : 0);
}

// device copies of the outputs of one profile call (gilp_plan_info.output_bytes)
inline int64_t gilp_output_bytes(const gil_params *p, int n_groups, int n_bins, bool states, bool per_system) {
    const int64_t S = p->n_systems, O = p->n_obs, N = p->n_cap;
    return S * ((states ? O * N * 6 : 0) + O * GIL_NSCALARS * 8 + N * 24 + 24) + (int64_t)n_groups * O * (7 * (int64_t)n_bins * 8 + 4) +
           (per_system ? S * O * 3 * (int64_t)n_bins * 4 : 0);
}

namespace {

constexpr int GILP_PLUS = 1, GILP_BOUND = 2, GILP_ALIVE = 4;   // F_PLUS, F_BOUND, F_ALIVE of the loop kernels' flag byte
constexpr int GILP_COLS = 7;                   // GILP_NCOLS of the header

struct GilpArgs {                              // what a profile instantiation gets on top of the loop's own arguments
    unsigned long long *sums;                  // [n_groups][n_obs][7][n_bins], zeroed before the launch
    int *members;                              // [n_groups][n_obs], zeroed before the launch
    int *rows;                                 // [n_systems][n_obs][3][n_bins] (zero-filled), or nullptr
    const int32_t *group;                      // [n_systems]
    int n_bins, n_used, width, first_obs, want_field;
};

// Observation k of system `sys`: every thread of the workgroup calls it (it holds barriers).  pos / flg: the particle slots
// (LDS or global); W, S: the smoothed histograms of the observed state; field_mode false: every site carries mg.  `slots`:
// the workgroup's gilp_lds_bytes() of LDS, used here only.
template <int NT>
__device__ inline void gilp_record(const GilpArgs &c, void *slots, size_t sys, int k, int nobs, int L, int ncap, const int *pos,
                                   const uint8_t *flg, const double *W, const double *S, bool field_mode, double mg) {
    const int t = threadIdx.x, nb = c.n_bins, nu = c.n_used, width = c.width;
    int *cnt = static_cast<int *>(slots);                                      // [3][nb] n+, n-, n_bound
    unsigned long long *fld = reinterpret_cast<unsigned long long *>(static_cast<char *>(slots) + 8 * (((size_t)3 * nb + 1) / 2));   // [nb]
    for (int q = t; q < 3 * nb; q += NT) cnt[q] = 0;
    if (c.want_field) for (int q = t; q < nb; q += NT) fld[q] = 0;
    __syncthreads();
    for (int i = t; i < ncap; i += NT) {                       // particle slots -> bin counts
        const uint8_t f = flg[i];
        if (!(f & GILP_ALIVE)) continue;
        const int b = pos[i] / width;                          // pos < L, so b < n_used <= nb
        atomicAdd(&cnt[((f & GILP_PLUS) ? 0 : nb) + b], 1);
        if (f & GILP_BOUND) atomicAdd(&cnt[2 * nb + b], 1);
    }
    if (c.want_field) {
        if (field_mode) {
            for (int x = t; x < L; x += NT) {                  // sites -> the bin's fixed-point field sum
                const double w = W[x];
                double m = 0.0;
                if (w > 0.0) { m = S[x] / w; m = m > 1.0 ? 1.0 : (m < -1.0 ? -1.0 : m); }
                const long long q = llrint(m * 4294967296.0);
                if (q != 0) atomicAdd(&fld[x / width], (unsigned long long)q);
            }
        } else {
            const long long q = llrint(mg * 4294967296.0);
            for (int b = t; b < nu; b += NT) fld[b] = (unsigned long long)(q * (long long)(min(L, (b + 1) * width) - b * width));
        }
    }
    __syncthreads();
    const size_t row = ((size_t)c.group[sys] * nobs + k) * GILP_COLS * (size_t)nb;
    for (int b = t; b < nu; b += NT) {                         // a lane per bin: contiguous words of a column
        const long long np = cnt[b], nm = cnt[nb + b], nd = cnt[2 * nb + b];
        unsigned long long *dst = c.sums + row + b;
        if (np) { atomicAdd(dst, (unsigned long long)np); atomicAdd(dst + 3 * (size_t)nb, (unsigned long long)(np * np)); }
        if (nm) { atomicAdd(dst + (size_t)nb, (unsigned long long)nm); atomicAdd(dst + 4 * (size_t)nb, (unsigned long long)(nm * nm)); }
        if (nd) atomicAdd(dst + 2 * (size_t)nb, (unsigned long long)nd);
        if (np && nm) atomicAdd(dst + 5 * (size_t)nb, (unsigned long long)(np * nm));
        if (c.want_field) { const unsigned long long f = fld[b]; if (f) atomicAdd(dst + 6 * (size_t)nb, f); }
        if (c.rows) {
            int *r = c.rows + ((sys * nobs + k) * 3) * (size_t)nb + b;
            r[0] = (int)np; r[nb] = (int)nm; r[2 * (size_t)nb] = (int)nd;
        }
    }
    if (t == 0) atomicAdd(&c.members[(size_t)c.group[sys] * nobs + k], 1);
    __syncthreads();                                           // the slots are free for the next observation
}

}  // namespace
