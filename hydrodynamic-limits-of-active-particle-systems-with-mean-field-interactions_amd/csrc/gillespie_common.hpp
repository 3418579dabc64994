// gillespie_common.hpp -- host side of what the two shapes of the exact event loop share: gillespie_hip.hip (many systems,
// each in one workgroup's LDS) and gillespie_big_hip.hip (one large system in global memory), both of include/gillespie.h.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "gillespie.h"
#include "aps_common.hpp"
#include "dev_mem.hpp"

namespace {

// the rate code's parameters of a run: no time step, no caller's flip table yet (gil_upload_flip_table)
inline Model gil_model(const gil_params *p) {
    Model M{};
    M.L = p->L; M.K = p->K; M.periodic = p->periodic ? 1 : 0; M.field_mode = p->sigma_grid > 0.0 ? 1 : 0;
    M.minus_anchor = p->minus_anchor ? 1 : 0; M.immobilize = p->immobilize ? 1 : 0; M.suppress_flip = p->suppress_flip ? 1 : 0;
    M.crowding = p->crowding ? 1 : 0; M.rate_diffusion = p->rate_diffusion; M.rate_active = p->rate_active;
    M.k_on = p->k_on; M.k_off = p->k_off; M.k_exit = p->k_exit; M.dt = 0.0;
    M.seed_lo = (uint32_t)p->seed; M.seed_hi = (uint32_t)(p->seed >> 32); M.ens_base = 0;
    M.flip_n = 0; M.flip_tab = nullptr;
    return M;
}

// nullptr when the n particles of one initial state are acceptable, else the text of the complaint
inline const char *gil_check_state(const gil_params *p, int n, const int32_t *pos, const int8_t *sigma) {
    std::vector<int> occ((size_t)p->L, 0);
    for (int i = 0; i < n; ++i) {
        if (pos[i] < 0 || pos[i] >= p->L) return "position outside [0, L)";
        if (++occ[(size_t)pos[i]] > p->K) return "site capacity exceeded";
        if (sigma[i] != 1 && sigma[i] != -1) return "sigma must be +1 or -1";
    }
    return nullptr;
}

// nullptr when a caller's flip table is acceptable (or absent), else the text of the complaint: aps_set_flip_table's rules.
// A negative or non-finite rate would make a particle's cumulative sums non-monotone on the device.  Host arithmetic only:
// the drivers ask before they touch the device.
inline const char *gil_check_flip_table(const gil_params *p) {
    if (!p->flip_table) return nullptr;
    if (p->flip_n < 1 || p->flip_n > (1 << 24)) return "flip_n must be in [1, 2^24]";
    for (size_t i = 0, n = (size_t)2 * ((size_t)p->flip_n + 1); i < n; ++i)
        if (!(p->flip_table[i] >= 0.0) || !std::isfinite(p->flip_table[i])) return "rates must be finite and >= 0";
    return nullptr;
}

// a caller's flip_rate_fn, tabulated (aps_set_flip_table's layout): onto the device and into the model
inline int gil_upload_flip_table(OneShot &job, const gil_params *p, Model &M) {
    if (!p->flip_table) return 0;
    if (const char *why = gil_check_flip_table(p)) return job.fail(job.e_arg, std::string(job.who) + ": " + why);
    if (int rc = job.upload(&M.flip_tab, p->flip_table, (size_t)2 * ((size_t)p->flip_n + 1), "flip_table")) return rc;
    M.flip_n = p->flip_n;
    return 0;
}

}  // namespace

// gils_run (gillespie_hip.hip, include/gillespie_structure.h) reaches the large-system kernel of gillespie_big_hip.hip
// through these two: inside the library only.  The plan gives the LDS bytes of a workgroup with the structure sums'
// slots and the work bytes of the whole batch; the run is gilm_run's driver with the rows of structure sums.
__attribute__((visibility("hidden"))) int gils_large_plan(const char *who, std::string &err, const gil_params *p, int32_t *lds_bytes,
                                                          int64_t *work_bytes);
__attribute__((visibility("hidden"))) int gils_large_run(const char *who, std::string &err, const gil_params *p, const int32_t *n0,
                                                         const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0, const double *uniforms,
                                                         int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs,
                                                         int32_t *n_recorded, int64_t *n_events, double *t_final, double *exits,
                                                         int32_t *n_exits, double *kernel_ms, int k_max, int first_obs, double *structure_obs);
