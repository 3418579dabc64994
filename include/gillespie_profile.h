/* gillespie_profile.h -- C ABI of the exact event loop WITH ENSEMBLE DENSITY AND FIELD PROFILES taken on the device (part of
 * libaps_hip.so).
 *
 * Same dynamics, parameters (gil_params, reused unchanged), buffers and error codes as include/gillespie.h.  The reference keeps
 * per run three M x L arrays, rho_plus_list, rho_minus_list and m_local_list (PARTICLE_solver_CLASS.py:205-213, :517-536), and
 * the comparison with the hydrodynamic limit is made on their ensemble means.  Here the event-loop kernels coarse-grain the
 * observed state into n_bins bins of sites and add it to the sums of the system's GROUP (the ensemble whose members add into
 * the same sums, for instance all runs at one beta): what leaves the device is [groups][observations][7][bins], not states.
 *
 * Bins: width = ceil(L / n_bins) sites, the bin of site x is x / width (the rule of aps_observe_bins).  n_bins_used =
 * ceil(L / width) bins hold sites, the last of them L - (n_bins_used - 1) * width of them; bins beyond stay zero.
 *
 * ensemble_sums [n_groups][n_obs][GILP_NCOLS][n_bins], int64, bins innermost (the lanes that add a column touch contiguous
 * words).  Per bin, for the state recorded at observation k, with n+ / n- / n_bound the live plus, live minus and live bound
 * particles on the bin's sites (a bound particle also counts in n+ or n-), summed over the members of the group that recorded
 * observation k:
 *      [0] sum n+      [1] sum n-      [2] sum n_bound      [3] sum n+^2      [4] sum n-^2      [5] sum n+ n-
 *      [6] sum F, zero unless want_field.  F = sum over the bin's sites of llrint(m(x) * 2^32), m(x) = clip(S[x] / W[x], -1, 1)
 *          where W > 0, else 0: the field of the observed state (what gils_run sums); with sigma_grid = 0 (global mean field)
 *          every site carries sum sigma / n.  Fixed point makes the sum an integer, as every other sum of this library, so it
 *          does not depend on the order in which the systems arrive: a repeated call, or a system at another place of the
 *          batch, gives the same bits.  |F| <= 2^32 per site, hence want_field is refused when L * n_systems >= 2^31.
 *          NO SECOND MOMENT OF THE FIELD IS TAKEN: the square of a 2^32 fixed-point value does not fit 64 bits.
 * members [n_groups][n_obs], int32: the systems of the group that recorded observation k.  A system that ended before
 * observation k (n_recorded) adds nothing to that row.  Rows before first_obs are zero in both arrays.
 * profile_obs [n_systems][n_obs][3][n_bins], int32, optional: one system's own (n+, n-, n_bound) per bin; rows before first_obs
 * and rows the loop never reached are zero.  At n_bins = L it is a single run's heat map.
 *
 * Each workgroup forms the bin counts of its system completely in LDS (the squares need them) and then adds the non-zero ones
 * to the group's row with 64-bit integer global atomics that return nothing; integer addition is exact, so the arrival order
 * does not matter.  The device copies of ensemble_sums and members are zeroed before the launch.  No workgroup waits on another.
 *
 * gilp_run picks the shape as gils_run / gilc_run do: a system with L <= GIL_MAX_L and n_cap <= GIL_MAX_N whose loop plus
 * profile slots fit the 160 KB of LDS runs in the batch kernel (Philox counter (event, system)), any other in the large-system
 * kernel (system s: key seed + s, as gilm_run).  Recording changes nothing else: states, scalar sums, exit log, event counts
 * and times are those of gil_run_batch / gilm_run for the same arguments.
 * All functions return 0 on success and a negative code on failure; gilp_last_error() gives the text.
 */
#ifndef GILLESPIE_PROFILE_H
#define GILLESPIE_PROFILE_H

#include <stdint.h>

#include "gillespie.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GILP_NCOLS 7            /* columns of ensemble_sums */
#define GILP_MAX_BINS 1024      /* n_bins is in [1, min(L, GILP_MAX_BINS)] */
#define GILP_MAX_GROUPS 4096    /* n_groups is in [1, GILP_MAX_GROUPS] */

typedef struct gilp_plan_info {
    int32_t shape;              /* GILS_SHAPE_BATCH (0) or GILS_SHAPE_LARGE (1) of gillespie_structure.h */
    int32_t threads;            /* per system: 64 (n_cap <= 1024) or 256 in the batch shape, 1024 in the large shape */
    int32_t lds_bytes;          /* dynamic LDS of one workgroup: the loop's own (batch shape: rounded up to 8) plus the profile
                                   slots, 8 * ceil(3 * n_bins / 2) for the counts plus 8 * n_bins with want_field */
    int32_t bin_width;          /* ceil(L / n_bins) */
    int32_t n_bins_used;        /* ceil(L / bin_width) */
    int32_t reserved;
    int64_t work_bytes;         /* device scratch of the whole batch: n_systems * 4 for the group table, plus in the large shape
                                   n_systems * work_bytes_per_system of gilm_plan_info */
    int64_t output_bytes;       /* device copies of the outputs: n_systems * (n_obs * n_cap * 6 when states are wanted
                                   + n_obs * GIL_NSCALARS * 8 + n_cap * 24 (exit log) + 24)
                                   + n_groups * n_obs * (GILP_NCOLS * n_bins * 8 + 4)
                                   + n_systems * n_obs * 3 * n_bins * 4 when the per-system rows are wanted */
} gilp_plan_info;

const char *gilp_last_error(void);

/* What gilp_run would use for these parameters: pure host arithmetic, no device is touched.  Refuses what gilp_run refuses on
 * these numbers alone, naming the offending number (n_bins outside [1, min(L, 1024)], n_groups outside [1, 4096], first_obs
 * outside [0, n_obs], want_field with L * n_systems >= 2^31, the limits of the shape), and a batch whose work_bytes +
 * output_bytes exceed 2^38 (gilp_run compares with the free device memory and gives both numbers). */
int gilp_plan(const gil_params *p, int32_t n_bins, int32_t n_groups, int32_t first_obs, int32_t want_field, int32_t want_states,
              int32_t want_per_system, gilp_plan_info *out);

/* group_of_system: int32[n_systems], or NULL when every system belongs to group 0; an id outside [0, n_groups) is refused.
 * want_field: 0 or 1.  The arguments from n0 to n_exits are those of gil_run_batch, in its order, with the same meaning; any
 * output of those may be NULL.  Required: ensemble_sums and members; profile_obs may be NULL. */
int gilp_run(const gil_params *p, int32_t n_bins, int32_t first_obs, int32_t want_field, const int32_t *group_of_system,
             int32_t n_groups,
             const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0, const double *uniforms,
             int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs, int32_t *n_recorded,
             int64_t *n_events, double *t_final, double *exits, int32_t *n_exits,
             int64_t *ensemble_sums, int32_t *members, int32_t *profile_obs, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* GILLESPIE_PROFILE_H */
