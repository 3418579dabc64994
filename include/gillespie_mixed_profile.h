/* gillespie_mixed_profile.h -- C ABI of the exact event loop for MIXED BATCHES WITH ENSEMBLE DENSITY AND FIELD PROFILES taken on
 * the device (part of libaps_hip.so).
 *
 * The study this combines: the ensemble means <rho+(x, t)>, <rho-(x, t)>, <m(x, t)> that are set against the hydrodynamic-limit
 * PDE (PARTICLE_solver_CLASS.py:205-213, :517-536), swept over what a launch of gilp_run (include/gillespie_profile.h) has one
 * value of: the kernel width sigma (the particle counterpart of include/pde_sweep.h) and the density N / L.  gilx_run
 * (include/gillespie_mixed.h) and gilxm_run (include/gillespie_mixed_many.h) put systems of different widths and blocking
 * tables into one launch, without profiles.  gilxp_run is that mixed launch with the profile sums of gilp_run, in both shapes.
 *
 * WHAT A SYSTEM COMPUTES, two identities:
 *   (a) every output but ensemble_sums, members and profile_obs is, bit for bit (times included), what gilx_run (batch shape)
 *       or gilxm_run (large shape) returns for the same p, v and start states: recording changes nothing else;
 *   (b) the three profile outputs are the bin pass of gilp_run on the states of (a), every system with its own variant's field
 *       (a variant with sigma_grid = 0 carries the global mean on every site).
 * Parameters (gil_params and gilx_variants, both reused unchanged; p->sigma_grid and p->block_table are IGNORED as in gilx_run),
 * Philox keys, streams and their defaults, the launch order (NULL: falling n0) and the error codes are those of the mixed
 * launch of the shape.  ensemble_sums [n_groups][n_obs][GILP_NCOLS][n_bins], members [n_groups][n_obs] and profile_obs
 * [n_systems][n_obs][3][n_bins], their bins, columns, fixed-point field sum and zero rows: include/gillespie_profile.h, word for
 * word.  A group may hold systems of different variants.  The sums are 64-bit integer atomics whose result nobody reads; the
 * device copies of ensemble_sums and members are zeroed before the launch; no workgroup waits on another.
 *
 * The shape is chosen as gilp_run chooses it, with the longest table of the batch: the batch shape (gilx_run's kernel) when
 * L <= GIL_MAX_L, n_cap <= GIL_MAX_N and the loop plus the profile slots fit the 160 KB of LDS, otherwise the large shape
 * (gilxm_run's kernel).  The defaults of v->seed and v->stream follow the shape, so a caller who wants a system's numbers to be
 * those of another launch asks gilxp_plan for the shape first and passes both.
 * All functions return 0 on success and a negative code on failure; gilxp_last_error() gives the text.
 */
#ifndef GILLESPIE_MIXED_PROFILE_H
#define GILLESPIE_MIXED_PROFILE_H

#include <stdint.h>

#include "gillespie.h"
#include "gillespie_mixed.h"
#include "gillespie_profile.h"
#include "gillespie_structure.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gilxp_plan_info {
    int32_t shape;              /* GILS_SHAPE_BATCH (0) or GILS_SHAPE_LARGE (1) of gillespie_structure.h */
    int32_t threads;            /* per system: 64 (n_cap <= 1024) or 256 in the batch shape, 1024 in the large shape */
    int32_t lds_bytes;          /* dynamic LDS of one workgroup: the mixed launch's for the longest table (gilx_plan's, rounded up
                                   to 8, or gilxm_plan's) plus the profile slots, 8 * ceil(3 * n_bins / 2) for the counts plus
                                   8 * n_bins with want_field */
    int32_t max_tlen;           /* length of the longest weight table (taps without the closing zero) */
    int32_t bin_width;          /* ceil(L / n_bins) */
    int32_t n_bins_used;        /* ceil(L / bin_width) */
    int64_t table_doubles;      /* all V tables back to back, each with its closing zero */
    int64_t work_bytes;         /* device scratch of the whole batch: n_systems * 4 for the group table, plus in the large shape
                                   n_systems * work_bytes_per_system of gilxm_plan_info */
    int64_t output_bytes;       /* device copies of the outputs: gilp_plan_info's formula */
} gilxp_plan_info;

const char *gilxp_last_error(void);

/* What gilxp_run would use: pure host arithmetic, no device is touched.  Needs of p and v what gilx_plan needs.  Refuses, naming
 * the offending value, first what the mixed launch refuses (gilx_plan where the batch shape takes the launch, else gilxm_plan),
 * then what gilp_plan refuses: n_bins outside [1, min(L, 1024)], n_groups outside [1, 4096], first_obs outside [0, n_obs],
 * want_field with L * n_systems >= 2^31, a large-shape launch beyond 160 KB of LDS, and a batch whose work_bytes + output_bytes
 * exceed 2^38 (gilxp_run compares with the free device memory). */
int gilxp_plan(const gil_params *p, const gilx_variants *v, int32_t n_bins, int32_t n_groups, int32_t first_obs, int32_t want_field,
               int32_t want_states, int32_t want_per_system, gilxp_plan_info *out);

/* n_bins, first_obs, want_field, group_of_system, n_groups: those of gilp_run (an id outside [0, n_groups) is refused).  The
 * arguments from n0 to n_exits are those of gil_run_batch, in its order, with the meaning they have in gilx_run / gilxm_run; any
 * output of those may be NULL.  Required: ensemble_sums and members; profile_obs may be NULL. */
int gilxp_run(const gil_params *p, const gilx_variants *v, int32_t n_bins, int32_t first_obs, int32_t want_field,
              const int32_t *group_of_system, int32_t n_groups,
              const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0, const double *uniforms,
              int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs, int32_t *n_recorded,
              int64_t *n_events, double *t_final, double *exits, int32_t *n_exits,
              int64_t *ensemble_sums, int32_t *members, int32_t *profile_obs, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* GILLESPIE_MIXED_PROFILE_H */
