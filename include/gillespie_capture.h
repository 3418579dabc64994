/* gillespie_capture.h -- C ABI of the exact event loop WITH ANCHOR-CAPTURE AND CLUSTER STATISTICS taken on the device (part
 * of libaps_hip.so).
 *
 * Same dynamics, parameters (gil_params, reused unchanged), buffers and error codes as include/gillespie.h.  The reference's
 * capture study (PARTICLE_solver_CLASS.py:766-976, plot_individuals: cluster sizes, bound-state lifetimes, survival curve,
 * cumulative exits per anchor) reads them off the snapshots of one run.  Here the event-loop kernels take them where the state
 * lives:
 *
 *  - at every bind, unbind and exit, in the thread that applies the event: a bind time per particle slot (0 for particles that
 *    start bound); when a bound state ends, lifetime = t - t_bind goes into life_hist[end][min(h_bins - 1, floor(lifetime /
 *    h_dt))] and into the sums life_sums[end] = {sum lifetime, sum lifetime^2}, end = 0 for unbinding and 1 for the exit of a
 *    bound particle; an exit is counted for the anchor group of its site.  t is the clock of the exit log: the loop time when
 *    the event is applied, before its own waiting time is added.  Particles still bound at the end are not counted.
 *  - at every observation k >= first_obs: one row of GILC_NFIXED + n_groups + c_bins integers,
 *      [0] live particles   [1] bound particles   [2] binds so far   [3] unbinds so far   [4] exits so far
 *      [5] occupied sites   [6] clusters          [7] largest cluster                     [8] sum of size^2
 *      [9 .. 9 + G)              exits so far per anchor group
 *      [9 + G .. 9 + G + c_bins) clusters of size 1, 2, ..., c_bins - 1, and >= c_bins
 *    A cluster is a maximal run of consecutive sites with at least one particle, scanned from site 0 to L - 1; runs do not
 *    join across the seam, also on a ring.  "So far" counts the events applied before the observation, i.e. the exits logged
 *    with a time < times_obs[k] (the event that crossed the observation time was drawn before it).  Rows before first_obs,
 *    and rows of observations the loop never reached (n_recorded), are zero.
 *
 * gilc_run picks the shape as gils_run does (include/gillespie_structure.h): a system with L <= GIL_MAX_L and n_cap <=
 * GIL_MAX_N whose loop plus capture slots fit the 160 KB of LDS runs in the batch kernel (Philox counter (event, system)), any
 * other in the large-system kernel (system s: key seed + s, as gilm_run).  Recording changes nothing else: states, scalar sums,
 * exit log, event counts and times are those of gil_run_batch / gilm_run for the same arguments.
 * All functions return 0 on success and a negative code on failure; gilc_last_error() gives the text.
 */
#ifndef GILLESPIE_CAPTURE_H
#define GILLESPIE_CAPTURE_H

#include <stdint.h>

#include "gillespie.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GILC_NFIXED 9           /* entries of a row before the per-group and per-size counts */
#define GILC_MAX_GROUPS 32      /* n_groups is in [0, GILC_MAX_GROUPS] */
#define GILC_MAX_CBINS 64       /* c_bins is in [2, GILC_MAX_CBINS] */
#define GILC_MAX_HBINS 256      /* h_bins is in [1, GILC_MAX_HBINS] */

typedef struct gilc_plan_info {
    int32_t shape;              /* GILS_SHAPE_BATCH (0) or GILS_SHAPE_LARGE (1) of gillespie_structure.h */
    int32_t threads;            /* per system: 64 (n_cap <= 1024) or 256 in the batch shape, 1024 in the large shape */
    int32_t lds_bytes;          /* dynamic LDS of one workgroup: the loop's own (batch shape: rounded up to 8) plus the capture
                                   slots, 8 * (12 + threads / 64 + 2 * h_bins + n_groups + c_bins), plus in the batch shape
                                   8 * n_cap for the bind times */
    int32_t row_len;            /* GILC_NFIXED + n_groups + c_bins */
    int64_t work_bytes;         /* device scratch of the whole batch: L * 4 for the group table when n_groups > 0, plus in the
                                   large shape n_systems * (work_bytes_per_system of gilm_plan_info + 8 * n_cap bind times) */
    int64_t output_bytes;       /* device copies of the outputs: n_systems * (n_obs * n_cap * 6 when states are wanted
                                   + n_obs * GIL_NSCALARS * 8 + n_cap * 24 (exit log) + 24 + n_obs * row_len * 8
                                   + 2 * h_bins * 8 + 32) */
} gilc_plan_info;

const char *gilc_last_error(void);

/* What gilc_run would use for these parameters: pure host arithmetic, no device is touched.  Refuses what gilc_run refuses
 * on these numbers alone, naming the offending number (n_groups outside [0, 32], c_bins outside [2, 64], h_bins outside
 * [1, 256], first_obs outside [0, n_obs], the limits of the shape), and a batch whose work_bytes + output_bytes exceed 2^38
 * (gilc_run compares with the free device memory and gives both numbers). */
int gilc_plan(const gil_params *p, int32_t n_groups, int32_t c_bins, int32_t h_bins, int32_t first_obs, int32_t want_states,
              gilc_plan_info *out);

/* group_of_site: int32[L], the anchor group of a site or -1, or NULL (no exits per group are counted; n_groups may still be
 * positive, its columns stay zero).  Refused: a group id >= n_groups (or < -1), a group on a site that p->anchor_mask does
 * not mark, h_dt <= 0 or not finite.  The arguments from n0 to n_exits are those of gil_run_batch, in its order, with the
 * same meaning; any output of those may be NULL.  Required: capture_obs [n_systems][n_obs][row_len], life_hist
 * [n_systems][2][h_bins], life_sums [n_systems][2][2]. */
int gilc_run(const gil_params *p, const int32_t *group_of_site, int32_t n_groups, int32_t c_bins, int32_t h_bins, double h_dt,
             int32_t first_obs,
             const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0, const double *uniforms,
             int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs, int32_t *n_recorded,
             int64_t *n_events, double *t_final, double *exits, int32_t *n_exits,
             int64_t *capture_obs, int64_t *life_hist, double *life_sums, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* GILLESPIE_CAPTURE_H */
