/* gillespie_resume.h -- C ABI of the exact event loop run in SEGMENTS: a launch may end with a checkpoint, and a launch may
 * start from one (part of libaps_hip.so).
 *
 * Same dynamics, parameters (gil_params, reused unchanged), buffers and error codes as include/gillespie.h.  gilr_run is
 * gil_run_batch (systems in one workgroup's LDS), gilrm_run is gilm_run of include/gillespie_many.h (large systems), each
 * with two more arguments: the checkpoint the launch starts from and the checkpoint it leaves.  The structure and capture
 * entry points carry sums of their own across a run and cannot be resumed; the profile entry points, whose rows belong to one
 * observation each, have their segments in include/gillespie_profile_resume.h.  The mixed entry points (gilx_run,
 * gilxm_run, gilxs_run) need more than gil_checkpoint holds -- a slot count per system and, with the structure sums, the window
 * accumulators: their segments are gilxr_run, gilxmr_run and gilxsr_run of include/gillespie_mixed_resume.h, under these rules.
 *
 * CUT INVARIANCE.  A run resumed from a checkpoint is, bit for bit, the run that was never interrupted: the states and the
 * twelve scalar sums at every observation, the event counts, the final time and the concatenated exit logs are equal,
 * wherever and however often the run is cut.  This holds because
 *   * the random numbers of event e are a function of e, the key and the stream alone (gillespie.h, RANDOM NUMBERS), and a
 *     supplied `uniforms` table and `max_events` are indexed by the ABSOLUTE event number, counted from the run's start;
 *   * the smoothed histograms W, S are sums of weights on an exact grid, so a rebuild from the particles has the bits of the
 *     incrementally kept ones;
 *   * a particle's rate is a pure function of its state, the histograms and the occupancy around it;
 *   * the total rate and the block sums are taken from the rates in a fixed order by both kernels.
 * The parameters that are NOT part of the state (beta, the rates, the flip table, T) are those of the resuming launch: a
 * launch resumed with other values is the exact process with the parameter switched at the checkpoint's time.
 *
 * OBSERVATIONS.  A run has one grid of observation times, numbered from 0.  A launch gets a slice of it: p->times_obs holds
 * the ABSOLUTE times of the observations obs_first, ..., obs_first + p->n_obs - 1, and every per-observation output has
 * p->n_obs rows.  p->ref_obs counts within the slice (-1 where the origin of the displacement sums lies in another launch:
 * the checkpoint carries the origin).  p->T is the run's T in every launch.
 *   * A fresh start (from == NULL) records row 0 before the first event, as gil_run_batch does.
 *   * PENDING OBSERVATIONS.  The event that ends a launch may have passed observation times beyond the launch's slice.  In the
 *     uninterrupted run that event records them, with the state it left -- which is the checkpoint's.  A resumed start therefore
 *     records every observation k >= next_obs with times_obs[k] <= t before its first event, unless t > T (the uninterrupted
 *     run stopped at that event without recording, ref :515-516).
 *   * A checkpoint with t = +inf is a system whose total rate fell to zero; it records nothing and ends at once, like every
 *     checkpoint with t > T.
 *   * A launch ends where the loop of gil_run_batch ends: its last row is recorded, t > T, the total rate is zero, or
 *     max_events events have fired since the run's start.  The event that crossed T is applied and counted.
 * System s starts at row next_obs[s] - obs_first of the slice; the rows before it are left zero.  n_recorded[s] is the row
 * after the last one recorded (the start row where nothing was), and the checkpoint left has next_obs = obs_first +
 * n_recorded.  A system whose checkpoint lies before obs_first must have ended (t > T, or max_events reached): it records
 * nothing, n_recorded[s] is 0 and its checkpoint is passed on unchanged; otherwise the call is refused.
 * The exit log (exits, n_exits) holds the exits of this launch only.
 */
#ifndef GILLESPIE_RESUME_H
#define GILLESPIE_RESUME_H

#include <stdint.h>

#include "gillespie.h"
#include "gillespie_many.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GILR_PLUS 1             /* bits of gil_checkpoint.flags */
#define GILR_BOUND 2
#define GILR_ALIVE 4

/* The state of n_systems systems between two launches: caller-allocated host arrays.  A slot that never held a particle
 * has flags 0 and position 0; a particle that left keeps its last position (the observations show it) and loses ALIVE. */
typedef struct gil_checkpoint {
    int32_t *pos;               /* [n_systems][n_cap] site of every slot */
    uint8_t *flags;             /* [n_systems][n_cap] GILR_PLUS | GILR_BOUND | GILR_ALIVE */
    int32_t *ref;               /* [n_systems][n_cap] origin of the displacement sums (the site at observation ref_obs), or -1 */
    double *t;                  /* [n_systems] time after the last applied event; may exceed T, +inf when the total rate is zero */
    int64_t *n_events;          /* [n_systems] events fired since the run's start = index of the next event's random numbers */
    int32_t *next_obs;          /* [n_systems] first observation of the run's grid not yet recorded */
} gil_checkpoint;

const char *gilr_last_error(void);

/* gil_run_batch with a start and an end state.  from == NULL: a fresh start from n0 / pos0 / sigma0 / bound0 at t = 0 (which
 * are not read otherwise and may be NULL); obs_first is then the grid index of row 0, normally 0.  to == NULL: no checkpoint
 * wanted.  `from` and `to` may be the same struct.  The remaining arguments are those of gil_run_batch. */
int gilr_run(const gil_params *p, const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0,
             const double *uniforms, int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs,
             int32_t *n_recorded, int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, double *kernel_ms,
             int32_t obs_first, const gil_checkpoint *from, gil_checkpoint *to);

/* gilm_run likewise (system s draws with the key p->seed + s, as there). */
int gilrm_run(const gil_params *p, const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0,
              const double *uniforms, int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs,
              int32_t *n_recorded, int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, double *kernel_ms,
              int32_t obs_first, const gil_checkpoint *from, gil_checkpoint *to);

#ifdef __cplusplus
}
#endif
#endif /* GILLESPIE_RESUME_H */
