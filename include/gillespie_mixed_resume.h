/* gillespie_mixed_resume.h -- C ABI of MIXED BATCHES of the exact event loop run in SEGMENTS: a mixed launch may end with a
 * checkpoint, and a mixed launch may start from one (part of libaps_hip.so).
 *
 * gilxr_run is gilx_run (include/gillespie_mixed.h), gilxmr_run is gilxm_run (include/gillespie_mixed_many.h: large systems)
 * and gilxsr_run is gilxs_run (include/gillespie_mixed_structure.h: with the structure sums and their window reduction), each
 * with three more arguments behind kernel_ms: the grid index of the launch's first observation, the checkpoint the launch
 * starts from and the checkpoint it leaves.  Parameters, variants, buffers and error codes are those of these headers; the
 * rules of a segment are those of include/gillespie_resume.h, which this header refers to for their reasons:
 *
 *   * CUT INVARIANCE.  A chain of such launches gives, bit for bit, what gilx_run / gilxm_run / gilxs_run give in one launch:
 *     the states, the scalar sums and the head rows at every observation, every entry of window, n_window and n_empty, the
 *     event counts, the final times and the concatenated exit logs, wherever and however often the run is cut.
 *   * OBSERVATIONS.  p->times_obs holds the ABSOLUTE times of the observations obs_first .. obs_first + p->n_obs - 1 of the
 *     run's grid, every per-observation output (head_obs and structure_obs too) has p->n_obs rows, p->ref_obs counts within
 *     the slice (-1: the origin lies in another launch), p->T is the run's.  A fresh start records row 0 before the first event;
 *     a resumed start first records the PENDING observations k >= next_obs with times_obs[k] <= t, unless t > T.
 *   * A checkpoint with t = +inf (the total rate fell to zero) or t > T records nothing and ends at once; a launch also ends
 *     when max_events events have fired since the run's start.  `uniforms` and max_events count from the run's start.
 *   * A system whose checkpoint lies before obs_first must have ended: it is skipped, n_recorded[s] is 0 and its checkpoint is
 *     passed on unchanged, n_slots and the window sums included; otherwise the call is refused.
 *   * from == NULL is a fresh start from n0 / pos0 / sigma0 / bound0 (not read otherwise, may be NULL then); to == NULL: no
 *     checkpoint is wanted.  `from` and `to` may be the same struct.
 *   * The exit log holds the exits of this launch only.
 *
 * What a mixed launch needs beyond gil_checkpoint:
 *
 * n_slots.  A mixed system groups its rate sums by its own slot count, chunk = ceil(n0[s] / threads) (gillespie_mixed.h), and
 * its loops run over these slots.  The slot count of a resumed system is therefore the checkpoint's n_slots[s] = the n0[s] of
 * the run's start, dead slots included -- NOT the number of live particles: with another grouping the total rate differs in
 * its last bit and the trajectory departs.  On resume n0 is not read.  n_slots[s] must lie in [0, n_cap], and a slot at or
 * beyond it must have flags 0; the refusal names the system.  In the checkpoint left, the slots at and beyond n_slots[s] have
 * position 0, flags 0 and origin -1.  (The large shape sums its rates in blocks of the launch's n_cap; it checks n_slots and
 * passes it on.)
 *
 * Keys and variants.  The Philox key and stream of a system come from v->seed and v->stream, and the variants from v: they
 * belong to the RESUMING launch, as in gilx_run.  The caller passes the same keys for the same trajectory.  The variants are
 * parameters like beta: a launch resumed with another table is the exact process with the range switched at the checkpoint.
 * The default launch order (v->order == NULL) is by falling n_slots.
 *
 * Structure launches (gilxsr_run).  first_obs is an ABSOLUTE index on the run's grid, >= 0: row k of a slice belongs to the
 * window when obs_first + k >= first_obs.  On a resumed start the accumulators window, n_window and n_empty start from the
 * checkpoint's values instead of zero (whether the window has taken its first observation is n_window == 0, carried across
 * the cut); at the end they go into `to`: the checkpoint carries the window sums, they are no separate output.  head_obs and
 * structure_obs cover the slice's rows.  Refused: from->window (or n_window, n_empty) == NULL, a negative n_window or
 * n_empty; `to` without the three arrays.  k_max must be the run's in every launch (the layout of `window`).
 *
 * Plans.  gilx_plan, gilxm_plan and gilxs_plan hold for the resumable entry points: a resumed launch uses the same LDS and
 * the same thread counts.  gilxr_run and gilxsr_run use n_systems * n_cap * 9 bytes more of device memory, for the end state.
 *
 * All functions return 0 on success and a negative code on failure; gilxr_last_error() gives the text for all three.
 */
#ifndef GILLESPIE_MIXED_RESUME_H
#define GILLESPIE_MIXED_RESUME_H

#include <stdint.h>

#include "gillespie.h"
#include "gillespie_mixed.h"
#include "gillespie_resume.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The state of a mixed batch between two launches: caller-allocated host arrays. */
typedef struct gilx_checkpoint {
    gil_checkpoint base;        /* pos, flags, ref, t, n_events, next_obs: include/gillespie_resume.h, unchanged */
    int32_t *n_slots;           /* [n_systems] the system's slot count n0[s] of the run's start */
    double *window;             /* [n_systems][k_max][3] a0, sum d, sum d^2; structure launches only, else NULL */
    int32_t *n_window;          /* [n_systems] observations the window took; structure launches only, else NULL */
    int32_t *n_empty;           /* [n_systems] window observations without a live particle; structure launches only, else NULL */
} gilx_checkpoint;

const char *gilxr_last_error(void);

/* gilx_run with a start and an end state. */
int gilxr_run(const gil_params *p, const gilx_variants *v,
              const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0, const double *uniforms,
              int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs, int32_t *n_recorded,
              int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, double *kernel_ms,
              int32_t obs_first, const gilx_checkpoint *from, gilx_checkpoint *to);

/* gilxm_run likewise (the keys' defaults are gilxm_run's: p->seed + s, stream 0). */
int gilxmr_run(const gil_params *p, const gilx_variants *v,
               const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0, const double *uniforms,
               int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs, int32_t *n_recorded,
               int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, double *kernel_ms,
               int32_t obs_first, const gilx_checkpoint *from, gilx_checkpoint *to);

/* gilxs_run likewise; window, n_window and n_empty travel in the checkpoints.  head_obs is required, structure_obs optional. */
int gilxsr_run(const gil_params *p, const gilx_variants *v, int32_t k_max, int32_t first_obs,
               const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0, const double *uniforms,
               int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs, int32_t *n_recorded,
               int64_t *n_events, double *t_final, double *exits, int32_t *n_exits,
               double *structure_obs, double *head_obs, double *kernel_ms,
               int32_t obs_first, const gilx_checkpoint *from, gilx_checkpoint *to);

#ifdef __cplusplus
}
#endif
#endif /* GILLESPIE_MIXED_RESUME_H */
