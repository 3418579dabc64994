/* gillespie_profile_resume.h -- C ABI of the exact event loop WITH ENSEMBLE PROFILES run in SEGMENTS: a profile launch may end
 * with a checkpoint, and a profile launch may start from one (part of libaps_hip.so).
 *
 * gilpr_run is the profile launch of include/gillespie_profile.h, gilxpr_run the mixed profile launch of
 * include/gillespie_mixed_profile.h, each with the three arguments a segment adds in include/gillespie_resume.h and
 * include/gillespie_mixed_resume.h: the grid index of the slice's first row, the checkpoint the launch starts from and the
 * checkpoint it leaves.  Parameters (gil_params, gilx_variants), buffers, bins, columns, the fixed-point field sum and the error
 * codes are those headers', unchanged.
 *
 * WHY THE LOOP STATE IS ALL A CUT HANDS OVER.  A row of ensemble_sums, members and profile_obs belongs to ONE observation: the
 * bin counts of the state recorded there, added over the members of a group.  Nothing of a row is carried to the next.  The
 * checkpoint is therefore gil_checkpoint / gilx_checkpoint as they are -- no new struct -- and the rows of a chain of segments,
 * laid one after the other along the observation axis, are the rows of the one launch bit for bit: the trajectory by the cut
 * invariance of include/gillespie_resume.h, the rows because they are exact integer sums of that trajectory's states.
 *
 * SHAPE AND KEYS.  Both pick the shape exactly as their one-launch counterparts do: the batch kernel where the loop plus the
 * profile slots fit the 160 KB of LDS, else the large-system kernel with the large shape's key convention (unmixed: system s
 * draws with p->seed + s; mixed: the defaults of v->seed and v->stream follow the shape).  The shape does not depend on n_obs,
 * so every segment of a chain gets the same one; the plans of the two one-launch headers hold for a segment, with n_obs the
 * slice's length.  On top of the plan's bytes a segment stages the start state and, in the batch shape, room for the end state:
 * n_systems * (n_cap * 9 + 20) bytes in, n_systems * n_cap * 9 bytes out (pos, ref: int32, flags: a byte, per slot; t, n_events,
 * first row: per system); the large shape ends in its work memory and stages the n_systems * (n_cap * 5 + 20) bytes that its
 * start state does not already hold.
 *
 * SLICES.  The rules are those of include/gillespie_resume.h:
 *   * p->times_obs holds the ABSOLUTE times of the observations obs_first, ..., obs_first + p->n_obs - 1;
 *   * first_obs is ABSOLUTE on the run's grid and must be >= 0 (the one-launch counterparts bound it by n_obs; here it may lie in
 *     a later slice or beyond the grid).  Rows of the slice before it are zero in all three arrays;
 *   * ensemble_sums [n_groups][p->n_obs][GILP_NCOLS][n_bins], members [n_groups][p->n_obs] and profile_obs
 *     [n_systems][p->n_obs][3][n_bins] have p->n_obs rows: row k is observation obs_first + k.  Their device copies are
 *     zero-filled for every launch.
 * START AND END.  A fresh start (from == NULL) records row 0 before the first event.  PENDING OBSERVATIONS: a resumed start
 * records every observation k >= next_obs with times_obs[k] <= t before its first event, and these rows go through the same bin
 * pass, with the state the checkpoint holds (the global mean of a sigma_grid = 0 system is rebuilt from its live flags).  A
 * checkpoint with t = +inf or t > T records nothing.  A system whose checkpoint lies before obs_first must have ended (t > T, or
 * max_events reached): it records nothing and adds nothing to members; a live one is refused.  to == NULL asks for no
 * checkpoint; `from` and `to` may be the same struct.
 * In gilx_checkpoint, n_slots is checked as the mixed segments check it (inside [0, n_cap], no flags at or beyond it), and
 * window, n_window and n_empty must be NULL in both `from` and `to`: a profile launch carries no window sums, and a call that
 * passes them is refused.
 *
 * REFUSALS, on the host before any device is touched, each naming the offending value, in this order: what the mixed launch
 * refuses (gilxpr_run), what the profile call refuses (n_bins, n_groups, a negative first_obs, want_field, group ids, the limits
 * of the shape), what the segment refuses (the checkpoint's arrays and numbers), then a batch whose work and output bytes
 * exceed what a plan accepts.  All functions return 0 on success and a negative code on failure; gilpr_last_error() gives the
 * text for both.
 */
#ifndef GILLESPIE_PROFILE_RESUME_H
#define GILLESPIE_PROFILE_RESUME_H

#include <stdint.h>

#include "gillespie.h"
#include "gillespie_mixed.h"
#include "gillespie_profile.h"
#include "gillespie_resume.h"
#include "gillespie_mixed_resume.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *gilpr_last_error(void);

/* The profile launch of include/gillespie_profile.h, its arguments in its order, as one segment. */
int gilpr_run(const gil_params *p, int32_t n_bins, int32_t first_obs, int32_t want_field, const int32_t *group_of_system,
              int32_t n_groups,
              const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0, const double *uniforms,
              int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs, int32_t *n_recorded,
              int64_t *n_events, double *t_final, double *exits, int32_t *n_exits,
              int64_t *ensemble_sums, int32_t *members, int32_t *profile_obs, double *kernel_ms,
              int32_t obs_first, const gil_checkpoint *from, gil_checkpoint *to);

/* The mixed profile launch of include/gillespie_mixed_profile.h, its arguments in its order, as one segment. */
int gilxpr_run(const gil_params *p, const gilx_variants *v, int32_t n_bins, int32_t first_obs, int32_t want_field,
               const int32_t *group_of_system, int32_t n_groups,
               const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0, const double *uniforms,
               int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs, int32_t *n_recorded,
               int64_t *n_events, double *t_final, double *exits, int32_t *n_exits,
               int64_t *ensemble_sums, int32_t *members, int32_t *profile_obs, double *kernel_ms,
               int32_t obs_first, const gilx_checkpoint *from, gilx_checkpoint *to);

#ifdef __cplusplus
}
#endif
#endif /* GILLESPIE_PROFILE_RESUME_H */
