/* pde_resume.h -- C ABI of the hydrodynamic-limit solver run in SEGMENTS: a launch may end with a checkpoint, and a launch
 * may start from one (part of libaps_hip.so).
 *
 * Same scheme, parameters (pde_params, reused unchanged), buffers and error codes as include/pde.h.  pder_solve is
 * pde_solve_batch, pdekr_solve is pdek_solve (include/pde_sweep.h) and pdewr_solve is pdew_solve (include/pde_wide.h), each with
 * two more arguments: the checkpoint the launch starts from and the checkpoint it leaves.  The three older entry points are
 * the `from == NULL, to == NULL` case of the same kernels.
 *
 * THE CUT.  The loop of a solve is `row 0, (step, row) x nsteps`; a "row" is what is recorded of a state -- the series, the
 * Fourier modes, a snapshot when the row's number is a multiple of snapshot_interval -- followed by the tracers' move in
 * that state's magnetisation.  A checkpoint at step c is the state after row c was recorded and the tracers made the move of
 * row c, before step(): a fresh launch of N1 steps followed by a resumed launch of N2 steps is a fresh launch of N1 + N2.
 * There is no "final" flag, and extending a finished run is resuming it.
 *
 * CUT INVARIANCE.  Chained launches give, bit for bit, the rows, final state and checkpoint of the single launch, wherever and
 * however often the run is cut, PROVIDED EVERY SEGMENT RUNS THE SAME PATH (the same entry point, workgroups and convolution).
 * It holds because the tracer noise is a function of the ABSOLUTE step number, the tracer, the system and the seed alone
 * (include/pde.h, TRACER NOISE), every sum is combined in a fixed order, and the magnetisation -- and, on the wide shape, the
 * per-slab sums and sweep maps one step leaves for the next -- is a pure function of the fields, rebuilt from the checkpoint
 * by the same arithmetic.  A checkpoint itself does not depend on the execution shape: one taken on one path may be resumed
 * on another, and the result then agrees with the single launch as closely as the two paths agree on a fresh start.
 * What is NOT part of the state (beta, kernel_sigma, every other field of pde_params) is that of the resuming launch: a launch
 * resumed with another beta is the same scheme with the parameter switched at the checkpoint's step.  L, n_tracers, window
 * and n_systems size the checkpoint and must be those it was taken with.
 *
 * A RESUMED LAUNCH (from != NULL).  rho_p0, rho_m0, tracer_x0, tracer_s0 are not read and may be NULL.  p->nsteps >= 1 is the
 * number of steps of THIS launch.  The launch recomputes the magnetisation of the checkpoint's fields without recording a
 * row (step() needs it), then runs (step, row) nsteps times: rows c + 1 .. c + nsteps.
 *   * Series (m, var, v_eff, D_eff, fft_re, fft_im) have n_rows rows, counted from the launch's first row: nsteps + 1 on a fresh
 *     start, nsteps on a resume.  rand_u / rand_n are [n_systems][n_rows][n_tracers] likewise.
 *   * Snapshots are the rows whose ABSOLUTE number is a multiple of snapshot_interval: n_snap of them, the first being
 *     snapshot first_snap of the run (row first_snap * snapshot_interval).  A launch may hold none; the snapshot pointers
 *     are then ignored.
 *   * The Philox counters and the NaN rule of v_eff / D_eff (row n < window) use the absolute n.
 * pder_extents is this arithmetic; size the buffers with it.
 */
#ifndef PDE_RESUME_H
#define PDE_RESUME_H

#include <stdint.h>

#include "pde.h"
#include "pde_sweep.h"
#include "pde_wide.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The state of n_systems systems between two launches: caller-allocated host arrays. */
typedef struct pde_checkpoint {
    double *rho_p, *rho_m;   /* [n_systems][L] fields of step `step` */
    double *tracer_x;        /* [n_systems][n_tracers] unwrapped, after the move of row `step` */
    int8_t *tracer_s;
    double *hist;            /* [n_systems][window][n_tracers]: slot n % window = positions after the move of row n,
                                for n = max(0, step - window + 1) .. step; the other slots are written as 0 */
    int32_t step;            /* c: steps taken since the run's start */
} pde_checkpoint;
/* tracer_x, tracer_s and hist may be NULL iff n_tracers == 0. */

const char *pder_last_error(void);
const char *pdekr_last_error(void);
const char *pdewr_last_error(void);

/* The rows and snapshots of a launch of p->nsteps steps: a pure host function.  from_step = -1: a fresh start, else the
 * step of the checkpoint the launch resumes.  first_row: the absolute number of the launch's first recorded row (0, or
 * from_step + 1); n_rows: rows recorded; n_snap: snapshots among them (may be 0); first_snap: the run's number of the first
 * of them (its row is first_snap * snapshot_interval; meaningful also when n_snap == 0: the next snapshot to come).  Any
 * output may be NULL.  PDE_ERR_ARG (text: pder_last_error) for from_step < -1, nsteps < 0 (fresh) or < 1 (resumed),
 * snapshot_interval < 1, from_step + nsteps beyond INT32_MAX. */
int pder_extents(const pde_params *p, int32_t from_step, int32_t *first_row, int32_t *n_rows, int32_t *n_snap, int32_t *first_snap);

/* The three solves.  Refused with PDE_ERR_ARG and a text before any device is asked for, next to everything the one-shot
 * entry point refuses: from->step < 0; p->nsteps < 1 on a resume; from->step + p->nsteps beyond INT32_MAX; a NULL rho_p or
 * rho_m in `from` or `to`; a NULL tracer_x, tracer_s or hist in `from` or `to` with n_tracers > 0.  `to` (may be NULL)
 * receives the checkpoint at the launch's last row; `from` and `to` may be the same object. */
int pder_solve(const pde_params *p, int32_t n_systems, const double *beta, const double *rho_p0, const double *rho_m0,
               const double *tracer_x0, const int8_t *tracer_s0, const double *rand_u, const double *rand_n,
               double *rho_p, double *rho_m, double *m_series, double *var_series, double *v_eff_series,
               double *D_eff_series, double *snapshots, double *m_snapshots, double *fft_re, double *fft_im,
               double *tracer_x, int8_t *tracer_s, double *kernel_ms, const pde_checkpoint *from, pde_checkpoint *to);

int pdekr_solve(const pde_params *p, int32_t n_systems, const double *beta, const double *kernel_sigma,
                const double *rho_p0, const double *rho_m0, const double *tracer_x0, const int8_t *tracer_s0,
                const double *rand_u, const double *rand_n,
                double *rho_p, double *rho_m, double *m_series, double *var_series, double *v_eff_series,
                double *D_eff_series, double *snapshots, double *m_snapshots, double *fft_re, double *fft_im,
                double *tracer_x, int8_t *tracer_s, double *kernel_ms, const pde_checkpoint *from, pde_checkpoint *to);

int pdewr_solve(const pde_params *p, int32_t n_systems, int32_t workgroups, const double *beta, const double *rho_p0,
                const double *rho_m0, const double *tracer_x0, const int8_t *tracer_s0, const double *rand_u, const double *rand_n,
                double *rho_p, double *rho_m, double *m_series, double *var_series, double *v_eff_series,
                double *D_eff_series, double *snapshots, double *m_snapshots, double *fft_re, double *fft_im,
                double *tracer_x, int8_t *tracer_s, double *kernel_ms, const pde_checkpoint *from, pde_checkpoint *to);

#ifdef __cplusplus
}
#endif
#endif /* PDE_RESUME_H */
