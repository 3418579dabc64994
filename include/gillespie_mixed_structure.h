/* gillespie_mixed_structure.h -- C ABI of the exact event loop for MIXED BATCHES WITH STRUCTURE SUMS and their WINDOW
 * REDUCTION on the device (part of libaps_hip.so).
 *
 * The study this combines: how the pattern observables of PARTICLE_solver_BIOLOGY_local_structure.py:55-103 (var(total), the
 * Fourier amplitudes, the dominant mode, the low-k power, the local-magnetisation variance) and the series var(t), |m|(t)
 * depend on the interaction range -- the particle counterpart of the PDE width sweep (include/pde_sweep.h).  gils_run
 * (include/gillespie_structure.h) takes the sums for one interaction range per launch and returns a row of 4 + 2 k_max doubles
 * per system and observation; gilx_run (include/gillespie_mixed.h) runs systems of different ranges in one launch, without the
 * sums.  gilxs_run is gilx_run with the sums of gils_run, and it reduces them over the window of observations where they are
 * formed, so that nothing of size n_obs x k_max has to leave the device.
 *
 * Dynamics, parameters, Philox keys, launch order, variants and the outputs from pos_obs to n_exits: those of gilx_run.  A row:
 * that of gils_run, with the system's own table and field mode (a variant with sigma_grid = 0 carries the global mean on every
 * site).  One variant is the uniform batch: the window reduction without mixing.
 *
 *   head_obs[s][k][0..3]   n, sum occ^2, sum m, sum m^2 of EVERY observation the loop recorded, from 0 on (32 bytes each): row
 *                          entries 0..3, so var(t) needs no rows
 *   window[s][j][0..2]     for mode j < k_max, over the observations k >= first_obs the loop recorded that had a live particle:
 *                          a0_j, sum_t d_j(t), sum_t d_j(t)^2   with a_j(t) = sqrt(re^2 + im^2) / n_t (three roundings and a
 *                          division; the library is compiled without contraction), a0_j = a_j at the first such observation,
 *                          d_j(t) = a_j(t) - a0_j.  Shifted, so that mean = a0 + sum d / M and the ddof = 1 spread
 *                          (sum d^2 - (sum d)^2 / M) / (M - 1) are free of the cancellation of sum a^2 - (sum a)^2 / M, and a
 *                          constant mode (mode 0) has spread 0 exactly.  Accumulated by the one thread that owns the mode, in
 *                          observation order: deterministic, no atomics.
 *   n_window[s]            the observations accumulated
 *   n_empty[s]             window observations without a live particle: they add nothing
 * All functions return 0 on success and a negative code on failure; gilxs_last_error() gives the text.
 */
#ifndef GILLESPIE_MIXED_STRUCTURE_H
#define GILLESPIE_MIXED_STRUCTURE_H

#include <stdint.h>

#include "gillespie.h"
#include "gillespie_mixed.h"
#include "gillespie_structure.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gilxs_plan_info {
    int32_t threads;            /* per system: 64 while n_cap <= 1024, else 256 */
    int32_t lds_bytes;          /* dynamic LDS of one workgroup: gils_plan's for the longest table of the batch */
    int32_t phase_in_lds;       /* 1 when every workgroup keeps a copy of the phase table (L * 16 bytes) in LDS */
    int32_t max_tlen;           /* length of the longest weight table (taps without the closing zero) */
    int32_t systems_per_cu;     /* by LDS: 160 KB / lds_bytes */
    int32_t row_len;            /* 4 + 2 * k_max */
    int64_t work_bytes;         /* device scratch of the whole batch: the phase table, L * 16 */
    int64_t output_bytes;       /* device copies of the outputs: gilx_plan's, plus n_systems * (n_obs * 32 (head rows)
                                   + k_max * 24 (window) + 8), plus n_systems * n_obs * row_len * 8 when rows are wanted */
} gilxs_plan_info;

const char *gilxs_last_error(void);

/* What gilxs_run would use: pure host arithmetic, no device is touched.  Needs of p and v what gilx_plan needs.  Refuses what
 * gilx_plan refuses, and, naming the offending value: k_max outside [1, min(L, GILS_MAX_K)], first_obs outside [0, n_obs], a
 * launch beyond 160 KB of LDS, and a batch whose work_bytes + output_bytes exceed 2^38 (gilxs_run compares with the free
 * device memory). */
int gilxs_plan(const gil_params *p, const gilx_variants *v, int32_t k_max, int32_t first_obs, int32_t want_states,
               int32_t want_rows, gilxs_plan_info *out);

/* The arguments from n0 to n_exits are those of gilx_run, in its order, with the same meaning; any of its outputs may be NULL.
 * structure_obs [n_systems][n_obs][4 + 2 k_max] may be NULL: then no row is stored.  Rows of observations before first_obs
 * and of observations the loop never reached are zero, as in gils_run.  head_obs [n_systems][n_obs][4], window
 * [n_systems][k_max][3], n_window and n_empty [n_systems] are required. */
int gilxs_run(const gil_params *p, const gilx_variants *v, int32_t k_max, int32_t first_obs,
              const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0, const double *uniforms,
              int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs, int32_t *n_recorded,
              int64_t *n_events, double *t_final, double *exits, int32_t *n_exits,
              double *structure_obs, double *head_obs, double *window, int32_t *n_window, int32_t *n_empty, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* GILLESPIE_MIXED_STRUCTURE_H */
