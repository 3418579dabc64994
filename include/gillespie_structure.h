/* gillespie_structure.h -- C ABI of the exact event loop WITH STRUCTURE SUMS taken on the device (part of libaps_hip.so).
 *
 * Same dynamics, parameters (gil_params, reused unchanged), buffers and error codes as include/gillespie.h.  The
 * reference's pattern / structure study (PARTICLE_solver_BIOLOGY_local_structure.py:55-103, driver :671-753) needs, per
 * observation, var(total), |fft(total)| and the local magnetisation over the lattice; the reference keeps three M x L
 * arrays per run for them.  Here the event-loop kernels reduce them where the state lives, at every observation from
 * `first_obs` on, to one row of 4 + 2 k_max doubles -- the layout of aps_observe_structure (include/aps.h):
 *   [0] live particles n                      [1] sum over sites of occ[x]^2          (integers, exact in binary64)
 *   [2] sum over the L sites of m(x)          [3] sum over the L sites of m(x)^2
 *   [4 + 2k], [5 + 2k]  Re, Im of sum over live particles of exp(-2 pi i k pos / L),  k = 0 .. k_max - 1
 * m(x) = clip(S[x] / W[x], -1, 1) where W[x] > 0 and 0 elsewhere (the field the rates use: of the observed state); with the
 * global mean field (sigma_grid = 0) every site carries sum sigma / n.
 *
 * gils_run picks the shape by the limits of gillespie.h: a system with L <= GIL_MAX_L and n_cap <= GIL_MAX_N that fits the
 * 160 KB of LDS runs in the batch kernel (Philox counter (event, system), as gil_run_batch); any other in the large-system
 * kernel with its limits and its key rule (system s: key seed + s, as gilm_run of gillespie_many.h).  Recording changes
 * nothing else: states, scalar sums, event counts and times are those of gil_run_batch / gilm_run for the same arguments.
 * All functions return 0 on success and a negative code on failure; gils_last_error() gives the text.
 */
#ifndef GILLESPIE_STRUCTURE_H
#define GILLESPIE_STRUCTURE_H

#include <stdint.h>

#include "gillespie.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GILS_MAX_K 4096         /* k_max is in [1, min(L, GILS_MAX_K)] */
#define GILS_SHAPE_BATCH 0      /* the system in one workgroup's LDS (gil_run_batch's kernel) */
#define GILS_SHAPE_LARGE 1      /* the state in global memory, 1024 threads (gilm_run's kernel) */

typedef struct gils_plan_info {
    int32_t shape;              /* GILS_SHAPE_* */
    int32_t threads;            /* per system: 64 (n_cap <= 1024) or 256 in the batch shape, 1024 in the large shape */
    int32_t lds_bytes;          /* dynamic LDS of one workgroup: the loop's own, rounded up to 8, plus
                                   8 * (4 * threads / 64 + (threads > 64 ? 2 * threads : 0)) for the sums, plus L * 16 when
                                   phase_in_lds */
    int32_t row_len;            /* 4 + 2 * k_max */
    int32_t phase_in_lds;       /* batch shape: 1 when every workgroup keeps a copy of the phase table (L * 16 bytes) in LDS,
                                   which it does whenever the 160 KB leave room for it; 0: gathered from global memory */
    int32_t reserved;
    int64_t work_bytes;         /* device scratch of the whole batch: the phase table L * 16, plus in the large shape
                                   n_systems * work_bytes_per_system of gilm_plan_info */
    int64_t output_bytes;       /* device copies of the outputs: n_systems * (n_obs * n_cap * 6 when states are wanted
                                   + n_obs * GIL_NSCALARS * 8 + n_cap * 24 (exit log) + 24 + n_obs * row_len * 8) */
} gils_plan_info;

const char *gils_last_error(void);

/* What gils_run would use for these parameters: pure host arithmetic, no device is touched.  Refuses what gils_run
 * refuses on the parameters alone (k_max outside [1, min(L, GILS_MAX_K)], first_obs outside [0, n_obs], the limits of the
 * shape), and a batch whose work_bytes + output_bytes exceed 2^38 (gils_run compares with the free device memory). */
int gils_plan(const gil_params *p, int32_t k_max, int32_t first_obs, int32_t want_states, gils_plan_info *out);

/* Arguments after first_obs as in gil_run_batch, in the same order, with the same meaning; any output of those may be
 * NULL.  structure_obs [n_systems][n_obs][4 + 2 k_max] is required (without it, use gil_run_batch / gilm_run): rows of
 * observations before first_obs and of observations the loop never reached (n_recorded) are zero, and no Fourier work
 * is done for them. */
int gils_run(const gil_params *p, int32_t k_max, int32_t first_obs,
             const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0, const double *uniforms,
             int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs, int32_t *n_recorded,
             int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, double *structure_obs, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* GILLESPIE_STRUCTURE_H */
