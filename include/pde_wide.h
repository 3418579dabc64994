/* pde_wide.h -- C ABI of the wide shape of the hydrodynamic-limit solver (part of libaps_hip.so).
 *
 * Same scheme, parameters, buffers and error codes as include/pde.h; a different execution shape.  pde_solve_batch runs
 * one persistent workgroup per system, which suits many small systems.  Here the L sites of ONE system are cut into
 * `workgroups` contiguous slabs (the first L % workgroups of them one site longer), one workgroup per slab, a batch is a
 * grid of (workgroups, n_systems), and a time step is a short chain of kernel launches on one stream: what crosses slabs
 * (the two sweeps of the implicit diffusion, the reach of the Gaussian kernel, every sum) is handed over at a kernel
 * boundary.  No workgroup waits on another.  Sums are combined from per-slab partials in a fixed order: a call repeated
 * gives the same bits, and a system's result does not depend on its place in a batch.
 * Tracer noise: the counters, key, conversion and rows of include/pde.h (TRACER NOISE), whatever the number of slabs.
 * All functions return 0 on success and a negative code on failure; pdew_last_error() gives the text.
 */
#ifndef PDE_WIDE_H
#define PDE_WIDE_H

#include <stdint.h>

#include "pde.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PDEW_MAX_WORKGROUPS 4096          /* slabs per system */
#define PDEW_MIN_SLAB 4                   /* sites in the shortest slab */
#define PDEW_MAX_GRID (1 << 20)           /* workgroups * n_systems: what the arrays of per-slab partials are sized for */
#define PDEW_AUTO_SLAB 256                /* workgroups = 0 chooses ceil(L / PDEW_AUTO_SLAB) slabs */

typedef struct pdew_plan_info {
    int32_t workgroups;         /* G: slabs per system */
    int32_t slab_len;           /* sites in the longest slab: ceil(L / G) */
    int32_t slab_len_min;       /* sites in the shortest slab: floor(L / G) */
    int32_t n_long_slabs;       /* L % G: the first so many slabs have slab_len sites, the others slab_len_min (all, when 0) */
    int32_t ktaps;              /* reach of the Gaussian kernel in sites (0 unless kernel_mode == 1) */
    int32_t launches_per_step;  /* kernel launches enqueued per time step */
    int32_t lds_bytes;          /* direct: dynamic LDS of the magnetisation kernel; spectral: LDS of a transform kernel */
    int32_t conv_log2;          /* m: the spectral convolution transforms 2^m words per block (0 when no transform runs) */
    int64_t work_bytes;         /* global working memory: fields, per-slab partials and maps, tracer ring (not inputs / outputs) */
} pdew_plan_info;

const char *pdew_last_error(void);

/* What pdew_solve would use for these parameters: no device is touched, nothing is launched.
 * workgroups = 0 lets the library choose.  p->convolution: 0 or 1; launches_per_step, lds_bytes and work_bytes describe the
 * chosen path. */
int pdew_plan(const pde_params *p, int32_t n_systems, int32_t workgroups, pdew_plan_info *out);

/* pde_solve_batch on the wide shape.  The buffer arguments are those of pde_solve_batch, in the same order, with the same
 * meaning, with one difference: with n_tracers == 0, v_eff_series and D_eff_series are left as the caller passed them
 * (pde_solve_batch and pdek_solve overwrite them with unspecified values).  workgroups = G per system (0: the library chooses); 1 <= G <= PDEW_MAX_WORKGROUPS, floor(L / G) >= PDEW_MIN_SLAB,
 * G * n_systems <= PDEW_MAX_GRID, n_systems <= 65535.
 * p->convolution (used with kernel_mode 1 only): 0 = direct circular convolution, 1 = spectral (include/pde_spectral.h; a kernel of one
 * tap, ktaps == 0, is summed directly and conv_log2 is 0: its one product is exact, a transform's round-off is not); a shape
 * the spectral path cannot take fails with PDE_ERR_ARG and a text that says why -- there is no fall-back to the direct sum. */
int pdew_solve(const pde_params *p, int32_t n_systems, int32_t workgroups, const double *beta, const double *rho_p0,
               const double *rho_m0, const double *tracer_x0, const int8_t *tracer_s0, const double *rand_u, const double *rand_n,
               double *rho_p, double *rho_m, double *m_series, double *var_series, double *v_eff_series,
               double *D_eff_series, double *snapshots, double *m_snapshots, double *fft_re, double *fft_im,
               double *tracer_x, int8_t *tracer_s, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* PDE_WIDE_H */
