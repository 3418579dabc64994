/* pde_sweep.h -- C ABI of the kernel-width sweep of the hydrodynamic-limit solver (part of libaps_hip.so).
 *
 * Same scheme, parameters, buffers and error codes as include/pde.h, same execution shape as pde_solve_batch (one persistent
 * workgroup per system, the state in LDS), but every system has its OWN kernel width next to its own beta: the reference's
 * kernel-sigma sweeps (IMEX_PDE_solver_run_sweep_magn.py:55-85, ..._magn2.py) are one launch.  For kernels that span a large
 * part of the ring the magnetisation can be evaluated by a complex binary64 transform held in the workgroup's LDS
 * (p->convolution == 1), O(M log M) per step instead of O(L * reach).
 *
 * Mode of system s, the rule of the Python class: p->kernel_mode == 0 -> every system uses the local ratio (kernel_sigma may
 * be NULL); otherwise global mean (mode 2) when kernel_sigma[s] > 100000, else the periodic Gaussian kernel (mode 1) with its
 * own normalised taps, cut at 1e-17 of the centre tap, the antipodal tap of an even ring halved.
 *
 * Transform (p->convolution == 1, every mode-1 system whose kernel reaches beyond its own site, kt >= 1): the window
 * z[(i - kt) mod L], i < L + 2 kt, z = s + i tot, zero up to M = 2^m, m = max(PDEK_MIN_LOG2, ceil(log2(L + 2 kt))); forward,
 * product with the taps' real spectrum, inverse; outputs
 * kt .. kt + L - 1 are kept.  Upper limit: PDEK_MAX_LOG2 and PDEK_LDS_LIMIT.  The launch's LDS is, in bytes,
 *     8 * ((5 L + ((ktaps_max + 2) & ~1) + 259) & ~3) + 16384        fields, taps, sums, the scans' scratch (as pde_solve_batch)
 *   + 33 * M_max                                                      buffer of M words padded by one in sixteen, M / 2 twiddles, M spectrum values
 * M = 2048 takes 67 584 bytes and fits while 5 L + ktaps <= 9 720 or so (L = 1900 with ktaps = 74); M = 4096 would take 135 168 and
 * leave room for no L that needs it.  So L + 2 ktaps <= 2048: a ring-wide kernel (ktaps = L / 2) is eligible up to L = 1024, the
 * reference drivers' L = 1000 included.  A shape beyond that, or one whose fields would have to live in global memory
 * (L > ~2900: the ground of include/pde_wide.h), is refused with PDE_ERR_ARG and a text containing "eligible" by both
 * functions; there is no fall-back.
 * Tracer noise: the counters, key, conversion and rows of include/pde.h (TRACER NOISE); `sys` is the system's index in the sweep.
 * All functions return 0 on success and a negative code on failure; pdek_last_error() gives the text.
 */
#ifndef PDE_SWEEP_H
#define PDE_SWEEP_H

#include <stdint.h>

#include "pde.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PDEK_MIN_LOG2 8                   /* smallest transform: 256 words */
#define PDEK_MAX_LOG2 11                  /* largest transform that fits LDS next to the fields: 2048 words */
#define PDEK_LDS_LIMIT (160 * 1024)       /* bytes of LDS one workgroup may use */

typedef struct pdek_plan_info {
    int32_t ktaps_max;          /* largest reach among the systems, in sites: sizes the taps' place in LDS */
    int32_t conv_log2_max;      /* largest m among the systems (0: no transform runs): sizes the transform's place in LDS */
    int32_t lds_bytes;          /* dynamic LDS of the launch */
    int32_t fields_in_lds;      /* 1: the five fields of a system live in LDS (always, for an eligible shape) */
} pdek_plan_info;

const char *pdek_last_error(void);

/* What pdek_solve would use: a pure host function, no device is touched.  kernel_sigma[n_systems] (may be NULL when
 * p->kernel_mode == 0); info and the three arrays [n_systems] may each be NULL.  conv_log2[s] is 0 where no transform runs
 * (p->convolution == 0, the system's mode is not 1, or its kernel is one tap: ktaps[s] == 0, where the direct sum is one exact
 * product and a transform's round-off, divided by den + 1e-12 on an empty site, would only lose accuracy).  A kernel_sigma
 * that is not finite or not > 0 where a Gaussian kernel
 * is asked for is refused. */
int pdek_plan(const pde_params *p, int32_t n_systems, const double *kernel_sigma,
              pdek_plan_info *info, int32_t *kernel_mode, int32_t *ktaps, int32_t *conv_log2);

/* pde_solve_batch with a kernel width per system: kernel_sigma[n_systems] replaces p->kernel_sigma; the 19 buffers and
 * kernel_ms are those of pde_solve_batch, in the same order, with the same meaning.  p->convolution: 0 = the direct circular
 * sum over the system's own taps (the arithmetic of pde_solve_batch), 1 = the transform for every mode-1 system with
 * ktaps >= 1.  Uses exactly
 * the plan of pdek_plan.  A system's result depends on its own parameters and (device-side tracer noise) on its index, not
 * on its companions in the launch. */
int pdek_solve(const pde_params *p, int32_t n_systems, const double *beta, const double *kernel_sigma,
               const double *rho_p0, const double *rho_m0, const double *tracer_x0, const int8_t *tracer_s0,
               const double *rand_u, const double *rand_n,
               double *rho_p, double *rho_m, double *m_series, double *var_series, double *v_eff_series,
               double *D_eff_series, double *snapshots, double *m_snapshots, double *fft_re, double *fft_im,
               double *tracer_x, int8_t *tracer_s, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* PDE_SWEEP_H */
