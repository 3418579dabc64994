/* pde_spectral.h -- C ABI of the plan rule of the spectral convolution of the wide shape (part of libaps_hip.so).
 *
 * pdew_solve with pde_params.convolution = 1 evaluates the Gaussian-kernel magnetisation (kernel_mode 1) by the convolution
 * theorem instead of the direct sum: complex binary64 transforms of length 2^m over overlap-save blocks of the ring.  Block
 * b owns the sites [b S, min(L, (b + 1) S)), transforms the window of its sites +- ktaps (taken mod L) and writes the
 * magnetisation of its own sites only.  This header gives the rule that cuts the ring; it needs no device.
 *
 *   cap = min(max_log2, 21).  One block if L + 2 ktaps <= 2^cap.  Otherwise the shape is eligible only if
 *   2 ktaps <= 2^cap / 2; then B = ceil(L / (2^cap - 2 ktaps)), S = ceil(L / B), B = ceil(L / S).
 *   m is the smallest value with 2^m >= S + 2 ktaps, and never below 8.
 *
 * pdew_solve takes max_log2 from the environment variable PDE_SPECTRAL_MAX_LOG2 (default 21) and further requires
 * B * n_systems <= 65535.  Both functions return as those of include/pde.h do: 0 or a negative code, the text from
 * pdes_last_error().
 */
#ifndef PDE_SPECTRAL_H
#define PDE_SPECTRAL_H

#include <stdint.h>

#include "pde.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *pdes_last_error(void);

/* blocks = B, log2_m = m, block_sites = S for a ring of L sites and a kernel reaching ktaps sites either side
 * (0 <= ktaps <= L / 2).  PDE_ERR_ARG with a text when the shape is not eligible. */
int pdes_plan(int32_t L, int32_t ktaps, int32_t max_log2, int32_t *blocks, int32_t *log2_m, int32_t *block_sites);

#ifdef __cplusplus
}
#endif
#endif /* PDE_SPECTRAL_H */
