/* gillespie_mixed_many.h -- C ABI of the exact event loop for MIXED BATCHES OF LARGE SYSTEMS (part of libaps_hip.so).
 *
 * gilx_run (include/gillespie_mixed.h) puts systems that differ in the interaction range and in the blocking table into one
 * launch, but only systems that fit one workgroup's LDS (L <= GIL_MAX_L, n_cap <= GIL_MAX_N).  gilm_run
 * (include/gillespie_many.h) runs systems beyond that, with one table for the whole launch.  Here the large-system kernel of
 * gilm_run -- one persistent workgroup of 1024 threads per system, state in global memory -- takes a VARIANT per system
 * (struct gilx_variants, reused unchanged): a sigma sweep or a density x beta sweep at L = 8192 is one launch that fills the
 * device, where a loop of gilm_run launches occupies as many compute units as one sigma or one particle number has systems.
 *
 * Same dynamics, parameters (gil_params, reused unchanged; p->sigma_grid and p->block_table are IGNORED here), buffers and
 * error codes as include/gillespie.h.  WHAT A SYSTEM COMPUTES: system s produces, bit for bit in every output (times
 * included), what gilm_run computes for a system with the same start state and beta in a launch with its variant's sigma_grid
 * and block_table, the same n_cap, and Philox key seed[s], stream stream[s].  The V weight tables are built one by one by the
 * host code that builds gilx_run's, so their bits are those of such a launch.  Rate sums are grouped as gilm_run groups them:
 * blocks of 256 slots over n_cap, ceil(n_blocks / 1024) blocks per thread of the 1024-thread scan.
 *
 * n_cap: a system's numbers do not depend on n_cap as long as both launches have at most 1024 rate blocks
 * (n_cap <= 262144, one block per thread): the slots at and beyond n0[s] carry rate 0, so a block sum and the scan over the
 * 1024 threads only ever add trailing zeros, and the draws depend on the event index alone.  A system of a mixed launch with
 * the launch's n_cap therefore equals, bit for bit, the gilm_run system with any n_cap of its own under that condition
 * (pos_obs / sigma_obs / flags_obs / exits keep the stride of the launch they came from).
 *
 * Random numbers: system s draws with the Philox key v->seed[s] (NULL: (p->seed + s) mod 2^64, the sum taken in 64 bits as
 * gilm_run takes it) and v->stream[s] in counter word 2 (NULL: 0), whichever workgroup takes it.  One variant with these
 * defaults is gilm_run itself.  The defaults differ from gilx_run's (p->seed, s) on purpose: each follows its own shape's
 * single-launch convention.  Counters, domain constants and the conversion to the four numbers of an event:
 * include/gillespie.h, RANDOM NUMBERS.
 *
 * The weight table of a variant lies in LDS when its table_len + 1 entries fit the 10000 kept there, decided per system; the
 * LDS region is sized for the longest such table of the launch.  A variant with a longer table reads it from global memory,
 * as in gilm_run; both kinds may share a launch.
 *
 * Outputs are indexed by the SYSTEM, never by the workgroup, with the strides of gilm_run (n_cap per system).
 * All functions return 0 on success and a negative code on failure; gilxm_last_error() gives the text.
 */
#ifndef GILLESPIE_MIXED_MANY_H
#define GILLESPIE_MIXED_MANY_H

#include <stdint.h>

#include "gillespie.h"
#include "gillespie_many.h"
#include "gillespie_mixed.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gilxm_plan_info {
    int32_t n_systems;
    int32_t n_blocks;           /* rate blocks of 256 particle slots: ceil(n_cap / 256) */
    int32_t max_tlen;           /* length of the longest weight table (taps without the closing zero) */
    int32_t max_tlen_lds;       /* length of the longest table kept in LDS (table_len + 1 <= 10000); -1: no variant's is */
    int32_t n_global;           /* variants whose table is read from global memory */
    int32_t lds_bytes;          /* dynamic LDS of one workgroup: 8 * (max_tlen_lds >= 0 ? max_tlen_lds + 2 rounded down to even : 0)
                                   + 8 * (32 + 4 * 1024 + 4 + GIL_NSCALARS) + 4 * (2 * n_blocks + 32): gilm_plan's for that table */
    int64_t table_doubles;      /* all V tables back to back, each with its closing zero */
    int64_t work_bytes_per_system;   /* as gilm_plan: n_cap * 21 + L * 24 + L * K * 4 + n_blocks * 8 */
    int64_t output_bytes;            /* device copies of the outputs: n_systems * (n_obs * n_cap * 6 when states are wanted
                                        + n_obs * GIL_NSCALARS * 8 + n_cap * 24 (exit log) + 24) */
} gilxm_plan_info;

const char *gilxm_last_error(void);

/* What gilxm_run would use: pure host arithmetic, no device is touched.  Needs of p: L, K, periodic, n_systems, n_cap, n_obs;
 * of v: n_variants and sigma_grid (variant_of_system and order are checked when given).  Limits are gilm_run's: L in
 * [2, 2^25], K in [1, 32], L * K <= 2^27, n_cap in [1, 2^20], n_systems in [1, GILM_MAX_SYSTEMS].  Refuses what gilxm_run
 * refuses on these numbers, naming the offending value: a number beyond those limits, n_variants outside [1, 4096], a variant
 * index outside [0, V), a negative or non-finite sigma_grid, an order that is no permutation, a launch beyond 160 KB of LDS,
 * and a batch whose n_systems * work_bytes_per_system + output_bytes exceeds 2^38 bytes (gilxm_run compares with the free
 * device memory). */
int gilxm_plan(const gil_params *p, const gilx_variants *v, int32_t want_states, gilxm_plan_info *out);

/* The arguments are those of gilx_run, in its order, with the meaning they have in gilm_run; any output may be NULL.
 * v->order NULL: falling n0, ties by index. */
int gilxm_run(const gil_params *p, const gilx_variants *v,
              const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0, const double *uniforms,
              int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs, int32_t *n_recorded,
              int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* GILLESPIE_MIXED_MANY_H */
