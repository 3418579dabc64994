/* gillespie_mixed.h -- C ABI of the exact event loop for MIXED BATCHES (part of libaps_hip.so).
 *
 * gil_run_batch (include/gillespie.h) takes systems that differ in beta, initial state and particle number; the interaction
 * range -- and with it the weight table, its length and the global-mean mode -- and the blocking table behind the `blocked`
 * sum are one value per launch.  Two of the reference's drivers sweep exactly those: the sigma sweep
 * (PARTICLE_solver_BIOLOGY_EXCLUSION_sweep_beta_2.py:1030-1075) and the density x beta double sweep (..._double_sweep.py:851-861,
 * where the blocking threshold follows the particle number).  Here every system refers to one of V VARIANTS, a variant being a
 * sigma_grid and a blocking table, and the whole sweep is one launch.  L, K, periodic, the rates, the anchors and the flip table
 * are the launch's.
 *
 * Same dynamics, parameters (gil_params, reused unchanged; p->sigma_grid and p->block_table are IGNORED here), buffers and error
 * codes as include/gillespie.h.  What a system computes is what gil_run_batch computes for it in a launch with its variant's
 * sigma_grid and block_table, Philox key seed[s] and system index stream[s]: the V weight tables are built one by one by the
 * same host code, so their bits are those of such a launch.  One difference: a system's rate sums are grouped by its own slot
 * count, chunk = ceil(n0[s] / threads), where gil_run_batch groups by n_cap; the total rate can differ in its last bit between
 * the two when n0[s] < n_cap or the thread counts differ, and the times with it (1e-16 relative per event).
 *
 * Random numbers: system s draws with the Philox key v->seed[s] (both 32-bit halves; NULL: p->seed for every system) and the
 * stream v->stream[s] in counter word 2 (NULL: s), whichever workgroup takes it (`order` does not enter).  Two systems may share
 * a stream number under different keys, or a key under different streams; the same (key, stream) pair twice gives the same
 * numbers twice.  gilxs_run (include/gillespie_mixed_structure.h) draws the same way.  Counters, domain constants and the
 * conversion to the four numbers of an event: include/gillespie.h, RANDOM NUMBERS.
 *
 * Outputs are indexed by the SYSTEM, never by the workgroup, with the strides of gil_run_batch (n_cap per system).  A system's
 * loops run over its own n0[s] slots; the slots at and beyond n0[s] are zero in pos_obs, sigma_obs and flags_obs.
 * The large-system shape (gilm_run) takes no mixed batches through these functions; its own mixed launch is gilxm_run of
 * include/gillespie_mixed_many.h.
 * All functions return 0 on success and a negative code on failure; gilx_last_error() gives the text.
 */
#ifndef GILLESPIE_MIXED_H
#define GILLESPIE_MIXED_H

#include <stdint.h>

#include "gillespie.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GILX_MAX_VARIANTS 4096  /* n_variants is in [1, GILX_MAX_VARIANTS] */

typedef struct gilx_variants {
    int32_t n_variants;                 /* V */
    int32_t reserved;
    const double *sigma_grid;           /* [V], each finite and >= 0; 0 selects the global mean field for the variant's systems */
    const uint8_t *block_table;         /* [V][(K+1)*(K+1)] or NULL: gil_params.block_table of each variant */
    const int32_t *variant_of_system;   /* [n_systems], each in [0, V) */
    const uint64_t *seed;               /* [n_systems] or NULL: Philox key of a system; NULL: p->seed for all */
    const int32_t *stream;              /* [n_systems] or NULL: the system index in the Philox counter; NULL: s */
    const int32_t *order;               /* [n_systems] or NULL: order[b] is the system workgroup b takes, a permutation of
                                           0 .. n_systems - 1.  NULL: falling n0 (ties by index) -- workgroups start roughly in
                                           block order, and the long systems should start first when more are queued than fit */
} gilx_variants;

typedef struct gilx_plan_info {
    int32_t threads;            /* per system: 64 while n_cap <= 1024, else 256 */
    int32_t lds_bytes;          /* dynamic LDS of one workgroup: gil_run_batch's for the longest table of the batch */
    int32_t max_tlen;           /* length of the longest weight table (taps without the closing zero) */
    int32_t systems_per_cu;     /* by LDS: 160 KB / lds_bytes */
    int64_t table_doubles;      /* all V tables back to back, each with its closing zero */
    int64_t output_bytes;       /* device copies of the outputs: n_systems * (n_obs * n_cap * 6 when states are wanted
                                   + n_obs * GIL_NSCALARS * 8 + n_cap * 24 (exit log) + 24) */
} gilx_plan_info;

const char *gilx_last_error(void);

/* What gilx_run would use: pure host arithmetic, no device is touched.  Needs of p: L, K, periodic, n_systems, n_cap, n_obs; of
 * v: n_variants and sigma_grid (variant_of_system and order are checked when given).  Refuses what gilx_run refuses on these
 * numbers, naming the offending value: n_variants outside [1, 4096], a variant index outside [0, V), a negative or non-finite
 * sigma_grid, an order that is no permutation, a launch beyond 160 KB of LDS, and L > GIL_MAX_L or n_cap > GIL_MAX_N (the
 * large-system shape takes no mixed batches). */
int gilx_plan(const gil_params *p, const gilx_variants *v, int32_t want_states, gilx_plan_info *out);

/* The arguments from n0 to n_exits are those of gil_run_batch, in its order, with the same meaning; any output may be NULL. */
int gilx_run(const gil_params *p, const gilx_variants *v,
             const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0, const double *uniforms,
             int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs, int32_t *n_recorded,
             int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* GILLESPIE_MIXED_H */
