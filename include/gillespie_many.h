/* gillespie_many.h -- C ABI of the exact event loop for MANY LARGE systems in one launch (part of libaps_hip.so).
 *
 * Same dynamics, parameters (gil_params, reused unchanged), buffers and error codes as include/gillespie.h.  The two
 * shapes there leave a gap: the batch kernel needs a system to fit one workgroup's LDS, the large-system kernel takes one
 * system per call and records no sums.  Here a batch of systems of the large kind -- state in global memory, one
 * persistent workgroup of 1024 threads each, the kernel of the large-system entry point -- runs as one grid of independent
 * workgroups, and the twelve scalar sums of the batch kernel are taken on the device at every observation.  No
 * workgroup waits on another: a batch with more systems than the device has compute units queues.
 *
 * Random numbers: system s uses the Philox key (p->seed + s) mod 2^64 -- the sum is taken in 64 bits, so it carries into the key's
 * high word and wraps to 0 past 2^64 - 1 -- and the counters of the large-system entry point with stream 0 (counter word 2), so
 * system s of a batch is, bit for bit, the single large run with seed p->seed + s (and the same n_cap).  Systems of one batch
 * therefore differ in the KEY, not in the stream; two batches whose seeds are closer than their sizes share systems.  The
 * counters, the two domain constants and the conversion to the four numbers of an event: include/gillespie.h, RANDOM NUMBERS.
 * All functions return 0 on success and a negative code on failure; gilm_last_error() gives the text.
 */
#ifndef GILLESPIE_MANY_H
#define GILLESPIE_MANY_H

#include <stdint.h>

#include "gillespie.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GILM_MAX_SYSTEMS 65535

typedef struct gilm_plan_info {
    int32_t n_systems;
    int32_t n_blocks;           /* rate blocks of 256 particle slots: ceil(n_cap / 256) */
    int32_t table_len;          /* non-zero taps of the weight table (0: global mean field) */
    int32_t table_in_lds;       /* 1 when the table_len + 1 entries fit the 10000 kept in LDS, else read from global memory */
    int32_t lds_bytes;          /* dynamic LDS of one workgroup: 8 * (table in LDS ? table_len + 2 rounded down to even : 0)
                                   + 8 * (32 + 4 * 1024 + 4 + GIL_NSCALARS) + 4 * (2 * n_blocks + 32) */
    int32_t reserved;
    int64_t work_bytes_per_system;   /* n_cap * 21 (pos, work list, reference positions: int; flags: byte; rate: double)
                                        + L * 24 (occ, occp: int; W, S: double) + L * K * 4 (site map) + n_blocks * 8 (block sums) */
    int64_t output_bytes;            /* device copies of the outputs: n_systems * (n_obs * n_cap * 6 when states are wanted
                                        + n_obs * GIL_NSCALARS * 8 when scalars are wanted + n_cap * 24 (exit log) + 24) */
} gilm_plan_info;

const char *gilm_last_error(void);

/* What gilm_run would use for these parameters (p->n_systems systems): pure host arithmetic, no device is touched.
 * Refuses what gilm_run would refuse on the parameters alone, and a batch whose
 * n_systems * work_bytes_per_system + output_bytes exceeds 2^38 bytes (gilm_run compares with the free device memory). */
int gilm_plan(const gil_params *p, int32_t want_states, int32_t want_scalars, gilm_plan_info *out);

/* Arguments as in the batch entry point of gillespie.h, in the same order, with the same meaning: inputs [n_systems][n_cap],
 * uniforms [n_systems][max_events][4] or NULL, pos_obs / sigma_obs / flags_obs [n_systems][n_obs][n_cap],
 * scalars_obs [n_systems][n_obs][GIL_NSCALARS], exits [n_systems][n_cap][3]; x_wall, ref_obs, front_lo and block_table of
 * gil_params are used by the scalar sums.  Any output may be NULL; without state pointers only the sums leave the device.
 * Limits: L in [2, 2^25], L * K <= 2^27, n_cap <= 2^20, 1 <= n_systems <= GILM_MAX_SYSTEMS.  A batch whose work and
 * output bytes exceed the free device memory is refused with GIL_ERR_ARG and a text that gives the numbers. */
int gilm_run(const gil_params *p, const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0,
             const double *uniforms, int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs,
             int32_t *n_recorded, int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, double *kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* GILLESPIE_MANY_H */
