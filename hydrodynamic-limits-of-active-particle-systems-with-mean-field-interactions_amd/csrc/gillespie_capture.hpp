// gillespie_capture.hpp -- device side of include/gillespie_capture.h: the anchor-capture and cluster statistics of
// PARTICLE_solver_CLASS.py:766-976 (plot_individuals: cluster sizes, bound-state lifetimes, exits per anchor) taken inside
// the exact event loop.  One set of device functions, called by the capture instantiations of both loop kernels
// (gillespie_hip.hip: the system in LDS, 64 or 256 threads; gillespie_big_hip.hip: the state in global memory, 1024 threads):
//   * at an event, in the one thread that applies it (no atomics, a fixed floating-point order): the bind time of the particle
//     slot, the lifetime histogram and sums when a bound state ends, the exits per anchor group;
//   * at an observation, by the whole workgroup: one row of GILC_NFIXED + n_groups + c_bins integers --
//       [0] live  [1] bound  [2] binds  [3] unbinds  [4] exits  [5] occupied sites  [6] clusters  [7] largest  [8] sum size^2
//       [9 .. 9 + G) exits per group     [9 + G ..) clusters of size 1 .. c_bins - 1 and >= c_bins
//     A cluster is a maximal run of sites with occ > 0 between site 0 and site L - 1 (no wrap, as the reference's
//     get_cluster_sizes).  A run ends at x when occ[x] > 0 and x + 1 is empty or the wall; its size is x minus the index of
//     the last empty site before it, which is a running maximum over the sites: tiles of NT consecutive sites, a lane per
//     site, a wavefront max-scan plus one LDS slot per wavefront, the last empty index carried from tile to tile.
// Everything a workgroup keeps between events lives in its capture slots in LDS (8 bytes each, gilc_lds_slots), so the event
// loop holds no register for it; the slots reach global memory at an observation (row) and once at the end (lifetimes).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>

#include "gillespie.h"

// What gilc_run hands to the drivers of the two kernels (host side; the two sources are linked into one library)
struct GilcCall {
    const int32_t *group_of_site;              // [L], -1 = none, or nullptr
    int n_groups, c_bins, h_bins, first_obs;
    double h_dt;
    int64_t *capture_obs, *life_hist;          // [S][n_obs][9 + G + c_bins], [S][2][h_bins]
    double *life_sums;                         // [S][2][2]
};

namespace {

constexpr int GILC_ALIVE = 4, GILC_BOUND = 2;  // F_ALIVE, F_BOUND of the loop kernels' flag byte
constexpr int GILC_FIXED = 9;                  // GILC_NFIXED of the header

struct GilcArgs {                              // what a capture instantiation gets on top of the loop's own arguments
    long long *rows;                           // [n_systems][n_obs][9 + G + c_bins], zero-filled: rows nobody writes stay zero
    long long *life_hist;                      // [n_systems][2][h_bins]
    double *life_sums;                         // [n_systems][2][2]  sum, sum of squares per way of ending
    double *tbind;                             // large shape: [n_systems][n_cap] bind times (the batch shape keeps them in LDS)
    const int32_t *group;                      // [L] anchor group of a site, -1 none; or nullptr
    double h_dt;
    int n_groups, c_bins, h_bins, first_obs;
};

// 8-byte slots of LDS per workgroup: 4 lifetime sums, 2 h_bins histogram counts, binds + unbinds + G exit counts, 6 sums of
// an observation, c_bins cluster counts, nt / 64 for the scan (two ints per wavefront: the tiles alternate)
constexpr size_t gilc_lds_slots(int nt, int n_groups, int c_bins, int h_bins) {
    return (size_t)12 + (size_t)(nt / 64) + 2 * (size_t)h_bins + (size_t)n_groups + (size_t)c_bins;
}

struct GilcLds {
    double *sums;                              // [2][2]
    long long *hist, *cnt, *acc, *chist;       // [2][h_bins]; binds, unbinds, exits[G]; occupied, clusters, largest, size^2, live, bound; [c_bins]
    int *scan;                                 // [2][nt / 64] last empty site of each wavefront's part of a tile
    double *tbind;                             // [n_cap] behind the slots (batch shape)
};

__device__ __forceinline__ GilcLds gilc_lds(void *base, const GilcArgs &c, int nw) {
    GilcLds s;
    s.sums = static_cast<double *>(base);
    s.hist = reinterpret_cast<long long *>(s.sums + 4);
    s.cnt = s.hist + 2 * c.h_bins;
    s.acc = s.cnt + 2 + c.n_groups;
    s.chist = s.acc + 6;
    s.scan = reinterpret_cast<int *>(s.chist + c.c_bins);
    s.tbind = reinterpret_cast<double *>(s.chist + c.c_bins + nw);
    return s;
}

// every thread, before the first event: the slots that outlive an observation start from zero
template <int NT>
__device__ inline void gilc_init(const GilcLds &s, const GilcArgs &c, double *tbind, int ncap) {
    const int n = 4 + 2 * c.h_bins + 2 + c.n_groups;           // sums, hist and cnt are contiguous
    for (int q = threadIdx.x; q < n; q += NT) reinterpret_cast<long long *>(s.sums)[q] = 0;   // a zero double is a zero integer
    for (int i = threadIdx.x; i < ncap; i += NT) tbind[i] = 0.0;   // particles that start bound: bound since t = 0
}

// ---- the thread that applies the event; t = the loop time before the event's own waiting time (the exit log's clock)
__device__ __forceinline__ void gilc_on_bind(const GilcLds &s, double *tbind, int i, double t) {
    tbind[i] = t;
    s.cnt[0] += 1;
}

__device__ __forceinline__ void gilc_end_of_bound_state(const GilcLds &s, const GilcArgs &c, const double *tbind, int i, double t, int end) {
    const double life = t - tbind[i];
    // clamped while still a double (a literal, not a loop-invariant value the large kernel would have to spill), then in integers
    const int b = min((int)fmin(floor(life / c.h_dt), 1.0e9), c.h_bins - 1);
    s.hist[end * c.h_bins + b] += 1;
    s.sums[2 * end] += life;
    s.sums[2 * end + 1] += life * life;
}

__device__ __forceinline__ void gilc_on_unbind(const GilcLds &s, const GilcArgs &c, const double *tbind, int i, double t) {
    gilc_end_of_bound_state(s, c, tbind, i, t, 0);
    s.cnt[1] += 1;
}

__device__ __forceinline__ void gilc_on_exit(const GilcLds &s, const GilcArgs &c, const double *tbind, int i, int site, bool bound, double t) {
    if (bound) gilc_end_of_bound_state(s, c, tbind, i, t, 1);
    if (c.group) {
        const int g = c.group[site];
        if (g >= 0) s.cnt[2 + g] += 1;
    }
}

// ---- observation: every thread of the workgroup calls it (it holds barriers).  occ: particles per site (LDS bytes or
// global ints); flg: the particle slots' flags; n_exit: exits so far (every thread holds it).
template <int NT, typename Occ>
__device__ inline void gilc_record_row(long long *row, const GilcLds &s, const GilcArgs &c, int L, int ncap, const uint8_t *flg,
                                       const Occ *occ, int n_exit) {
    constexpr int NW = NT / 64;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int q = t; q < 6 + c.c_bins; q += NT) s.acc[q] = 0;   // acc and chist are contiguous
    long long n_live = 0, n_bound = 0;
    for (int i = t; i < ncap; i += NT) {
        const uint8_t f = flg[i];
        if (f & GILC_ALIVE) { n_live += 1; n_bound += (f & GILC_BOUND) ? 1 : 0; }
    }
    __syncthreads();
    long long n_occ = 0, n_cl = 0, s2 = 0;
    int big = 0, carry = -1, par = 0;                          // carry: last empty site before this tile
    for (int base = 0; base < L; base += NT, par ^= NW) {
        const int x = base + t;
        const bool in = x < L;
        const int here = in ? (int)occ[x] : 0, next = x + 1 < L ? (int)occ[x + 1] : 0;
        int e = (in && here == 0) ? x : -1;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(e, off); if (lane >= off) e = max(e, o); }
        if (lane == 63) s.scan[par + wave] = e;
        __syncthreads();                                       // one barrier per tile: the next tile writes the other half
        int before = carry;
#pragma unroll
        for (int w = 0; w < NW; ++w) { const int m = s.scan[par + w]; carry = max(carry, m); if (w < wave) before = max(before, m); }
        e = max(e, before);
        if (here > 0) {
            n_occ += 1;
            if (next == 0) {
                const int size = x - e;
                n_cl += 1; big = max(big, size); s2 += (long long)size * size;
                atomicAdd(reinterpret_cast<unsigned long long *>(s.chist + (min(size, c.c_bins) - 1)), 1ull);
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n_occ += __shfl_xor(n_occ, off); n_cl += __shfl_xor(n_cl, off); s2 += __shfl_xor(s2, off);
        n_live += __shfl_xor(n_live, off); n_bound += __shfl_xor(n_bound, off); big = max(big, __shfl_xor(big, off));
    }
    if (lane == 0) {
        atomicAdd(reinterpret_cast<unsigned long long *>(s.acc + 0), (unsigned long long)n_occ);
        atomicAdd(reinterpret_cast<unsigned long long *>(s.acc + 1), (unsigned long long)n_cl);
        atomicMax(s.acc + 2, (long long)big);
        atomicAdd(reinterpret_cast<unsigned long long *>(s.acc + 3), (unsigned long long)s2);
        atomicAdd(reinterpret_cast<unsigned long long *>(s.acc + 4), (unsigned long long)n_live);
        atomicAdd(reinterpret_cast<unsigned long long *>(s.acc + 5), (unsigned long long)n_bound);
    }
    __syncthreads();
    const int G = c.n_groups;
    for (int q = t; q < GILC_FIXED + G + c.c_bins; q += NT) {
        long long v;
        if (q == 0) v = s.acc[4];
        else if (q == 1) v = s.acc[5];
        else if (q == 2) v = s.cnt[0];
        else if (q == 3) v = s.cnt[1];
        else if (q == 4) v = n_exit;
        else if (q < GILC_FIXED) v = s.acc[q - 5];
        else if (q < GILC_FIXED + G) v = s.cnt[2 + q - GILC_FIXED];
        else v = s.chist[q - GILC_FIXED - G];
        row[q] = v;
    }
    __syncthreads();
}

// every thread, after the last event: the lifetime histograms and sums of the system leave LDS
template <int NT>
__device__ inline void gilc_flush(const GilcLds &s, const GilcArgs &c, size_t sys) {
    for (int q = threadIdx.x; q < 2 * c.h_bins; q += NT) c.life_hist[sys * 2 * (size_t)c.h_bins + q] = s.hist[q];
    if (threadIdx.x < 4) c.life_sums[sys * 4 + threadIdx.x] = s.sums[threadIdx.x];
}

}  // namespace
