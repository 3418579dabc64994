// gillespie_big_hip.hip -- gil_run_large of include/gillespie.h, gilm_run of include/gillespie_many.h, gilxm_run of
// include/gillespie_mixed_many.h and the large shape of gils_run, gilc_run, gilp_run, gilrm_run, gilxmr_run, gilxp_run, gilpr_run and gilxpr_run: the reference's
// exact event loop (PARTICLE_solver_CLASS.py:511-538) for systems far too large for a workgroup's LDS (the BASELINE size:
// N = 1e5 particles on L = 2e5 sites, where the reference manages 0.8 events/s because it recomputes the whole
// field and all N rates before every event).  One kernel and one host driver serve both entry points: a batch is a grid
// of independent workgroups, gil_run_large is the batch of one.
//
// One persistent workgroup of 1024 threads per system (blockIdx.x; no workgroup waits on another, so a batch larger
// than the device simply queues); the state lives in global memory (L2-resident), every per-system array in slices of
// one system's length, only the weight table and small work areas in LDS.  What makes an event cheap:
//   * the smoothed histograms W, S are kept incrementally (exact weight grid) -- an event changes them on
//     the sites within the table's reach of one or two sites;
//   * a site -> particle map (K slots per site) finds the particles whose rates that changes without scanning all N;
//   * rates are summed in two levels (blocks of 256 particles, then the block sums): only the blocks holding
//     re-evaluated particles are re-summed, the choice of the particle descends the two levels.
// Event semantics, threshold order, exit handling and observation timing are those of gillespie_hip.hip (same
// channels() device function, same draws).  Parity: same-uniforms trajectories against the oracle and against the
// LDS-resident kernel (tests/test_gpu_gillespie.py).
// Host side: gil_large_run takes the call record of gillespie_common.hpp (GilIo, GilExtras) and stages through its helpers; the entry
// points of gillespie_hip.hip that fall to this shape call it and gil_large_plan.

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "gillespie.h"
#include "gillespie_many.h"
#include "gillespie_mixed_many.h"
#include "aps_common.hpp"
#include "gillespie_common.hpp"
#include "gillespie_structure.hpp"        // the structure sums of an observation (structure instantiation only)
#include "gillespie_capture.hpp"          // anchor capture and cluster statistics (capture instantiation only)
#include "gillespie_profile.hpp"          // ensemble density and field profiles (profile instantiation only)
#include "gillespie_resume.hpp"           // start and end state of a launch (resumable instantiation only)
#include "gillespie_mixed.hpp"            // a variant per system: table, blocking table, Philox key (mixed instantiation only)

namespace {

constexpr int BT = 1024, BW = BT / 64;      // threads, waves of the workgroup
constexpr int PB = 256;                     // particles per rate block
constexpr int MAX_NB = 4096;                // rate blocks (N <= 2^20)
constexpr int TAB_LDS_MAX = 10000;          // table entries kept in LDS
std::string g_big_err, g_many_err, g_gilxm_err;
enum { F_PLUS = 1, F_BOUND = 2, F_ALIVE = 4 };
enum { GS_N = 0, GS_SPIN, GS_POS, GS_WALL, GS_MAXPOS, GS_FRONT, GS_ATTEMPT, GS_BLOCKED, GS_DISP, GS_DISP2, GS_NDISP, GS_EVENTS };

struct BigArgs {
    Model m;
    gil_params p;
    int tlen, n_init, nblk, cb, tab_in_lds;
    double beta;                                             // n_init, beta: of the workgroup's system (select_system)
    const double *table, *times, *uniforms, *betas;          // shared: table, times, anchor, front_lo, block_table
    const uint8_t *anchor, *block_table;
    const int32_t *front_lo, *n0;
    const int32_t *pos0; const int8_t *sigma0; const uint8_t *bound0;
    // global scratch, [n_systems] slices
    int *pos, *occ, *occp, *slot, *work, *ref;
    uint8_t *flg;
    double *rate, *bsum, *W, *S;
    // outputs, [n_systems] slices
    int32_t *pos_obs; int8_t *sigma_obs; uint8_t *flags_obs; long long *scalars;
    int32_t *n_recorded; long long *n_events; double *t_final, *exits; int32_t *n_exits;
};

// Narrows a copy of the arguments to system `sys` (uniform over the workgroup, so the slices' addresses stay in scalar
// registers): the code below indexes one system.  Philox key = seed + sys, i.e. system s of a batch draws what a
// single run with seed + s draws.
__device__ inline void select_system(BigArgs &a, size_t sys) {
    const size_t N = (size_t)a.p.n_cap, L = (size_t)a.m.L, O = (size_t)a.p.n_obs;
    a.n_init = a.n0[sys]; a.beta = a.betas[sys];
    const unsigned long long key = (((unsigned long long)a.m.seed_hi << 32) | a.m.seed_lo) + sys;
    a.m.seed_lo = (uint32_t)key; a.m.seed_hi = (uint32_t)(key >> 32);
    a.pos0 += sys * N; a.sigma0 += sys * N;
    if (a.bound0) a.bound0 += sys * N;
    if (a.uniforms) a.uniforms += sys * (size_t)a.p.max_events * 4;
    a.pos += sys * N; a.work += sys * N; a.ref += sys * N; a.flg += sys * N; a.rate += sys * N;
    a.occ += sys * L; a.occp += sys * L; a.W += sys * L; a.S += sys * L;
    a.slot += sys * L * (size_t)a.m.K; a.bsum += sys * (size_t)a.nblk;
    if (a.pos_obs) a.pos_obs += sys * O * N;
    if (a.sigma_obs) a.sigma_obs += sys * O * N;
    if (a.flags_obs) a.flags_obs += sys * O * N;
    if (a.scalars) a.scalars += sys * O * GIL_NSCALARS;
    if (a.exits) a.exits += sys * N * 3;
    if (a.n_recorded) a.n_recorded += sys;
    if (a.n_events) a.n_events += sys;
    if (a.t_final) a.t_final += sys;
    if (a.n_exits) a.n_exits += sys;
}

// W, S of site x from scratch: over all particles of the start state of the system `a` is narrowed to
__device__ inline void field_init_site(const BigArgs &a, int x) {
    double w = 0.0, s = 0.0;
    if (a.m.field_mode)
        for (int j = 0; j < a.n_init; ++j) {
            const double g = site_weight(a.m, a.table, a.tlen, x, a.pos0[j]);
            w += g; s += a.sigma0[j] > 0 ? g : -g;
        }
    a.W[x] = w; a.S[x] = s;
}

// W, S from scratch on all sites (one-time): a thread per site over all particles; the system in grid.y
__global__ __launch_bounds__(256) void big_field_init(const BigArgs a0) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= a0.m.L) return;
    BigArgs a = a0;
    select_system(a, (size_t)blockIdx.y);
    field_init_site(a, x);
}

// The same from a checkpoint (resumable launch): pos0 holds every slot's site, sigma0 its spin or 0 for a slot that is not alive
__device__ inline void field_init_site_live(const BigArgs &a, int x) {
    double w = 0.0, s = 0.0;
    if (a.m.field_mode)
        for (int j = 0; j < a.p.n_cap; ++j) {
            const int sg = a.sigma0[j];
            if (sg == 0) continue;
            const double g = site_weight(a.m, a.table, a.tlen, x, a.pos0[j]);
            w += g; s += sg > 0 ? g : -g;
        }
    a.W[x] = w; a.S[x] = s;
}

__global__ __launch_bounds__(256) void big_field_init_live(const BigArgs a0) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= a0.m.L) return;
    BigArgs a = a0;
    select_system(a, (size_t)blockIdx.y);
    field_init_site_live(a, x);
}

__device__ inline double big_rate(const BigArgs &a, const double *tab, int i, long long gs, long long gn) {
    (void)tab;
    const Model &M = a.m;
    const int L = M.L, p = a.pos[i];
    const uint8_t f = a.flg[i];
    double w, s;
    if (M.field_mode) { w = a.W[p]; s = a.S[p]; } else { w = (double)gn; s = (double)gs; }
    double mloc = 0.0;
    if (w > 0.0) { mloc = s / w; mloc = mloc > 1.0 ? 1.0 : (mloc < -1.0 ? -1.0 : mloc); }
    int l = p - 1, r = p + 1;
    if (M.periodic) { l = l < 0 ? l + L : l; r = r >= L ? r - L : r; }
    return channels(M, a.anchor ? a.anchor[p] != 0 : false, p, (f & F_PLUS) ? 1 : -1, (f & F_BOUND) != 0, mloc, a.beta,
                    a.occ[p], l >= 0 ? a.occ[l] : 0, r < L ? a.occ[r] : 0).total;
}

// lowest / highest thread of the workgroup for which `flag` holds, into *lo / *hi: one LDS atomic per wavefront
// (hundreds of same-address atomics from single lanes serialise at ~25 cycles each)
__device__ inline void note_first_last(bool flag, int *lo, int *hi) {
    const unsigned long long m = __ballot(flag);
    if (m && (threadIdx.x & 63) == 0) {
        const int base = (int)(threadIdx.x & ~63u);
        atomicMin(lo, base + __builtin_ctzll(m));
        atomicMax(hi, base + 63 - __builtin_clzll(m));
    }
}

// inclusive scan over the 1024 threads; `xw` = BW doubles of LDS
__device__ inline double block_scan_inclusive(double v, double *xw) {
    double inc = wave_scan_inclusive(v);
    const int t = threadIdx.x;
    __syncthreads();
    if ((t & 63) == 63) xw[t >> 6] = inc;
    __syncthreads();
    double before = 0.0;
    for (int w = 0; w < (t >> 6); ++w) before += xw[w];
    return inc + before;
}

// Adds this wavefront's sum of v to *dst (LDS): one atomic per wavefront
__device__ inline void wave_add_ll(long long v, long long *dst) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0 && v != 0) atomicAdd(reinterpret_cast<unsigned long long *>(dst), (unsigned long long)v);
}

// The twelve sums of gil_run_batch (gillespie_hip.hip, record) over one system's particles at an observation: integers, so
// the order of summation is free.  `acc` = GIL_NSCALARS words of LDS.  A particle index belongs to the same thread in
// both passes, also where `ref` is written: no barrier is needed for `ref`.
__device__ inline void big_scalar_sums(const int *pos, const uint8_t *flg, int *ref, const int *occ, const int *occp,
                                       const uint8_t *block_table, const int32_t *front_lo, long long *out, long long *acc,
                                       int N, int L, int K, bool set_ref, int x_wall, long long n_ev) {
    const int t = threadIdx.x;
    if (t < GIL_NSCALARS) acc[t] = t == GS_MAXPOS ? -1 : (t == GS_EVENTS ? n_ev : 0);
    __syncthreads();
    {
        long long v_n = 0, v_spin = 0, v_pos = 0, v_wall = 0;
        int v_max = -1;
#pragma unroll 1
        for (int i = t; i < N; i += BT) {
            const uint8_t f = flg[i];
            const int p = pos[i];
            if (set_ref) ref[i] = (f & F_ALIVE) ? p : -1;
            if (!(f & F_ALIVE)) continue;
            v_n += 1; v_spin += (f & F_PLUS) ? 1 : -1; v_pos += p; v_wall += p >= x_wall;
            v_max = max(v_max, p);
        }
        wave_add_ll(v_n, acc + GS_N); wave_add_ll(v_spin, acc + GS_SPIN); wave_add_ll(v_pos, acc + GS_POS); wave_add_ll(v_wall, acc + GS_WALL);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v_max = max(v_max, __shfl_xor(v_max, off));
        if ((t & 63) == 0) atomicMax(acc + GS_MAXPOS, (long long)v_max);
    }
    __syncthreads();
    {
        const long long mx = acc[GS_MAXPOS];
        const int lo = (front_lo && mx >= 0) ? front_lo[mx] : L;   // no window: no site counts
        long long v_front = 0, v_att = 0, v_blk = 0, v_d = 0, v_d2 = 0, v_nd = 0;
#pragma unroll 1
        for (int i = t; i < N; i += BT) {
            const uint8_t f = flg[i];
            if (!(f & F_ALIVE)) continue;
            const int p = pos[i], r0 = ref[i];
            v_front += p >= lo;
            if ((f & F_PLUS) && p < L - 1) {                   // plus movers, and whether the right neighbour blocks them
                v_att += 1;
                const int cp = occp[p + 1], cm = occ[p + 1] - cp;
                v_blk += block_table ? block_table[cp * (K + 1) + cm] : (cp + cm >= 1);
            }
            if (r0 >= 0) { const long long d = (long long)p - r0; v_d += d; v_d2 += d * d; v_nd += 1; }
        }
        wave_add_ll(v_front, acc + GS_FRONT); wave_add_ll(v_att, acc + GS_ATTEMPT); wave_add_ll(v_blk, acc + GS_BLOCKED);
        wave_add_ll(v_d, acc + GS_DISP); wave_add_ll(v_d2, acc + GS_DISP2); wave_add_ll(v_nd, acc + GS_NDISP);
    }
    __syncthreads();
    if (t < GIL_NSCALARS) out[t] = acc[t];
    __syncthreads();
}

struct GilsBigArgs : BigArgs { GilsArgs st; };              // arguments of the structure instantiation
struct GilcBigArgs : GilsBigArgs { GilcArgs cp; };          // arguments of the capture instantiation
struct GilpBigArgs : GilcBigArgs { GilpArgs pf; };          // arguments of the profile instantiation (the driver's one struct)
struct GilrBigArgs : BigArgs { GilrArgs rs; };              // arguments of the resumable instantiation
struct GilxBigArgs : BigArgs { GilxArgs mx; int tab_region; };   // arguments of the mixed instantiation; tab_region: doubles of LDS
                                                                 //   for the table, the longest of the launch that is kept there

// The same for a mixed launch: table, length and field mode are the system's own
__global__ __launch_bounds__(256) void big_field_init_mixed(const GilxBigArgs a0) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= a0.m.L) return;
    BigArgs a = a0;
    select_system(a, (size_t)blockIdx.y);
    gilxm_select(a, a0.mx, (int)blockIdx.y, TAB_LDS_MAX);
    field_init_site(a, x);
}

struct GilxrBigArgs : GilxBigArgs { GilrArgs rs; };         // arguments of the resumable mixed instantiation
struct GilxpBigArgs : GilxBigArgs { GilpArgs pf; };         // arguments of the mixed profile instantiation (gilxp_run's large shape)
struct GilprBigArgs : GilrBigArgs { GilpArgs pf; };         // arguments of the resumable profile instantiation (gilpr_run's large shape)
struct GilxprBigArgs : GilxrBigArgs { GilpArgs pf; };       // arguments of the resumable mixed profile instantiation (gilxpr_run's)

// From a checkpoint in a mixed launch: big_field_init_live with the system's own table, length and field mode
__global__ __launch_bounds__(256) void big_field_init_live_mixed(const GilxBigArgs a0) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= a0.m.L) return;
    BigArgs a = a0;
    select_system(a, (size_t)blockIdx.y);
    gilxm_select(a, a0.mx, (int)blockIdx.y, TAB_LDS_MAX);
    field_init_site_live(a, x);
}

// the argument struct of each variant of the large-system kernel
template <GilKind V> struct BigKernelArgs;
template <> struct BigKernelArgs<GilKind::Plain> { using type = BigArgs; };
template <> struct BigKernelArgs<GilKind::Structure> { using type = GilsBigArgs; };
template <> struct BigKernelArgs<GilKind::Capture> { using type = GilcBigArgs; };
template <> struct BigKernelArgs<GilKind::Profile> { using type = GilpBigArgs; };
template <> struct BigKernelArgs<GilKind::Resume> { using type = GilrBigArgs; };
template <> struct BigKernelArgs<GilKind::Mixed> { using type = GilxBigArgs; };
template <> struct BigKernelArgs<GilKind::MixedResume> { using type = GilxrBigArgs; };
template <> struct BigKernelArgs<GilKind::MixedProfile> { using type = GilxpBigArgs; };
template <> struct BigKernelArgs<GilKind::ProfileResume> { using type = GilprBigArgs; };
template <> struct BigKernelArgs<GilKind::MixedProfileResume> { using type = GilxprBigArgs; };

// V = the variant, a compile-time property, so that each kernel is the code it was before the others existed:
//   Structure  also reduce the structure sums at an observation (gillespie_structure.hpp);
//   Capture    anchor capture and cluster statistics (gillespie_capture.hpp).  Its slots lie behind ctl[] in LDS, its bind times
//              in global memory; the event loop holds no register for either;
//   Profile    ensemble density and field profiles (gillespie_profile.hpp).  Its slots lie behind ctl[] in LDS and are used at an
//              observation only;
//   Resume     a resumable launch (gillespie_resume.hpp): the start state is a checkpoint (pos0 / sigma0 as big_field_init_live
//              reads them, n0 = n_cap: any slot may be alive; flags, origins, clock, event count and first row from a0.rs).  The
//              end state is the global scratch itself (pos, flg, ref), which the driver reads back.
//   Mixed      a mixed batch (gillespie_mixed.hpp, include/gillespie_mixed_many.h): the workgroup takes system order[blockIdx.x],
//              and the weight table, its length, whether it lies in LDS, the field mode, the blocking table and the Philox key and
//              stream are that system's own, all uniform over the workgroup.  Outputs are indexed by the system.
//   MixedResume  a resumable mixed launch (include/gillespie_mixed_resume.h): Mixed with the start and end of Resume.  The
//              checkpoint's rows are the system's (RS_ROW), not the workgroup's; gilxm_select is applied before anything is read.
//              The rate sums are grouped by blocks of the launch's n_cap, so the slot count does not enter here.
//   MixedProfile  the ensemble profiles of a mixed launch (include/gillespie_mixed_profile.h): Mixed with the observation pass of
//              Profile.  The group table, members and the per-system rows are indexed by the SYSTEM (mx_sys), the field mode is the
//              one gilxm_select wrote, and the slots lie behind ctl[] of the launch's layout (tab_region).
//   ProfileResume, MixedProfileResume  a resumable profile launch (include/gillespie_profile_resume.h): the start and end of
//              Resume / MixedResume with the observation pass of Profile / MixedProfile over all N slots (it asks the flags).  The
//              observations a resumed start records before its first event go through the same pass, with the checkpoint's state
//              and the global mean rebuilt from its live flags; pf.first_obs and the group rows count within the launch's slice.
template <GilKind V>
__global__ __launch_bounds__(BT) void gil_big_kernel(const typename BigKernelArgs<V>::type a0) {
    constexpr bool ST = V == GilKind::Structure, CP = V == GilKind::Capture;
    constexpr bool PF = V == GilKind::Profile || V == GilKind::MixedProfile || V == GilKind::ProfileResume || V == GilKind::MixedProfileResume;
    constexpr bool RS = V == GilKind::Resume || V == GilKind::MixedResume || V == GilKind::ProfileResume || V == GilKind::MixedProfileResume;
    constexpr bool MX = V == GilKind::Mixed || V == GilKind::MixedResume || V == GilKind::MixedProfile || V == GilKind::MixedProfileResume;
    extern __shared__ double lds[];
    BigArgs a = a0;
    uint32_t stream = 0u;                                      // Philox counter word 2: the system's own with MX
    [[maybe_unused]] int mx_sys = 0;                           // MX: the system this workgroup took
// RS: the system's row of the checkpoint -- with MX not the workgroup's (MX is a constant: one arm is compiled)
#define RS_ROW (MX ? (size_t)mx_sys : (size_t)blockIdx.x)
    if constexpr (MX) {
        const int sys = __builtin_amdgcn_readfirstlane(a0.mx.order[blockIdx.x]);
        select_system(a, (size_t)sys);
        stream = gilxm_select(a, a0.mx, sys, TAB_LDS_MAX);
        mx_sys = sys;
    } else select_system(a, (size_t)__builtin_amdgcn_readfirstlane((int)blockIdx.x));
    const Model &M = a.m;
    const int L = M.L, K = M.K, t = threadIdx.x, lane = t & 63, wave = t >> 6, nobs = a.p.n_obs, N = a.p.n_cap;
    double *tabl = lds;                                        // [tlen + 1] when it fits
    int tab_region = a.tab_in_lds ? ((a.tlen + 2) & ~1) : 0;   // with MX the launch's: the longest table kept in LDS
    if constexpr (MX) tab_region = a0.tab_region;
    double *xw = tabl + tab_region;                            // [32] cross-wave scratch
    double *draws = xw + 32;                                   // [BT][4]
    double *dsel = draws + 4 * BT;                             // [4] cumulative rate before the chosen block etc.
    long long *acc = reinterpret_cast<long long *>(dsel + 4);  // [GIL_NSCALARS] the scalar sums of an observation
    int *bflag = reinterpret_cast<int *>(acc + GIL_NSCALARS);  // [nblk] block needs re-summing
    int *blist = bflag + a.nblk;                               // [nblk] list of those blocks
    int *ctl = blist + a.nblk;                                 // [32]
    const double *tab = a.tab_in_lds ? tabl : a.table;
    if (a.tab_in_lds) for (int i = t; i <= a.tlen; i += BT) tabl[i] = a.table[i];
    for (int j = t; j < a.nblk; j += BT) bflag[j] = 0;
    if constexpr (CP) gilc_init<BT>(gilc_lds(ctl + 32, a0.cp, BW), a0.cp, a0.cp.tbind + (size_t)blockIdx.x * N, N);
    // ---- load the system: particles, occupancy, site -> particle map
    for (int x = t; x < L; x += BT) { a.occ[x] = 0; a.occp[x] = 0; }
    for (size_t q = t; q < (size_t)L * K; q += BT) a.slot[q] = -1;
    __syncthreads();
    long long ls = 0, ln = 0;
    for (int i = t; i < N; i += BT) {
        bool live; int p, r0 = -1; uint8_t f;
        if constexpr (RS) {                                    // the checkpoint's slots: departed ones stay dead, origins are kept
            p = a.pos0[i]; f = a0.rs.flg[RS_ROW * N + i]; r0 = a0.rs.ref[RS_ROW * N + i]; live = (f & F_ALIVE) != 0;
        } else {
            live = i < a.n_init;
            p = live ? a.pos0[i] : 0;
            f = live ? (uint8_t)(F_ALIVE | (a.sigma0[i] > 0 ? F_PLUS : 0) | ((a.bound0 && a.bound0[i]) ? F_BOUND : 0)) : 0;
        }
        a.pos[i] = p; a.flg[i] = f; a.rate[i] = 0.0; a.ref[i] = r0;
        if (live) {
            a.slot[(size_t)p * K + atomicAdd(&a.occ[p], 1)] = i;
            if (f & F_PLUS) atomicAdd(&a.occp[p], 1);
            ls += (f & F_PLUS) ? 1 : -1; ln += 1;
        }
    }
    __syncthreads();
    // global-mean mode: sum of spins, particles alive (every thread holds the totals)
    long long gsum_s = 0, gsum_n = 0;
    {
        long long *xl = reinterpret_cast<long long *>(xw);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { ls += __shfl_xor(ls, off); ln += __shfl_xor(ln, off); }
        if (lane == 0) { xl[wave] = ls; xl[BW + wave] = ln; }
        __syncthreads();
        for (int w = 0; w < BW; ++w) { gsum_s += xl[w]; gsum_n += xl[BW + w]; }
        __syncthreads();
    }
    for (int i = t; i < a.n_init; i += BT) { if (RS && !(a.flg[i] & F_ALIVE)) continue; a.rate[i] = big_rate(a, tab, i, gsum_s, gsum_n); }
    __syncthreads();
    for (int j = wave; j < a.nblk; j += BW) {                  // block sums
        double v = 0.0;
        for (int k = lane; k < PB; k += 64) { const int i = j * PB + k; if (i < N) v += a.rate[i]; }
        v = wave_scan_inclusive(v);
        if (lane == 63) a.bsum[j] = v;
    }
    __syncthreads();
    double tnow = 0.0, t_next = nobs > 1 ? a.times[1] : INFINITY;
    long long n_ev = 0, ev_base = 0;
    int k_obs = 0, n_exit = 0;
    if constexpr (RS) {
        tnow = a0.rs.t[RS_ROW]; n_ev = a0.rs.n_ev[RS_ROW]; k_obs = a0.rs.k_start[RS_ROW];
        ev_base = n_ev - BT;                                   // no draws held: the first iteration draws
    }

    auto record = [&](int k) {                                 // observation k: state and scalar sums (ref :517-536)
        const size_t o = (size_t)k * N;
        if (a.pos_obs || a.sigma_obs || a.flags_obs)
            for (int i = t; i < N; i += BT) {
                const uint8_t f = a.flg[i];
                if (a.pos_obs) a.pos_obs[o + i] = a.pos[i];
                if (a.sigma_obs) a.sigma_obs[o + i] = (f & F_PLUS) ? 1 : -1;
                if (a.flags_obs) a.flags_obs[o + i] = (uint8_t)(((f & F_BOUND) ? 1 : 0) | ((f & F_ALIVE) ? 2 : 0));
            }
        if (a.scalars)
            big_scalar_sums(a.pos, a.flg, a.ref, a.occ, a.occp, a.block_table, a.front_lo, a.scalars + (size_t)k * GIL_NSCALARS,
                            acc, N, L, K, k == a.p.ref_obs, a.p.x_wall, n_ev);
        if constexpr (ST) {
            const GilsArgs &sa = a0.st;
            if (k >= sa.first_obs) {
                double mg = 0.0;                               // global-mean mode: the one value of every site (ref :219-221)
                if (!M.field_mode && gsum_n > 0) { mg = (double)gsum_s / (double)gsum_n; mg = mg > 1.0 ? 1.0 : (mg < -1.0 ? -1.0 : mg); }
                gils_record_row<BT>(sa.rows + ((size_t)blockIdx.x * nobs + k) * (size_t)(4 + 2 * sa.k_max), sa.k_max, L, N, a.pos, a.flg,
                                    a.occ, a.W, a.S, M.field_mode != 0, mg, sa.phase, reinterpret_cast<double *>(ctl + 32), a.work);
            }
        }
        if constexpr (CP) {
            const GilcArgs &ca = a0.cp;
            if (k >= ca.first_obs)
                gilc_record_row<BT>(ca.rows + ((size_t)blockIdx.x * nobs + k) * (size_t)(GILC_FIXED + ca.n_groups + ca.c_bins),
                                    gilc_lds(ctl + 32, ca, BW), ca, L, N, a.flg, a.occ, n_exit);
        }
        if constexpr (PF) {
            if (k >= a0.pf.first_obs) {
                double mg = 0.0;                               // global-mean mode: the one value of every site (ref :219-221)
                if (!M.field_mode && gsum_n > 0) { mg = (double)gsum_s / (double)gsum_n; mg = mg > 1.0 ? 1.0 : (mg < -1.0 ? -1.0 : mg); }
                gilp_record<BT>(a0.pf, ctl + 32, MX ? (size_t)mx_sys : (size_t)blockIdx.x, k, nobs, L, N, a.pos, a.flg, a.W, a.S, M.field_mode != 0, mg);
            }
        }
    };
    if constexpr (RS) {
        // a fresh start records row 0; a resumed one the observations the checkpoint's last event passed (in the uninterrupted
        // run that event recorded them, with this state), unless that event passed T
        while (k_obs < nobs && (a0.rs.fresh ? k_obs == 0 : (tnow <= a.p.T && a.times[k_obs] <= tnow))) { record(k_obs); ++k_obs; }
        t_next = k_obs < nobs ? a.times[k_obs] : INFINITY;
    } else {
        record(0);
        k_obs = 1;
    }
    bool have_event = false, dirty_all = false;
    int ev_a = 0, ev_b = 0;
#ifdef APS_STAMPS
    unsigned long long st[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, s0 = __builtin_amdgcn_s_memtime();
#define BSTAMP(k) { const unsigned long long s1_ = __builtin_amdgcn_s_memtime(); st[k] += s1_ - s0; s0 = s1_; }
#else
#define BSTAMP(k)
#endif
    const int reach = (M.field_mode ? a.tlen - 1 : 0) + 1;
    while (tnow < a.p.T && k_obs < nobs && n_ev < a.p.max_events) {
        // ---- A: re-evaluate the rates the previous event changed
        if (have_event) {
            if (t == 0) { ctl[0] = 0; ctl[1] = 0; }
            __syncthreads();
            int lo, len;
            if (dirty_all) { lo = 0; len = 0; }                // handled below: every particle
            else {
                const bool wrapped = M.periodic && (ev_a - ev_b > 1 || ev_b - ev_a > 1);
                lo = (wrapped ? max(ev_a, ev_b) : min(ev_a, ev_b)) - reach;
                len = 2 * reach + 2;
                if (len >= L || (!M.periodic && reach >= L)) { lo = 0; len = L; }
            }
            auto append = [&](bool flag, int item) {           // one LDS atomic per wavefront: ballot + mbcnt compaction
                const unsigned long long m = __ballot(flag);
                if (!m) return;
                int base = 0;
                if (lane == 0) base = atomicAdd(&ctl[0], __popcll(m));
                base = __builtin_amdgcn_readfirstlane(base);
                if (flag) a.work[base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = item;
            };
            if (dirty_all) {
                for (int i0 = 0; i0 < N; i0 += BT) {
                    const int i = i0 + t;
                    append(i < N && (a.flg[i] & F_ALIVE), i);
                }
            } else {
                constexpr int U = 4;                           // site iterations whose occupancy loads are in flight together
                for (int k0 = 0; k0 < len; k0 += U * BT) {     // sites in reach -> their particles, through the map
                    int xs[U], ns[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int k = k0 + u * BT + t;
                        int x = lo + k;
                        if (M.periodic) { x %= L; if (x < 0) x += L; }
                        const bool in = k < len && x >= 0 && x < L;
                        xs[u] = in ? x : 0;
                        ns[u] = in ? a.occ[x] : 0;
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        for (int q = 0; __ballot(q < ns[u]); ++q) append(q < ns[u], q < ns[u] ? a.slot[(size_t)xs[u] * K + q] : 0);
                }
            }
            __syncthreads();
            BSTAMP(0)
            const int nwork = ctl[0];
            for (int base = 0; base < nwork; base += 4 * BT) {   // the list entries of four items per thread are fetched together
                int is[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { const int j = base + u * BT + t; is[u] = j < nwork ? a.work[j] : -1; }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = is[u];
                    if (i < 0) continue;
                    a.rate[i] = big_rate(a, tab, i, gsum_s, gsum_n);
                    if (atomicExch(&bflag[i / PB], 1) == 0) blist[atomicAdd(&ctl[1], 1)] = i / PB;
                }
            }
            __syncthreads();
            const int nb_dirty = ctl[1];
            for (int q = wave; q < nb_dirty; q += BW) {        // re-sum the touched blocks
                const int j = blist[q];
                double v = 0.0;
                for (int k = lane; k < PB; k += 64) { const int i = j * PB + k; if (i < N) v += a.rate[i]; }
                v = wave_scan_inclusive(v);
                if (lane == 63) { a.bsum[j] = v; bflag[j] = 0; }
            }
            __syncthreads();
        }
        BSTAMP(1)
        // ---- B: total rate, draws, choice of the block and of the particle
        double mine = 0.0;
        for (int j = t * a.cb; j < min(a.nblk, (t + 1) * a.cb); ++j) mine += a.bsum[j];
        const double inc = block_scan_inclusive(mine, xw);
        BSTAMP(5)
        if (t == BT - 1) dsel[0] = inc;
        if ((n_ev - ev_base) >= BT || n_ev == 0) {
            ev_base = n_ev;
            const long long evn = n_ev + t;
            double u0, u1, u2, u3;
            if (a.uniforms) {
                const bool in = evn < a.p.max_events;
                const double *src = a.uniforms + (size_t)(in ? evn : 0) * 4;
                u0 = in ? src[0] : 0.0; u1 = in ? src[1] : 0.0; u2 = in ? src[2] : 0.0; u3 = in ? src[3] : 0.0;
            } else {
                uint32_t x[4], y[4];
                philox4x32_10((uint32_t)evn, (uint32_t)(evn >> 32), stream, 0x47494C31u, M.seed_lo, M.seed_hi, x);
                philox4x32_10((uint32_t)evn, (uint32_t)(evn >> 32), stream, 0x47494C32u, M.seed_lo, M.seed_hi, y);
                u0 = ((double)(x[0] >> 5) * 67108864.0 + (double)(x[1] >> 6)) * 0x1.0p-53;
                u1 = ((double)(x[2] >> 5) * 67108864.0 + (double)(x[3] >> 6)) * 0x1.0p-53;
                u2 = ((double)(y[0] >> 5) * 67108864.0 + (double)(y[1] >> 6)) * 0x1.0p-53;
                u3 = ((double)(y[2] >> 5) * 67108864.0 + (double)(y[3] >> 6)) * 0x1.0p-53;
            }
            draws[4 * t] = -log1p(-u0); draws[4 * t + 1] = u1; draws[4 * t + 2] = u2; draws[4 * t + 3] = u3;
        }
        if (t == 0) { ctl[2] = BT; ctl[3] = -1; ctl[4] = PB; ctl[5] = -1; ctl[13] = -1; ctl[14] = BT; ctl[15] = -1; ctl[16] = BT; }
        __syncthreads();
        BSTAMP(6)
        const double R = dsel[0];
        if (!(R > 0.0)) { tnow = INFINITY; break; }           // ref :355
        const double *dr = draws + 4 * (int)(n_ev - ev_base);
        const double tau = (1.0 / R) * dr[0], target = dr[1] * R, u2 = dr[2], u3 = dr[3];
        note_first_last(inc > target && mine > 0.0, &ctl[2], &ctl[13]);
        note_first_last(mine > 0.0, &ctl[14], &ctl[3]);
        __syncthreads();
        BSTAMP(7)
        const int tsel = ctl[2] < BT ? ctl[2] : ctl[3];        // target rounded past the total: last thread with any rate
        if (t == tsel) {                                       // which of this thread's blocks
            double run = inc - mine;
            int jsel = -1;
            double before = run;
            for (int j = t * a.cb; j < min(a.nblk, (t + 1) * a.cb); ++j) {
                const double b = a.bsum[j];
                if (b > 0.0) { jsel = j; before = run; run += b; if (run > target) break; }
            }
            ctl[6] = jsel; dsel[1] = before;
        }
        __syncthreads();
        BSTAMP(8)
        const int jsel = ctl[6];
        {                                                      // the particle inside the block: its first 256 threads scan it
            double r = 0.0;
            const int i = jsel * PB + t;
            if (t < PB && i < N) r = a.rate[i];
            const double binc = block_scan_inclusive(r, xw) + dsel[1];
            note_first_last(t < PB && r > 0.0 && binc > target, &ctl[4], &ctl[15]);
            note_first_last(t < PB && r > 0.0, &ctl[16], &ctl[5]);
            __syncthreads();
        }
        const int isel = jsel * PB + (ctl[4] < PB ? ctl[4] : ctl[5]);
        BSTAMP(2)
        // ---- C: one thread applies the event (ref :363-446) and keeps the site map
        if (t == 0) {
            const int i = isel, p = a.pos[i];
            uint8_t f = a.flg[i];
            const bool plus = (f & F_PLUS) != 0;
            double w, s;
            if (M.field_mode) { w = a.W[p]; s = a.S[p]; } else { w = (double)gsum_n; s = (double)gsum_s; }
            double mloc = 0.0;
            if (w > 0.0) { mloc = s / w; mloc = mloc > 1.0 ? 1.0 : (mloc < -1.0 ? -1.0 : mloc); }
            int l = p - 1, rr = p + 1;
            if (M.periodic) { l = l < 0 ? l + L : l; rr = rr >= L ? rr - L : rr; }
            const Channels c = channels(M, a.anchor ? a.anchor[p] != 0 : false, p, plus ? 1 : -1, (f & F_BOUND) != 0, mloc, a.beta,
                                        a.occ[p], l >= 0 ? a.occ[l] : 0, rr < L ? a.occ[rr] : 0);
            const double v = u2 * c.total;
            const double e_diff = c.diff, e_act = e_diff + c.act, e_bind = e_act + c.bind, e_unbind = e_bind + c.unbind,
                         e_exit = e_unbind + c.leave;
            int kind = 0, to = p;                              // 0 nothing, 1 hop, 2 flip, 3 exit
            if (v < e_diff) {
                if (c.left + c.right > 0.0) { kind = 1; to = (u3 < c.left / (c.left + c.right)) ? p - 1 : p + 1; }
            } else if (v < e_act) { kind = 1; to = p + 1; }
            else if (v < e_bind) {
                f |= F_BOUND;
                if constexpr (CP) gilc_on_bind(gilc_lds(ctl + 32, a0.cp, BW), a0.cp.tbind + (size_t)blockIdx.x * N, i, tnow);
            } else if (v < e_unbind) {
                f &= (uint8_t)~F_BOUND;
                if constexpr (CP) gilc_on_unbind(gilc_lds(ctl + 32, a0.cp, BW), a0.cp, a0.cp.tbind + (size_t)blockIdx.x * N, i, tnow);
            }
            else if (v < e_exit) kind = 3;
            else kind = 2;
            auto unmap = [&](int site) {                       // take particle i out of the site's slots
                const int n = a.occ[site];
                for (int q = 0; q < n; ++q)
                    if (a.slot[(size_t)site * K + q] == i) { a.slot[(size_t)site * K + q] = a.slot[(size_t)site * K + n - 1]; break; }
                a.slot[(size_t)site * K + n - 1] = -1;
                a.occ[site] = n - 1;
            };
            if (kind == 1) {
                if (M.periodic) to = to < 0 ? to + L : (to >= L ? to - L : to);
                else to = to < 0 ? 0 : (to > L - 1 ? L - 1 : to);
                if (to == p) kind = 0;                         // clipped at a wall: nothing moved
                else {
                    unmap(p);
                    a.slot[(size_t)to * K + a.occ[to]] = i; a.occ[to] += 1;
                    if (plus) { a.occp[p] -= 1; a.occp[to] += 1; }
                    a.pos[i] = to;
                }
            } else if (kind == 2) {
                f ^= F_PLUS;
                a.occp[p] += plus ? -1 : 1;
            } else if (kind == 3) {
                f &= (uint8_t)~F_ALIVE;
                a.rate[i] = 0.0;
                unmap(p);
                if (plus) a.occp[p] -= 1;
                if (a.exits && n_exit < N) {
                    double *row = a.exits + (size_t)n_exit * 3;
                    row[0] = tnow; row[1] = (double)p; row[2] = (double)i;
                }
                if constexpr (CP) gilc_on_exit(gilc_lds(ctl + 32, a0.cp, BW), a0.cp, a0.cp.tbind + (size_t)blockIdx.x * N, i, p, (f & F_BOUND) != 0, tnow);
            }
            a.flg[i] = f;
            ctl[8] = kind; ctl[9] = p; ctl[10] = to; ctl[11] = plus ? 1 : -1; ctl[12] = i;
        }
        __syncthreads();
        const int kind = ctl[8], p_old = ctl[9], p_new = ctl[10], sg = ctl[11];
        if (kind == 3) n_exit += 1;
        BSTAMP(3)
        // ---- D: the event's change of the smoothed histograms
        if (!M.field_mode) {
            if (kind == 2) gsum_s -= 2 * sg;
            else if (kind == 3) { gsum_s -= sg; gsum_n -= 1; }
        } else if (kind != 0) {
            const int Rt = a.tlen - 1;
            const int centre = kind == 1 ? min(p_old, p_new) : p_old, span = kind == 1 ? 1 : 0;
            const bool wrap1 = kind == 1 && M.periodic && (p_old - p_new > 1 || p_new - p_old > 1);
            int lo = centre - Rt, len = 2 * Rt + 1 + span;
            if (wrap1 || len >= L || (!M.periodic && Rt >= L)) { lo = 0; len = L; }
            constexpr int U = 4;                               // sites per thread whose loads are in flight together
            for (int k0 = 0; k0 < len; k0 += U * BT) {
                int xs[U]; double ws[U], ss[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int k = k0 + u * BT + t;
                    int x = lo + k;
                    if (M.periodic) { x %= L; if (x < 0) x += L; }
                    const bool in = k < len && x >= 0 && x < L;
                    xs[u] = in ? x : -1;
                    ws[u] = in ? a.W[x] : 0.0; ss[u] = in ? a.S[x] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int x = xs[u];
                    if (x >= 0) {
                        const double g0 = site_weight(M, tab, a.tlen, x, p_old);
                        if (kind == 1) {
                            const double g1 = site_weight(M, tab, a.tlen, x, p_new), d = g1 - g0;  // exact on the weight grid
                            a.W[x] = ws[u] + d; a.S[x] = ss[u] + (sg > 0 ? d : -d);
                        } else if (kind == 2) {
                            a.S[x] = ss[u] - (sg > 0 ? 2.0 * g0 : -2.0 * g0);
                        } else {
                            a.W[x] = ws[u] - g0; a.S[x] = ss[u] - (sg > 0 ? g0 : -g0);
                        }
                    }
                }
            }
        }
        // a particle that left is no longer in the site map, so the next event's work list will not reach its block:
        // re-sum that block (its rate is zero now) here
        if (kind == 3 && wave == 0) {
            const int j = ctl[12] / PB;
            double v = 0.0;
            for (int k = lane; k < PB; k += 64) { const int i = j * PB + k; if (i < N) v += a.rate[i]; }
            v = wave_scan_inclusive(v);
            if (lane == 63) a.bsum[j] = v;
        }
        __syncthreads();
        BSTAMP(4)
        have_event = true;
        ev_a = p_old; ev_b = p_new;
        dirty_all = !M.field_mode && (kind == 2 || kind == 3);
        // ---- E: time and observations (ref :514-538)
        n_ev += 1;
        tnow += tau;
        if (tnow > a.p.T) break;
        while (__builtin_expect(k_obs < nobs && t_next <= tnow, 0)) { record(k_obs); ++k_obs; t_next = k_obs < nobs ? a.times[k_obs] : INFINITY; }
    }
#ifdef APS_STAMPS
    if (t == 0 && a.exits) for (int k = 0; k < 12; ++k) a.exits[k] = (double)st[k];   // diagnostic build only
#endif
    if constexpr (CP) gilc_flush<BT>(gilc_lds(ctl + 32, a0.cp, BW), a0.cp, (size_t)blockIdx.x);
    if (t == 0) {
        if (a.n_recorded) a.n_recorded[0] = k_obs;
        if (a.n_events) a.n_events[0] = n_ev;
        if (a.t_final) a.t_final[0] = tnow;
        if (a.n_exits) a.n_exits[0] = n_exit;
    }
}
#undef RS_ROW


// What a batch of p->n_systems large systems needs, by host arithmetic alone (gilm_plan); the weight table comes back
// through `table` where the caller wants it.  0, or e_arg with the text in `err`.
int big_plan(const char *who, std::string &err, const gil_params *p, bool want_states, bool want_scalars, gilm_plan_info *out,
             std::vector<double> *table) {
    auto bad = [&](const std::string &m) { err = std::string(who) + ": " + m; return GIL_ERR_ARG; };
    if (p->L < 2 || p->L > (1 << 25)) return bad("L must be in [2, 2^25]");
    if (p->K < 1 || p->K > 32) return bad("site capacity K must be in [1, 32]");
    if ((int64_t)p->L * p->K > (1ll << 27)) return bad("L * K must not exceed 2^27 (site map)");
    if (p->n_cap < 1 || p->n_cap > MAX_NB * PB || p->n_obs < 1 || p->max_events < 0) return bad("bad n_cap / n0 / n_obs / max_events");
    std::vector<double> tab; int tlen = 0, q = 0;
    weight_table(p->sigma_grid, p->L, p->K, p->periodic != 0, tab, tlen, q);
    const int64_t S = p->n_systems, L = p->L, N = p->n_cap, O = p->n_obs, nblk = (N + PB - 1) / PB;
    gilm_plan_info info{};
    info.n_systems = p->n_systems; info.n_blocks = (int32_t)nblk; info.table_len = tlen;
    info.table_in_lds = tlen + 1 <= TAB_LDS_MAX ? 1 : 0;
    info.lds_bytes = (int32_t)(((int64_t)(info.table_in_lds ? ((tlen + 2) & ~1) : 0) + 32 + 4 * BT + 4 + GIL_NSCALARS) * 8 + (2 * nblk + 32) * 4);
    // pos, work, ref (int), flg (byte), rate (double) per slot; occ, occp (int), W, S (double) per site; the site map; the block sums
    info.work_bytes_per_system = N * (4 + 4 + 4 + 1 + 8) + L * (4 + 4 + 8 + 8) + L * p->K * 4 + nblk * 8;
    // states: pos (int) + sigma + flags per slot and observation; scalars; exits; n_recorded, n_events, t_final, n_exits
    info.output_bytes = (want_states ? S * O * N * 6 : 0) + (want_scalars ? S * O * GIL_NSCALARS * 8 : 0) + S * N * 24 + S * 24;
    if (info.lds_bytes > 160 * 1024) return bad("LDS budget exceeded");
    if (S * info.work_bytes_per_system + info.output_bytes > GIL_PLAN_MAX_BYTES)
        return bad("the batch needs " + std::to_string(S * info.work_bytes_per_system) + " bytes of work memory and " +
                   std::to_string(info.output_bytes) + " bytes of outputs, more than the " + std::to_string(GIL_PLAN_MAX_BYTES) + " bytes a plan accepts");
    if (out) *out = info;
    if (table) *table = std::move(tab);
    return GIL_OK;
}

// The checks gilxm_plan and gilxm_run share, the variant tables and the plan of a mixed launch of large systems, by host
// arithmetic alone: 0 with `info` and `tb` filled, or GIL_ERR_ARG with the text in `err`.  The limits are big_plan's, here with
// the offending number; the variant checks and the tables are gilx_decide's (gillespie_mixed.hpp).
int gilxm_decide(const char *who, std::string &err, const gil_params *p, const gilx_variants *v, bool want_states, bool want_scalars,
                 gilxm_plan_info &info, GilxTables &tb) {
    auto bad = [&](const std::string &m) { err = std::string(who) + ": " + m; return GIL_ERR_ARG; };
    auto num = [](int64_t x) { return std::to_string(x); };
    if (p->L < 2 || p->L > (1 << 25)) return bad("L = " + num(p->L) + " is outside [2, 2^25 = " + num(1 << 25) + "]");
    if (p->K < 1 || p->K > 32) return bad("site capacity K = " + num(p->K) + " is outside [1, 32]");
    if ((int64_t)p->L * p->K > (1ll << 27)) return bad("L * K = " + num((int64_t)p->L * p->K) + " exceeds 2^27 = " + num(1ll << 27) + " (site map)");
    if (p->n_systems < 1 || p->n_systems > GILM_MAX_SYSTEMS) return bad("n_systems = " + num(p->n_systems) + " is outside [1, GILM_MAX_SYSTEMS = " + num(GILM_MAX_SYSTEMS) + "]");
    if (p->n_cap < 1 || p->n_cap > MAX_NB * PB) return bad("n_cap = " + num(p->n_cap) + " is outside [1, 2^20 = " + num(MAX_NB * PB) + "]");
    if (p->n_obs < 1) return bad("n_obs = " + num(p->n_obs) + " must be at least 1");
    if (p->max_events < 0) return bad("max_events = " + num(p->max_events) + " must not be negative");
    { const std::string why = gilx_check_variants(p, v); if (!why.empty()) return bad(why); }
    gilx_build_tables(p, v, tb);
    const int64_t S = p->n_systems, L = p->L, N = p->n_cap, O = p->n_obs, nblk = (N + PB - 1) / PB;
    info = gilxm_plan_info{};
    info.n_systems = p->n_systems; info.n_blocks = (int32_t)nblk; info.max_tlen = tb.max_tlen; info.max_tlen_lds = -1;
    for (const GilxVariant &gv : tb.var) {
        if (gv.tlen + 1 <= TAB_LDS_MAX) info.max_tlen_lds = std::max(info.max_tlen_lds, gv.tlen);
        else info.n_global += 1;
    }
    const int64_t region = info.max_tlen_lds >= 0 ? ((info.max_tlen_lds + 2) & ~1) : 0;
    const int64_t lds = (region + 32 + 4 * BT + 4 + GIL_NSCALARS) * 8 + (2 * nblk + 32) * 4;     // big_plan's, for that table
    info.lds_bytes = (int32_t)lds;
    info.table_doubles = (int64_t)tb.table.size();
    info.work_bytes_per_system = N * (4 + 4 + 4 + 1 + 8) + L * (4 + 4 + 8 + 8) + L * p->K * 4 + nblk * 8;
    info.output_bytes = S * ((want_states ? O * N * 6 : 0) + (want_scalars ? O * GIL_NSCALARS * 8 : 0) + N * 24 + 24);
    if (lds > 160 * 1024)
        return bad("the launch needs " + num(lds) + " bytes of LDS per system (n_cap = " + num(N) + ", longest table kept in LDS " +
                   num(info.max_tlen_lds) + "), more than the " + num(160 * 1024) + " bytes (160 KB) of a workgroup");
    return gil_refuse_plan_bytes(who, err, S * info.work_bytes_per_system, info.output_bytes);
}

// The large-system kernel of variant V: the one place that names the instantiation.  Raises its LDS limit and launches it; the
// timed window holds this launch alone.
template <GilKind V>
int big_launch(OneShot &job, int S, size_t lds, const typename BigKernelArgs<V>::type &a) {
    const auto kernel = &gil_big_kernel<V>;
    if (int rc = job.raise_lds_limit(reinterpret_cast<const void *>(kernel), lds)) return rc;
    job.ev.start();
    hipLaunchKernelGGL(kernel, dim3((unsigned)S), dim3(BT), lds, nullptr, a);
    job.ev.stop();
    return 0;
}

}  // namespace

// The one host driver of the large-system kernel (hidden: the entry points of gillespie_hip.hip call it too): S = p->n_systems
// systems, one workgroup each.  The callers have checked their required pointers and S.  pos0 / sigma0 / bound0 hold [S][n_cap]
// entries (a single system: its n0[0] particles).
int gil_large_run(const char *who, std::string &err, const gil_params *p, const GilIo &io, const GilExtras &ex) {
    auto bad = [&](const std::string &m) { err = std::string(who) + ": " + m; return GIL_ERR_ARG; };
    gilm_plan_info info{};
    std::vector<double> table;
    const gilx_variants *mx = ex.mx;                          // a mixed launch (gilxm_run; with ex.rs gilxmr_run): a variant per system
    gilxm_plan_info xinfo{}; GilxTables tb;
    if (mx) {
        if (int rc = gilxm_decide(who, err, p, mx, io.states(), io.scalars_obs != nullptr, xinfo, tb)) return rc;
        info.n_systems = xinfo.n_systems; info.n_blocks = xinfo.n_blocks; info.table_len = xinfo.max_tlen; info.lds_bytes = xinfo.lds_bytes;
        info.work_bytes_per_system = xinfo.work_bytes_per_system; info.output_bytes = xinfo.output_bytes;
        table = std::move(tb.table);
    } else if (int rc = big_plan(who, err, p, io.states(), io.scalars_obs != nullptr, &info, &table)) return rc;
    const int S = p->n_systems, L = p->L, N = p->n_cap;
    const GilcCall *cap = ex.cap; const GilpCall *prof = ex.prof; GilrCall *rs = ex.rs;
    if (ex.structure_obs) {                                   // rows of structure sums (gils_run)
        info.lds_bytes += (int32_t)(gils_lds_doubles(BT) * sizeof(double));
        info.output_bytes += (int64_t)S * p->n_obs * (4 + 2 * (int64_t)ex.k_max) * 8;
    }
    if (cap) {                                                // of capture counts (gilc_run)
        info.lds_bytes += (int32_t)(gilc_lds_slots(BT, cap->n_groups, cap->c_bins, cap->h_bins) * 8);
        info.output_bytes += (int64_t)S * (p->n_obs * (int64_t)(GILC_FIXED + cap->n_groups + cap->c_bins) * 8 + 2 * (int64_t)cap->h_bins * 8 + 32);
    }
    if (prof) {                                               // of ensemble profiles (gilp_run)
        info.lds_bytes += (int32_t)gilp_lds_bytes(prof->n_bins, prof->want_field != 0);
        info.output_bytes = gilp_output_bytes(p, prof->n_groups, prof->n_bins, io.states(), prof->profile_obs != nullptr);
    }
    if (info.lds_bytes > 160 * 1024) return bad("LDS budget exceeded");
    // a resumable launch (rs: its start state, checked by gilr_prepare, which comes back as the end state) reads no n0 / pos0 /
    // sigma0 / bound0: every slot's site, and its spin or 0 where it is not alive
    GilIo in = io;
    std::vector<int32_t> n0_all;
    std::vector<int8_t> spin_all;
    if (rs) {
        n0_all.assign((size_t)S, N);
        spin_all.resize(rs->flg.size());
        for (size_t q = 0; q < spin_all.size(); ++q) spin_all[q] = (rs->flg[q] & GILR_ALIVE) ? ((rs->flg[q] & GILR_PLUS) ? 1 : -1) : 0;
        in.n0 = n0_all.data(); in.pos0 = rs->pos.data(); in.sigma0 = spin_all.data(); in.bound0 = nullptr;
    } else { const std::string why = gil_check_start(p, io, mx ? nullptr : "bad n_cap / n0 / n_obs / max_events"); if (!why.empty()) return bad(why); }
    if (const char *why = gil_check_flip_table(p)) return bad(why);
    // a mixed launch: the system of every workgroup (default: falling n0, ties by index -- the long systems start first when more
    // are queued than fit), and every system's Philox key (default: p->seed + s in 64 bits, gilm_run's) and stream (default: 0)
    std::vector<int32_t> order, stream;
    std::vector<uint64_t> seed;
    if (mx) {
        order.resize((size_t)S); stream.resize((size_t)S); seed.resize((size_t)S);
        for (int s = 0; s < S; ++s) {
            order[(size_t)s] = mx->order ? mx->order[s] : s; stream[(size_t)s] = mx->stream ? mx->stream[s] : 0;
            seed[(size_t)s] = mx->seed ? mx->seed[s] : p->seed + (uint64_t)s;
        }
        const int32_t *slots = rs ? rs->n_slots.data() : io.n0;   // a resumable mixed launch: the checkpoint's slot counts
        if (!mx->order) std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return slots[x] > slots[y]; });
    }
    OneShot job{who, err, true, GIL_ERR_NODEVICE, GIL_ERR_ARG, GIL_ERR_HIP};   // zero-fill: the scratch arrays start from zero
    if (int rc = job.select_device(p->device)) return rc;
    const int64_t work_bytes = (int64_t)S * info.work_bytes_per_system + (ex.structure_obs ? (int64_t)L * 16 : 0) +
                               (cap ? (int64_t)S * N * 8 + (cap->n_groups > 0 ? (int64_t)L * 4 : 0) : 0) + (prof ? (int64_t)S * 4 : 0);
    if (int rc = gil_refuse_device_bytes(job, work_bytes, info.output_bytes)) return rc;
    GilpBigArgs a{};
    a.p = *p; a.tlen = info.table_len; a.nblk = info.n_blocks; a.cb = (a.nblk + BT - 1) / BT;
    a.tab_in_lds = info.table_in_lds;
    a.m = gil_model(p);
    if (mx) { a.p.sigma_grid = 0.0; a.p.block_table = nullptr; }   // ignored: the kernel takes every system's own
    const size_t SN = (size_t)S * N, SL = (size_t)S * L, KK = (size_t)(p->K + 1) * (p->K + 1);
    if (int rc = gil_stage_common(job, a, p, in, table, S == 1 && !rs ? (size_t)in.n0[0] : SN, io.scalars_obs != nullptr,
                                  mx ? mx->block_table : p->block_table, mx ? (size_t)mx->n_variants * KK : KK)) return rc;
    WORK(pos, SN); WORK(occ, SL); WORK(occp, SL); WORK(slot, SL * p->K); WORK(work, SN); WORK(ref, SN);
    WORK(flg, SN); WORK(rate, SN); WORK(bsum, (size_t)S * a.nblk); WORK(W, SL); WORK(S, SL);
    const size_t lds = (size_t)info.lds_bytes;
    GilprBigArgs b{};                                           // the resumable launches' arguments: a's own, the checkpoint and (gilpr_run) the profile's
    int rc = ex.structure_obs ? gil_stage_structure(job, a, p, ex.k_max, ex.first_obs, true, false)
             : cap            ? gil_stage_capture(job, a, p, *cap, true)
             : prof           ? gil_stage_profile(job, a, p, *prof) : 0;
    if (rc) return rc;
    if (rs && (rc = gil_stage_checkpoint(job, b.rs, p, *rs, false))) return rc;
    if ((rc = job.create_events())) return rc;
    static_cast<BigArgs &>(b) = a; b.pf = a.pf;
    GilxprBigArgs c{};                                          // the mixed launch's arguments: a's own and the variants (and, resumable,
    static_cast<BigArgs &>(c) = a;                              //   the checkpoint: GilxBigArgs is its base; gilxpr_run: the profile's too)
    c.rs = b.rs; c.pf = a.pf;
    GilxpBigArgs d{};                                           // the mixed profile launch's: the mixed launch's own and the profile's (below)
    if (mx) {
        c.tab_region = xinfo.max_tlen_lds >= 0 ? ((xinfo.max_tlen_lds + 2) & ~1) : 0;
        c.mx.has_block = mx->block_table ? 1 : 0;
        if ((rc = job.upload(&c.mx.order, order.data(), (size_t)S, "order"))) return rc;
        if ((rc = job.upload(&c.mx.variant_of_system, mx->variant_of_system, (size_t)S, "variant_of_system"))) return rc;
        if ((rc = job.upload(&c.mx.variants, tb.var.data(), tb.var.size(), "variants"))) return rc;
        if ((rc = job.upload(&c.mx.seed, seed.data(), (size_t)S, "seed"))) return rc;
        if ((rc = job.upload(&c.mx.stream, stream.data(), (size_t)S, "stream"))) return rc;
        static_cast<GilxBigArgs &>(d) = c; d.pf = a.pf;
    }
    const dim3 field_grid((unsigned)((L + 255) / 256), (unsigned)S);   // W, S of the start state: before the timed window
    if (rs && mx) hipLaunchKernelGGL(big_field_init_live_mixed, field_grid, dim3(256), 0, nullptr, static_cast<const GilxBigArgs &>(c));
    else if (rs) hipLaunchKernelGGL(big_field_init_live, field_grid, dim3(256), 0, nullptr, static_cast<const BigArgs &>(a));
    else if (mx) hipLaunchKernelGGL(big_field_init_mixed, field_grid, dim3(256), 0, nullptr, static_cast<const GilxBigArgs &>(c));
    else hipLaunchKernelGGL(big_field_init, field_grid, dim3(256), 0, nullptr, static_cast<const BigArgs &>(a));
    rc = ex.structure_obs ? big_launch<GilKind::Structure>(job, S, lds, a)
         : cap            ? big_launch<GilKind::Capture>(job, S, lds, a)
         : mx && prof && rs ? big_launch<GilKind::MixedProfileResume>(job, S, lds, c)
         : mx && prof     ? big_launch<GilKind::MixedProfile>(job, S, lds, d)
         : prof && rs     ? big_launch<GilKind::ProfileResume>(job, S, lds, b)
         : prof           ? big_launch<GilKind::Profile>(job, S, lds, a)
         : mx && rs       ? big_launch<GilKind::MixedResume>(job, S, lds, c)
         : mx             ? big_launch<GilKind::Mixed>(job, S, lds, c)
         : rs             ? big_launch<GilKind::Resume>(job, S, lds, b) : big_launch<GilKind::Plain>(job, S, lds, a);
    if (rc) return rc;
    if ((rc = job.finish(hipGetLastError(), "gil_big_kernel", io.kernel_ms))) return rc;
    if ((rc = gil_fetch_common(job, a, p, io))) return rc;
    if (ex.structure_obs) rc = gil_fetch_structure(job, a, p, ex.structure_obs);
    else if (cap) rc = gil_fetch_capture(job, a, p, *cap);
    else if (prof) rc = gil_fetch_profile(job, a, p, *prof);
    if (!rc && rs) rc = gil_fetch_checkpoint(job, *rs, p, a.pos, a.ref, a.flg);
    return rc ? rc : GIL_OK;
}

int gil_large_plan(const char *who, std::string &err, const gil_params *p, int32_t extra_lds, int32_t *lds_bytes, int64_t *work_bytes) {
    if (p->n_systems > GILM_MAX_SYSTEMS) { err = std::string(who) + ": n_systems must be in [1, GILM_MAX_SYSTEMS]"; return GIL_ERR_ARG; }
    gilm_plan_info info{};
    if (int rc = big_plan(who, err, p, false, false, &info, nullptr)) return rc;
    *lds_bytes = info.lds_bytes + extra_lds;
    *work_bytes = (int64_t)p->n_systems * info.work_bytes_per_system;
    if (*lds_bytes > 160 * 1024) { err = std::string(who) + ": LDS budget exceeded"; return GIL_ERR_ARG; }
    return GIL_OK;
}

int gil_large_mixed_plan(const char *who, std::string &err, const gil_params *p, const gilx_variants *v, bool want_states, int32_t extra_lds,
                         int32_t *lds_bytes, int64_t *work_bytes, int32_t *max_tlen, int64_t *table_doubles) {
    gilxm_plan_info info{}; GilxTables tb;
    if (int rc = gilxm_decide(who, err, p, v, want_states, true, info, tb)) return rc;
    *lds_bytes = info.lds_bytes + extra_lds;
    *work_bytes = (int64_t)p->n_systems * info.work_bytes_per_system;
    *max_tlen = info.max_tlen; *table_doubles = info.table_doubles;
    if (*lds_bytes > 160 * 1024) { err = std::string(who) + ": LDS budget exceeded"; return GIL_ERR_ARG; }
    return GIL_OK;
}

extern "C" {

int gil_run_large(const gil_params *p, int32_t n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0,
                  const double *uniforms, int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int32_t *n_recorded,
                  int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, double *kernel_ms) {
    auto bad = [&](const char *m) { g_big_err = std::string("gil_run_large: ") + m; return GIL_ERR_ARG; };
    if (!p || !pos0 || !sigma0 || !p->beta || !p->times_obs) return bad("null argument");
    if (p->n_systems != 1) return bad("one system per call");
    const GilIo io{&n0, pos0, sigma0, bound0, uniforms, pos_obs, sigma_obs, flags_obs, nullptr, n_recorded, n_events, t_final, exits, n_exits, kernel_ms};
    return gil_large_run("gil_run_large", g_big_err, p, io, GilExtras{});
}

const char *gil_large_last_error(void) { return g_big_err.c_str(); }

const char *gilm_last_error(void) { return g_many_err.c_str(); }

const char *gilxm_last_error(void) { return g_gilxm_err.c_str(); }

int gilxm_plan(const gil_params *p, const gilx_variants *v, int32_t want_states, gilxm_plan_info *out) {
    if (!p || !v || !out) { g_gilxm_err = "gilxm_plan: null argument"; return GIL_ERR_ARG; }
    gilxm_plan_info info; GilxTables tb;
    if (int rc = gilxm_decide("gilxm_plan", g_gilxm_err, p, v, want_states != 0, true, info, tb)) return rc;
    *out = info;
    return GIL_OK;
}

int gilxm_run(const gil_params *p, const gilx_variants *v, const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0,
              const double *uniforms, int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs,
              int32_t *n_recorded, int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, double *kernel_ms) {
    if (!p || !v || !n0 || !pos0 || !sigma0 || !p->beta || !p->times_obs || !v->variant_of_system) { g_gilxm_err = "gilxm_run: null argument"; return GIL_ERR_ARG; }
    const GilIo io{n0, pos0, sigma0, bound0, uniforms, pos_obs, sigma_obs, flags_obs, scalars_obs, n_recorded, n_events, t_final, exits, n_exits, kernel_ms};
    GilExtras ex;
    ex.mx = v;
    return gil_large_run("gilxm_run", g_gilxm_err, p, io, ex);
}

int gilm_plan(const gil_params *p, int32_t want_states, int32_t want_scalars, gilm_plan_info *out) {
    auto bad = [&](const char *m) { g_many_err = std::string("gilm_plan: ") + m; return GIL_ERR_ARG; };
    if (!p || !out) return bad("null argument");
    if (p->n_systems < 1 || p->n_systems > GILM_MAX_SYSTEMS) return bad("n_systems must be in [1, GILM_MAX_SYSTEMS]");
    return big_plan("gilm_plan", g_many_err, p, want_states != 0, want_scalars != 0, out, nullptr);
}

int gilm_run(const gil_params *p, const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0,
             const double *uniforms, int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs,
             int32_t *n_recorded, int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, double *kernel_ms) {
    auto bad = [&](const char *m) { g_many_err = std::string("gilm_run: ") + m; return GIL_ERR_ARG; };
    if (!p || !n0 || !pos0 || !sigma0 || !p->beta || !p->times_obs) return bad("null argument");
    if (p->n_systems < 1 || p->n_systems > GILM_MAX_SYSTEMS) return bad("n_systems must be in [1, GILM_MAX_SYSTEMS]");
    const GilIo io{n0, pos0, sigma0, bound0, uniforms, pos_obs, sigma_obs, flags_obs, scalars_obs, n_recorded, n_events, t_final, exits, n_exits, kernel_ms};
    return gil_large_run("gilm_run", g_many_err, p, io, GilExtras{});
}

}  // extern "C"
