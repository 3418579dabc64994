// gillespie_hip.hip -- MI355X (gfx950) implementation of the C ABI in include/gillespie.h.
//
// The reference's exact event loop (PARTICLE_solver_CLASS.py:511-538) for many independent systems at once: one
// PERSISTENT workgroup per system, the whole system in LDS (particles, site occupancy, the smoothed histograms
// W = tot_conv and S = s_conv, the weight table, the per-particle rates).  One loop iteration = one event:
//   A  every thread evaluates the rate table of its particles (ref :254-352) from m = clip(S/W)[pos] and the
//      occupancy of the neighbouring sites, workgroup scan of the totals -> R
//   B  waiting time ~ Exp(R), particle ~ rates / R (searchsorted over the running sums, like Generator.choice),
//      event type by the reference's threshold order diffuse < active < bind < unbind < exit < flip (ref :358-367)
//   C  one thread applies the event (ref :371-446)
//   D  all threads add the event's change of W, S on the sites in reach (the reference recomputes the whole field
//      before every event, :512; the weights sit on the exact grid of DESIGN.md, so the incremental sums equal a
//      recomputation bit for bit)
//   E  t += tau; states / scalar sums of the observation times that were crossed go to HBM (ref :517-536)
// Randomness: Philox4x32-10 keyed by the seed, counter (event index, system) -- or numbers supplied by the caller.
// Host side: every extern "C" run function fills a GilIo and a GilExtras (gillespie_common.hpp) and calls batch_run, mixed_run or,
// for the large shape, gil_large_run of gillespie_big_hip.hip (the resumable ones, the profile segments of
// include/gillespie_profile_resume.h among them, through gilr_drive / gilxr_drive); the drivers stage and fetch through the helpers of
// gillespie_common.hpp, and gil_launch<V> is the one place that names a kernel instantiation.

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "gillespie.h"
#include "gillespie_structure.h"
#include "gillespie_capture.h"
#include "gillespie_profile.h"
#include "gillespie_mixed.h"
#include "gillespie_mixed_structure.h"
#include "gillespie_mixed_profile.h"
#include "gillespie_resume.h"
#include "gillespie_mixed_resume.h"
#include "gillespie_profile_resume.h"
#include "aps_common.hpp"
#include "gillespie_common.hpp"           // the call record, the variant tags, the staging path of the drivers
#include "gillespie_structure.hpp"        // the structure sums of an observation (structure instantiations only)
#include "gillespie_capture.hpp"          // anchor capture and cluster statistics (capture instantiations only)
#include "gillespie_profile.hpp"          // ensemble density and field profiles (profile instantiations only)
#include "gillespie_mixed.hpp"            // a variant per system: table, blocking table, slots, Philox key (mixed instantiations only)
#include "gillespie_window.hpp"           // the window sums of the structure rows (mixed structure instantiations only)
#include "gillespie_resume.hpp"           // start and end state of a launch (resumable instantiations only)

namespace {

std::string g_gil_err;
enum { F_PLUS = 1, F_BOUND = 2, F_ALIVE = 4 };
enum { GS_N = 0, GS_SPIN, GS_POS, GS_WALL, GS_MAXPOS, GS_FRONT, GS_ATTEMPT, GS_BLOCKED, GS_DISP, GS_DISP2, GS_NDISP, GS_EVENTS };

struct GilArgs {
    Model m;
    gil_params p;
    int tlen, chunk;
    const double *betas, *table, *times, *uniforms;
    const uint8_t *anchor, *block_table;
    const int32_t *front_lo, *n0, *pos0;
    const int8_t *sigma0;
    const uint8_t *bound0;
    int32_t *pos_obs; int8_t *sigma_obs; uint8_t *flags_obs; long long *scalars;
    int32_t *n_recorded; long long *n_events; double *t_final, *exits; int32_t *n_exits;
};

template <int NT>
__device__ inline long long wg_sum_ll(long long v, long long *red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    long long s = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) s += red[w];
    return s;
}

struct GilsBatchArgs : GilArgs { GilsArgs st; };            // arguments of the structure instantiations
struct GilcBatchArgs : GilsBatchArgs { GilcArgs cp; };      // arguments of the capture instantiations
struct GilpBatchArgs : GilcBatchArgs { GilpArgs pf; };      // arguments of the profile instantiations (the driver's one struct)
struct GilxBatchArgs : GilArgs { GilxArgs mx; };            // arguments of the mixed instantiations (gilx_run's driver)
struct GilxsBatchArgs : GilxBatchArgs { GilsArgs st; GilwArgs wn; };   // arguments of the mixed structure instantiations (gilxs_run's)
struct GilrBatchArgs : GilArgs { GilrArgs rs; };            // arguments of the resumable instantiations (gilr_run's)
struct GilxrBatchArgs : GilxBatchArgs { GilrArgs rs; };     // arguments of the resumable mixed instantiations (gilxr_run's)
struct GilxsrBatchArgs : GilxsBatchArgs { GilrArgs rs; };   // arguments of the resumable mixed structure instantiations (gilxsr_run's)
struct GilxpBatchArgs : GilxBatchArgs { GilpArgs pf; };     // arguments of the mixed profile instantiations (gilxp_run's)
struct GilxDriverArgs : GilxsrBatchArgs { GilpArgs pf; };   // mixed_run's one struct: what every mixed launch takes is in it
struct GilprBatchArgs : GilrBatchArgs { GilpArgs pf; };     // arguments of the resumable profile instantiations (gilpr_run's)
struct GilxprBatchArgs : GilxrBatchArgs { GilpArgs pf; };   // arguments of the resumable mixed profile instantiations (gilxpr_run's)

// the argument struct of each variant of the batch kernel
template <GilKind V> struct GilKernelArgs;
template <> struct GilKernelArgs<GilKind::Plain> { using type = GilArgs; };
template <> struct GilKernelArgs<GilKind::Structure> { using type = GilsBatchArgs; };
template <> struct GilKernelArgs<GilKind::Capture> { using type = GilcBatchArgs; };
template <> struct GilKernelArgs<GilKind::Profile> { using type = GilpBatchArgs; };
template <> struct GilKernelArgs<GilKind::Mixed> { using type = GilxBatchArgs; };
template <> struct GilKernelArgs<GilKind::MixedStructure> { using type = GilxsBatchArgs; };
template <> struct GilKernelArgs<GilKind::Resume> { using type = GilrBatchArgs; };
template <> struct GilKernelArgs<GilKind::MixedResume> { using type = GilxrBatchArgs; };
template <> struct GilKernelArgs<GilKind::MixedStructureResume> { using type = GilxsrBatchArgs; };
template <> struct GilKernelArgs<GilKind::MixedProfile> { using type = GilxpBatchArgs; };
template <> struct GilKernelArgs<GilKind::ProfileResume> { using type = GilprBatchArgs; };
template <> struct GilKernelArgs<GilKind::MixedProfileResume> { using type = GilxprBatchArgs; };

// the structure sums' slots: behind the loop's own LDS (which ends with the plus-occupancy bytes), at the next multiple of 8
__device__ __forceinline__ double *gils_slots(double *lds, uint8_t *occp, int L) {
    const size_t end = (size_t)(reinterpret_cast<char *>(occp + ((L + 15) & ~15)) - reinterpret_cast<char *>(lds));
    return lds + ((end + 7) >> 3);
}

// NT = threads per system: one wavefront (no real barriers, six systems per CU by LDS) for small systems, four for large ones.
// V = the variant, a compile-time property, so that each kernel is the code it was before the others existed:
//   Structure       also reduce the structure sums at an observation (gillespie_structure.hpp);
//   Capture         anchor capture and cluster statistics (gillespie_capture.hpp);
//   Profile         ensemble density and field profiles (gillespie_profile.hpp);
//   Mixed           a mixed batch (gillespie_mixed.hpp): the system of a workgroup comes from a launch order, and the weight table,
//                   the blocking table, the slot count and the Philox key are the system's own.  In such a launch a.tlen is the
//                   longest table's length (the LDS layout is the launch's);
//   MixedStructure  the structure sums of a mixed launch, with the window reduction of gillespie_window.hpp; the rows themselves
//                   are optional there;
//   Resume          a resumable launch (gillespie_resume.hpp): the start state is a checkpoint (slots may be dead, the clock, the
//                   event count and the next observation are the checkpoint's) and the end state is written out.
//   MixedResume, MixedStructureResume  a resumable mixed launch (include/gillespie_mixed_resume.h): Mixed / MixedStructure with the
//                   start and end of Resume.  a.n0 holds the checkpoint's slot counts, so the system's loops and its chunk are
//                   those of the run's start, and the loops ask the flags; the end state beyond these slots is written as
//                   empty.  With the structure sums, st.first_obs counts within the launch's slice (the host subtracts the
//                   slice's first index), and the window's accumulators and counts start from the checkpoint's.
//   MixedProfile    the ensemble profiles of a mixed launch (include/gillespie_mixed_profile.h): Mixed with the observation pass of
//                   Profile over the system's own slots (those beyond were never loaded) and with the system's own field mode;
//                   the profile slots lie behind the launch's layout, which a.tlen = the longest table fixes.
//   ProfileResume, MixedProfileResume  a resumable profile launch (include/gillespie_profile_resume.h): the start and end of
//                   Resume / MixedResume with the observation pass of Profile / MixedProfile.  The observations a resumed start
//                   records before its first event go through the same pass, with the checkpoint's state and the global mean
//                   rebuilt from its live flags; pf.first_obs and the group rows count within the launch's slice (nobs rows).
template <int NT, GilKind V>
__global__ __launch_bounds__(NT) void gil_kernel(const typename GilKernelArgs<V>::type a) {
    constexpr bool XR = V == GilKind::MixedResume || V == GilKind::MixedStructureResume || V == GilKind::MixedProfileResume;   // MX and RS together
    constexpr bool ST = V == GilKind::Structure || V == GilKind::MixedStructure || V == GilKind::MixedStructureResume;
    constexpr bool CP = V == GilKind::Capture;
    constexpr bool PF = V == GilKind::Profile || V == GilKind::MixedProfile || V == GilKind::ProfileResume || V == GilKind::MixedProfileResume;
    constexpr bool MX = V == GilKind::Mixed || V == GilKind::MixedStructure || V == GilKind::MixedProfile || XR;
    constexpr bool RS = V == GilKind::Resume || V == GilKind::ProfileResume || XR;
    extern __shared__ double lds[];
    const Model &M = a.m;
    const GilxView vw = gilx_view<MX, NT>(a);                  // empty without MX
    const int L = M.L, K = M.K, t = threadIdx.x, sys = MX ? vw.sys : blockIdx.x, ncap = a.p.n_cap, nobs = a.p.n_obs;
// the launch's values, read where they are used as before MX existed, or with MX the system's own (MX is a constant: one arm is compiled)
#define GX_TLEN (MX ? vw.tlen : a.tlen)
#define GX_FIELD (MX ? vw.field_mode : M.field_mode)
#define GX_SLOTS (MX ? vw.nslots : ncap)
#define GX_CHUNK (MX ? vw.chunk : a.chunk)
#define GX_BLOCK (MX ? vw.block_table : a.block_table)
    double *W = lds, *S = W + L, *tab = S + L, *rate = tab + ((a.tlen + 2) & ~1), *red = rate + ncap + (ncap & 1);
    double *tinc = red + 8;                                   // [NT] inclusive scan of the threads' rate sums
    double *draws = tinc + NT;                                // [NT][4] -log1p(-u0), u1, u2, u3 of the next NT events
    long long *redl = reinterpret_cast<long long *>(draws + 4 * NT);   // [8]
    int *pos = reinterpret_cast<int *>(redl + 8);             // [ncap]
    int *ref = pos + ncap;                                    // [ncap] positions at the reference observation
    int *work = ref + ncap;                                   // [ncap] particles whose rates are re-evaluated before this event
    int *ctl = work + ncap;                                   // [16] broadcast slots
    uint8_t *flg = reinterpret_cast<uint8_t *>(ctl + 16);     // [ncap]
    uint8_t *occ = flg + ((ncap + 15) & ~15);                 // [L] particles per site
    uint8_t *occp = occ + ((L + 15) & ~15);                   // [L] plus particles per site (blocking table)
    const double beta = a.betas[sys];
    const int n_init = XR ? vw.nslots : (RS ? ncap : a.n0[sys]);   // RS: any slot may be alive, the loops below ask its flags
    // ---- load the system
    for (int i = t; i <= GX_TLEN; i += NT) tab[i] = (MX ? vw.table : a.table)[i];
    for (int x = t; x < L; x += NT) { occ[x] = 0; occp[x] = 0; }
    for (int i = t; i < GX_SLOTS; i += NT) {
        if constexpr (RS) {                                    // the checkpoint's slots: departed ones stay dead, origins are kept
            pos[i] = a.rs.pos[(size_t)sys * ncap + i]; flg[i] = a.rs.flg[(size_t)sys * ncap + i]; ref[i] = a.rs.ref[(size_t)sys * ncap + i];
            rate[i] = 0.0;
            continue;
        }
        const bool live = i < n_init;
        pos[i] = live ? a.pos0[(size_t)sys * ncap + i] : 0;
        flg[i] = live ? (uint8_t)(F_ALIVE | (a.sigma0[(size_t)sys * ncap + i] > 0 ? F_PLUS : 0) |
                                  ((a.bound0 && a.bound0[(size_t)sys * ncap + i]) ? F_BOUND : 0)) : 0;
        ref[i] = -1;
        rate[i] = 0.0;                                         // empty and departed slots keep rate zero
    }
    if constexpr (ST) {
        if (a.st.phase_in_lds) {
            double *ptab = gils_slots(lds, occp, L) + gils_lds_doubles(NT);
            for (int i = t; i < 2 * L; i += NT) ptab[i] = a.st.phase[i];
        }
    }
    if constexpr (CP) {                                        // the capture slots, and the bind times behind them
        const GilcLds cs = gilc_lds(gils_slots(lds, occp, L), a.cp, NT / 64);
        gilc_init<NT>(cs, a.cp, cs.tbind, ncap);
    }
    __syncthreads();
    if (t == 0) for (int i = 0; i < n_init; ++i) { if (RS && !(flg[i] & F_ALIVE)) continue; occ[pos[i]]++; if (flg[i] & F_PLUS) occp[pos[i]]++; }
    // field from scratch: W(x) = sum_j w(x, p_j), S(x) = sum_j sigma_j w(x, p_j)
    for (int x = t; x < L; x += NT) {
        double w = 0.0, s = 0.0;
        if (GX_FIELD)
            for (int j = 0; j < n_init; ++j) {
                if (RS && !(flg[j] & F_ALIVE)) continue;
                const double g = site_weight(M, tab, GX_TLEN, x, pos[j]);
                w += g; s += (flg[j] & F_PLUS) ? g : -g;
            }
        W[x] = w; S[x] = s;
    }
    __syncthreads();
    long long gsum_s = 0, gsum_n = 0;                          // global-mean mode: sum of spins, particles alive
    if (!GX_FIELD) {
        long long ls = 0, ln = 0;
        for (int i = t; i < n_init; i += NT) { if (RS && !(flg[i] & F_ALIVE)) continue; ls += (flg[i] & F_PLUS) ? 1 : -1; ln += 1; }
        gsum_s = wg_sum_ll<NT>(ls, redl); gsum_n = wg_sum_ll<NT>(ln, redl);
    }
    double tnow = 0.0;
    long long n_ev = 0;
    int k_obs = 0, n_exit = 0;
    // MX with ST only: observations the window took, and empty ones it met.  The other instantiations never read them, so
    // they cost no register there (their assembly is the parent's)
    [[maybe_unused]] int n_win = 0, n_emp = 0;
    if constexpr (XR && ST) { n_win = a.wn.n_window[sys]; n_emp = a.wn.n_empty[sys]; }   // the checkpoint's (zero on a fresh start)
    const int c0 = t * GX_CHUNK, c1 = min(GX_SLOTS, c0 + GX_CHUNK);

    auto record = [&](int k) {                                 // observation k: state and scalar sums (ref :517-536)
        const size_t o = ((size_t)sys * nobs + k) * ncap;
        long long v[GIL_NSCALARS] = {0, 0, 0, 0, -1, 0, 0, 0, 0, 0, 0, 0};
        if (k == a.p.ref_obs) for (int i = t; i < GX_SLOTS; i += NT) ref[i] = (flg[i] & F_ALIVE) ? pos[i] : -1;
        __syncthreads();
        for (int i = t; i < GX_SLOTS; i += NT) {
            const uint8_t f = flg[i];
            if (a.pos_obs) a.pos_obs[o + i] = pos[i];
            if (a.sigma_obs) a.sigma_obs[o + i] = (f & F_PLUS) ? 1 : -1;
            if (a.flags_obs) a.flags_obs[o + i] = (uint8_t)(((f & F_BOUND) ? 1 : 0) | ((f & F_ALIVE) ? 2 : 0));
            if (!(f & F_ALIVE)) continue;
            const int p = pos[i];
            v[GS_N] += 1; v[GS_SPIN] += (f & F_PLUS) ? 1 : -1; v[GS_POS] += p; v[GS_WALL] += p >= a.p.x_wall;
            v[GS_MAXPOS] = max(v[GS_MAXPOS], (long long)p);
            if ((f & F_PLUS) && p < L - 1) {
                v[GS_ATTEMPT] += 1;
                const int cp = occp[p + 1], cm = occ[p + 1] - occp[p + 1];
                v[GS_BLOCKED] += GX_BLOCK ? GX_BLOCK[cp * (K + 1) + cm] : (cp + cm >= 1);
            }
            if (ref[i] >= 0) { const long long d = (long long)p - ref[i]; v[GS_DISP] += d; v[GS_DISP2] += d * d; v[GS_NDISP] += 1; }
        }
        long long mx = v[GS_MAXPOS];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mx = max(mx, __shfl_xor(mx, off));
        __syncthreads();
        if ((t & 63) == 0) redl[4 + (t >> 6)] = mx;
        __syncthreads();
        mx = redl[4];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) mx = max(mx, redl[4 + w]);
        if (a.front_lo && mx >= 0) {
            const int lo = a.front_lo[mx];
            for (int i = t; i < GX_SLOTS; i += NT) if ((flg[i] & F_ALIVE) && pos[i] >= lo) v[GS_FRONT] += 1;
        }
        for (int q = 0; q < GIL_NSCALARS; ++q) {
            if (q == GS_MAXPOS || q == GS_EVENTS) continue;
            const long long s = wg_sum_ll<NT>(v[q], redl);
            if (t == 0 && a.scalars) a.scalars[((size_t)sys * nobs + k) * GIL_NSCALARS + q] = s;
        }
        if (t == 0 && a.scalars) {
            a.scalars[((size_t)sys * nobs + k) * GIL_NSCALARS + GS_MAXPOS] = mx;
            a.scalars[((size_t)sys * nobs + k) * GIL_NSCALARS + GS_EVENTS] = n_ev;
        }
        __syncthreads();
        if constexpr (ST) {
            const GilsArgs &sa = a.st;
            if (MX || k >= sa.first_obs) {                     // MX: the four site sums of every observation (the head rows)
                double mg = 0.0;                               // global-mean mode: the one value of every site (ref :219-221)
                if (!GX_FIELD && gsum_n > 0) { mg = (double)gsum_s / (double)gsum_n; mg = mg > 1.0 ? 1.0 : (mg < -1.0 ? -1.0 : mg); }
                if constexpr (MX) {
                    double *red = gils_slots(lds, occp, L);
                    const bool in = k >= sa.first_obs;         // Fourier work from first_obs on only: before it, no modes
                    const int kk = in ? sa.k_max : 0;
                    double *row = in && sa.rows ? sa.rows + ((size_t)sys * nobs + k) * (size_t)(4 + 2 * sa.k_max) : nullptr;
                    const GilwSink sink{a.wn.head + ((size_t)sys * nobs + k) * 4, a.wn.window + (size_t)sys * 3 * sa.k_max, n_win == 0};
                    if (sa.phase_in_lds) gils_record_row<NT>(row, kk, L, GX_SLOTS, pos, flg, occ, W, S, GX_FIELD != 0, mg, red + gils_lds_doubles(NT), red, work, sink);
                    else gils_record_row<NT>(row, kk, L, GX_SLOTS, pos, flg, occ, W, S, GX_FIELD != 0, mg, sa.phase, red, work, sink);
                    if (in) { if (gilw_live<NT>(red) > 0.0) n_win += 1; else n_emp += 1; }   // red: next written behind a barrier of the next observation
                } else {
                    double *row = sa.rows + ((size_t)sys * nobs + k) * (size_t)(4 + 2 * sa.k_max), *red = gils_slots(lds, occp, L);
                    // two calls: the gathers of the first are LDS reads, of the second global loads
                    if (sa.phase_in_lds) gils_record_row<NT>(row, sa.k_max, L, GX_SLOTS, pos, flg, occ, W, S, GX_FIELD != 0, mg, red + gils_lds_doubles(NT), red, work);
                    else gils_record_row<NT>(row, sa.k_max, L, GX_SLOTS, pos, flg, occ, W, S, GX_FIELD != 0, mg, sa.phase, red, work);
                }
            }
        }
        if constexpr (CP) {
            if (k >= a.cp.first_obs)
                gilc_record_row<NT>(a.cp.rows + ((size_t)sys * nobs + k) * (size_t)(GILC_FIXED + a.cp.n_groups + a.cp.c_bins),
                                    gilc_lds(gils_slots(lds, occp, L), a.cp, NT / 64), a.cp, L, ncap, flg, occ, n_exit);
        }
        if constexpr (PF) {
            if (k >= a.pf.first_obs) {
                double mg = 0.0;                               // global-mean mode: the one value of every site (ref :219-221)
                if (!GX_FIELD && gsum_n > 0) { mg = (double)gsum_s / (double)gsum_n; mg = mg > 1.0 ? 1.0 : (mg < -1.0 ? -1.0 : mg); }
                gilp_record<NT>(a.pf, gils_slots(lds, occp, L), (size_t)sys, k, nobs, L, GX_SLOTS, pos, flg, W, S, GX_FIELD != 0, mg);
            }
        }
    };

    double t_next;                                             // next observation time (kept in a register: no load per event)
    if constexpr (RS) {
        // a fresh start records row 0; a resumed one the observations the checkpoint's last event passed (in the uninterrupted
        // run that event recorded them, with this state), unless that event passed T
        tnow = a.rs.t[sys]; n_ev = a.rs.n_ev[sys]; k_obs = a.rs.k_start[sys];
        while (k_obs < nobs && (a.rs.fresh ? k_obs == 0 : (tnow <= a.p.T && a.times[k_obs] <= tnow))) { record(k_obs); ++k_obs; }
        t_next = k_obs < nobs ? a.times[k_obs] : INFINITY;
    } else {
        record(0);                                             // ref :489-508
        k_obs = 1;
        t_next = nobs > 1 ? a.times[1] : INFINITY;
    }
#ifdef APS_STAMPS
    unsigned long long st[5] = {0, 0, 0, 0, 0}, s0 = __builtin_amdgcn_s_memtime();
#define GSTAMP(k) { const unsigned long long s1_ = __builtin_amdgcn_s_memtime(); st[k] += s1_ - s0; s0 = s1_; }
#else
#define GSTAMP(k)
#endif
    long long ev_base = RS ? n_ev - NT : 0;                    // first event of the block of draws held in LDS (RS: none held, the first iteration draws)
    bool dirty_all = true;                                     // first event: every rate is evaluated
    int dirty_a = 0, dirty_b = 0;
    const int dirty_reach = (GX_FIELD ? GX_TLEN - 1 : 0) + 1;
    while (tnow < a.p.T && k_obs < nobs && n_ev < a.p.max_events) {
        // ---- A: rates (ref :254-352).  The reference recomputes every particle's rates before every event; here only
        // the particles whose inputs the last event changed are re-evaluated (field within the table's reach of the
        // event's sites, occupancy of the neighbouring sites) -- the others' rates are the values already in LDS.
        // (1) every thread lists its particles that need it (lanes that find none do not hold up the others: the
        //     expensive rate evaluation then runs once over the compacted list, a lane per listed particle)
        int nwork = 0;
        if (NT == 64) {                                        // one wavefront: ballot + mbcnt compaction, no LDS counter
            for (int k = 0; k < GX_CHUNK; ++k) {
                const int i = c0 + k;
                bool redo = i < c1 && (flg[i] & F_ALIVE);      // the rate of a particle that left was zeroed when it left
                if (redo && !dirty_all) {
                    int d0 = pos[i] - dirty_a, d1 = pos[i] - dirty_b;
                    d0 = d0 < 0 ? -d0 : d0; d1 = d1 < 0 ? -d1 : d1;
                    if (M.periodic) { d0 = min(d0, L - d0); d1 = min(d1, L - d1); }
                    redo = min(d0, d1) <= dirty_reach;
                }
                const unsigned long long m = __ballot(redo);
                if (redo) work[nwork + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = i;
                nwork += __popcll(m);
            }
        } else {
            if (t == 0) ctl[6] = 0;
            __syncthreads();
            for (int i = c0; i < c1; ++i) {
                if (!(flg[i] & F_ALIVE)) continue;
                bool redo = dirty_all;
                if (!redo) {
                    int d0 = pos[i] - dirty_a, d1 = pos[i] - dirty_b;
                    d0 = d0 < 0 ? -d0 : d0; d1 = d1 < 0 ? -d1 : d1;
                    if (M.periodic) { d0 = min(d0, L - d0); d1 = min(d1, L - d1); }
                    redo = min(d0, d1) <= dirty_reach;
                }
                if (redo) work[atomicAdd(&ctl[6], 1)] = i;
            }
            __syncthreads();
            nwork = ctl[6];
        }
        __syncthreads();
        for (int j = t; j < nwork; j += NT) {
            const int i = work[j], p = pos[i];
            const uint8_t f = flg[i];
            double w, s;
            if (GX_FIELD) { w = W[p]; s = S[p]; } else { w = (double)gsum_n; s = (double)gsum_s; }
            double mloc = 0.0;
            if (w > 0.0) { mloc = s / w; mloc = mloc > 1.0 ? 1.0 : (mloc < -1.0 ? -1.0 : mloc); }
            int l = p - 1, rr = p + 1;
            if (M.periodic) { l = l < 0 ? l + L : l; rr = rr >= L ? rr - L : rr; }
            rate[i] = channels(M, a.anchor ? a.anchor[p] != 0 : false, p, (f & F_PLUS) ? 1 : -1, (f & F_BOUND) != 0, mloc, beta,
                               occ[p], l >= 0 ? occ[l] : 0, rr < L ? occ[rr] : 0).total;
        }
        __syncthreads();
        double mine = 0.0;
        for (int i = c0; i < c1; ++i) mine += rate[i];
        double inc;                                            // inclusive scan over the threads
        if (NT == 64) inc = wave_scan_inclusive(mine);
        else {
            inc = mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) { const double o = __shfl_up(inc, off); if ((t & 63) >= off) inc += o; }
            __syncthreads();
            if ((t & 63) == 63) red[t >> 6] = inc;
            __syncthreads();
            double before = 0.0;
            for (int w = 0; w < (t >> 6); ++w) before += red[w];
            inc += before;
        }
        tinc[t] = inc;
        GSTAMP(0)
        // ---- B: draws (ref :358-362): the numbers of NT consecutive events are produced together, a lane per event
        if ((n_ev - ev_base) >= NT || n_ev == 0) {
            ev_base = n_ev;
            const long long evn = n_ev + t;
            double u0, u1, u2, u3;
            if (a.uniforms) {
                const bool in = evn < a.p.max_events;
                const double *src = a.uniforms + ((size_t)sys * a.p.max_events + (in ? evn : 0)) * 4;
                u0 = in ? src[0] : 0.0; u1 = in ? src[1] : 0.0; u2 = in ? src[2] : 0.0; u3 = in ? src[3] : 0.0;
            } else {
                uint32_t x[4], y[4];
                philox4x32_10((uint32_t)evn, (uint32_t)(evn >> 32), MX ? vw.stream : (uint32_t)sys, 0x47494C31u, MX ? vw.seed_lo : M.seed_lo, MX ? vw.seed_hi : M.seed_hi, x);
                philox4x32_10((uint32_t)evn, (uint32_t)(evn >> 32), MX ? vw.stream : (uint32_t)sys, 0x47494C32u, MX ? vw.seed_lo : M.seed_lo, MX ? vw.seed_hi : M.seed_hi, y);
                u0 = ((double)(x[0] >> 5) * 67108864.0 + (double)(x[1] >> 6)) * 0x1.0p-53;
                u1 = ((double)(x[2] >> 5) * 67108864.0 + (double)(x[3] >> 6)) * 0x1.0p-53;
                u2 = ((double)(y[0] >> 5) * 67108864.0 + (double)(y[1] >> 6)) * 0x1.0p-53;
                u3 = ((double)(y[2] >> 5) * 67108864.0 + (double)(y[3] >> 6)) * 0x1.0p-53;
            }
            draws[4 * t] = -log1p(-u0); draws[4 * t + 1] = u1; draws[4 * t + 2] = u2; draws[4 * t + 3] = u3;
        }
        if (t == 0) ctl[0] = NT;                               // first thread whose running sum exceeds the target
        __syncthreads();
        const double R = tinc[NT - 1];
        if (!(R > 0.0)) { tnow = INFINITY; break; }           // ref :355: tau = inf ends the loop
        const double *dr = draws + 4 * (int)(n_ev - ev_base);
        const double u[4] = {0.0, dr[1], dr[2], dr[3]};
        const double tau = (1.0 / R) * dr[0];
        const double target = u[1] * R;
        int tsel;
        if (NT == 64) {                                        // one wavefront: the choice is a ballot
            const unsigned long long above = __ballot(inc > target && mine > 0.0), any = __ballot(mine > 0.0);
            tsel = above ? __builtin_ctzll(above) : 63 - __builtin_clzll(any);   // target rounded past the total: last lane with any rate
        } else {
            if (inc > target && mine > 0.0) atomicMin(&ctl[0], t);
            __syncthreads();
            tsel = ctl[0];
            if (tsel >= NT) {                                  // target rounded past the total: last thread that has any rate
                if (t == 0) ctl[1] = -1;
                __syncthreads();
                if (mine > 0.0) atomicMax(&ctl[1], t);
                __syncthreads();
                tsel = ctl[1];
            }
        }
        GSTAMP(1)
        // ---- C: the chosen thread picks the particle and applies the event (ref :363-446)
        if (t == tsel) {
            double run = tinc[t] - mine;
            int isel = -1;
            for (int i = c0; i < c1; ++i) {
                if (rate[i] > 0.0) { isel = i; run += rate[i]; if (run > target) break; }
            }
            const int i = isel, p = pos[i];
            uint8_t f = flg[i];
            const bool plus = (f & F_PLUS) != 0;
            double w, s;
            if (GX_FIELD) { w = W[p]; s = S[p]; } else { w = (double)gsum_n; s = (double)gsum_s; }
            double mloc = 0.0;
            if (w > 0.0) { mloc = s / w; mloc = mloc > 1.0 ? 1.0 : (mloc < -1.0 ? -1.0 : mloc); }
            int l = p - 1, rr = p + 1;
            if (M.periodic) { l = l < 0 ? l + L : l; rr = rr >= L ? rr - L : rr; }
            const Channels c = channels(M, a.anchor ? a.anchor[p] != 0 : false, p, plus ? 1 : -1, (f & F_BOUND) != 0, mloc, beta,
                                        occ[p], l >= 0 ? occ[l] : 0, rr < L ? occ[rr] : 0);
            const double v = u[2] * c.total;
            const double e_diff = c.diff, e_act = e_diff + c.act, e_bind = e_act + c.bind, e_unbind = e_bind + c.unbind,
                         e_exit = e_unbind + c.leave;
            int kind = 0, to = p;                              // 0 nothing, 1 hop, 2 flip, 3 exit
            if (v < e_diff) {
                if (c.left + c.right > 0.0) { kind = 1; to = (u[3] < c.left / (c.left + c.right)) ? p - 1 : p + 1; }
            } else if (v < e_act) { kind = 1; to = p + 1; }
            else if (v < e_bind) {
                f |= F_BOUND;
                if constexpr (CP) { const GilcLds cs = gilc_lds(gils_slots(lds, occp, L), a.cp, NT / 64); gilc_on_bind(cs, cs.tbind, i, tnow); }
            } else if (v < e_unbind) {
                f &= (uint8_t)~F_BOUND;
                if constexpr (CP) { const GilcLds cs = gilc_lds(gils_slots(lds, occp, L), a.cp, NT / 64); gilc_on_unbind(cs, a.cp, cs.tbind, i, tnow); }
            }
            else if (v < e_exit) kind = 3;
            else kind = 2;
            if (kind == 1) {
                if (M.periodic) to = to < 0 ? to + L : (to >= L ? to - L : to);
                else to = to < 0 ? 0 : (to > L - 1 ? L - 1 : to);
                occ[p]--; occ[to]++;
                if (plus) { occp[p]--; occp[to]++; }
                pos[i] = to;
                if (to == p) kind = 0;                         // clipped at a wall: nothing moved
            } else if (kind == 2) {
                f ^= F_PLUS;
                if (plus) occp[p]--; else occp[p]++;
            } else if (kind == 3) {
                f &= (uint8_t)~F_ALIVE;
                rate[i] = 0.0;
                occ[p]--; if (plus) occp[p]--;
                if (a.exits && n_exit < ncap) {
                    double *row = a.exits + ((size_t)sys * ncap + n_exit) * 3;
                    row[0] = tnow; row[1] = (double)p; row[2] = (double)i;
                }
                if constexpr (CP) { const GilcLds cs = gilc_lds(gils_slots(lds, occp, L), a.cp, NT / 64); gilc_on_exit(cs, a.cp, cs.tbind, i, p, (f & F_BOUND) != 0, tnow); }
            }
            flg[i] = f;
            ctl[2] = kind; ctl[3] = p; ctl[4] = to; ctl[5] = plus ? 1 : -1;
        }
        __syncthreads();
        GSTAMP(2)
        // ---- D: the event's change of the smoothed histograms
        const int kind = ctl[2], p_old = ctl[3], p_new = ctl[4], sg = ctl[5];
        if (kind == 3) n_exit += 1;
        // whose rates must be re-evaluated before the next event: everybody when the global mean moved, otherwise the
        // particles within the table's reach (+1 site for the occupancy of neighbours) of the event's sites
        dirty_a = p_old; dirty_b = p_new;
        dirty_all = !GX_FIELD && (kind == 2 || kind == 3);
        if (!GX_FIELD) {
            if (kind == 2) gsum_s -= 2 * sg;
            else if (kind == 3) { gsum_s -= sg; gsum_n -= 1; }
        } else if (kind != 0) {
            const int Rt = GX_TLEN - 1;
            const int centre = kind == 1 ? min(p_old, p_new) : p_old, span = kind == 1 ? 1 : 0;
            const bool wrap1 = kind == 1 && M.periodic && (p_old - p_new > 1 || p_new - p_old > 1);   // hop across the seam
            int lo = centre - Rt, len = 2 * Rt + 1 + span;
            if (wrap1 || len >= L || (!M.periodic && Rt >= L)) { lo = 0; len = L; }
            for (int k = t; k < len; k += NT) {
                int x = lo + k;
                if (M.periodic) { x %= L; if (x < 0) x += L; }
                else if (x < 0 || x >= L) continue;
                const double g0 = site_weight(M, tab, GX_TLEN, x, p_old);
                if (kind == 1) {
                    const double g1 = site_weight(M, tab, GX_TLEN, x, p_new), d = g1 - g0;      // exact on the weight grid
                    W[x] += d; S[x] += sg > 0 ? d : -d;
                } else if (kind == 2) {
                    S[x] -= sg > 0 ? 2.0 * g0 : -2.0 * g0;
                } else {
                    W[x] -= g0; S[x] -= sg > 0 ? g0 : -g0;
                }
            }
        }
        __syncthreads();
        GSTAMP(3)
        // ---- E: time and observations (ref :514-538)
        n_ev += 1;
        tnow += tau;
        if (tnow > a.p.T) break;
        while (k_obs < nobs && t_next <= tnow) { record(k_obs); ++k_obs; t_next = k_obs < nobs ? a.times[k_obs] : INFINITY; }
        GSTAMP(4)
    }
#ifdef APS_STAMPS
    if (t == 0 && sys == 0 && a.exits) for (int k = 0; k < 5; ++k) a.exits[k] = (double)st[k];   // diagnostic build only
#endif
    if constexpr (CP) gilc_flush<NT>(gilc_lds(gils_slots(lds, occp, L), a.cp, NT / 64), a.cp, (size_t)sys);
    if constexpr (RS) {                                        // the end state: a resumed launch continues this trajectory
        __syncthreads();
        for (int i = t; i < ncap; i += NT) {
            if constexpr (XR) {                                // LDS holds the system's own slots only: the others are empty
                const bool own = i < vw.nslots;
                a.rs.pos_out[(size_t)sys * ncap + i] = own ? pos[i] : 0; a.rs.flg_out[(size_t)sys * ncap + i] = own ? flg[i] : (uint8_t)0;
                a.rs.ref_out[(size_t)sys * ncap + i] = own ? ref[i] : -1;
                continue;
            }
            a.rs.pos_out[(size_t)sys * ncap + i] = pos[i]; a.rs.flg_out[(size_t)sys * ncap + i] = flg[i]; a.rs.ref_out[(size_t)sys * ncap + i] = ref[i];
        }
    }
    if (t == 0) {
        if (a.n_recorded) a.n_recorded[sys] = k_obs;
        if (a.n_events) a.n_events[sys] = n_ev;
        if (a.t_final) a.t_final[sys] = tnow;
        if (a.n_exits) a.n_exits[sys] = n_exit;
        if constexpr (MX && ST) { a.wn.n_window[sys] = n_win; a.wn.n_empty[sys] = n_emp; }
    }
}
#undef GX_TLEN
#undef GX_FIELD
#undef GX_SLOTS
#undef GX_CHUNK
#undef GX_BLOCK

// threads and dynamic LDS bytes of one system in the batch kernel; st: with the structure sums' slots, and with a copy of the
// phase table behind them where the 160 KB leave room for it (phase_in_lds); cap: with the capture slots and the bind times;
// prof_bytes: with that many bytes of profile slots
void batch_shape(int L, int ncap, int tlen, bool st, int &NT, size_t &lds, bool *phase_in_lds = nullptr, const GilcCall *cap = nullptr,
                 size_t prof_bytes = 0) {
    NT = ncap <= 1024 ? 64 : 256;                             // one wavefront per system while a lane owns at most 16 particles
    lds = ((size_t)2 * L + ((tlen + 2) & ~1) + ncap + (ncap & 1) + 8 + 5 * NT + 8) * sizeof(double) +
          ((size_t)3 * ncap + 16) * sizeof(int) + (size_t)((ncap + 15) & ~15) + (size_t)2 * ((L + 15) & ~15);
    if (st) lds = ((lds + 7) & ~(size_t)7) + gils_lds_doubles(NT) * sizeof(double);
    if (st && phase_in_lds) {
        *phase_in_lds = lds + (size_t)16 * L <= 160 * 1024;
        if (*phase_in_lds) lds += (size_t)16 * L;
    }
    if (cap) lds = ((lds + 7) & ~(size_t)7) + (gilc_lds_slots(NT, cap->n_groups, cap->c_bins, cap->h_bins) + (size_t)ncap) * 8;
    if (prof_bytes) lds = ((lds + 7) & ~(size_t)7) + prof_bytes;
}

// device copies of the outputs of one capture call (gilc_plan_info.output_bytes)
int64_t gilc_output_bytes(const gil_params *p, const GilcCall &c, bool states) {
    const int64_t S = p->n_systems, O = p->n_obs, N = p->n_cap;
    return S * ((states ? O * N * 6 : 0) + O * GIL_NSCALARS * 8 + N * 24 + 24 + O * (GILC_NFIXED + c.n_groups + c.c_bins) * 8 +
                2 * (int64_t)c.h_bins * 8 + 32);
}

// device copies of the outputs of one call (gils_plan_info.output_bytes)
int64_t gils_output_bytes(const gil_params *p, int k_max, bool states, bool scalars) {
    const int64_t S = p->n_systems, O = p->n_obs, N = p->n_cap;
    return S * ((states ? O * N * 6 : 0) + (scalars ? O * GIL_NSCALARS * 8 : 0) + N * 24 + 24 + O * (4 + 2 * (int64_t)k_max) * 8);
}

// The batch kernel of variant V with NT threads a system: the one place that names the instantiation.  Raises its LDS limit
// and launches it; the timed window holds this launch alone.
template <GilKind V, int NT>
int gil_launch_nt(OneShot &job, int S, size_t lds, const typename GilKernelArgs<V>::type &a) {
    const auto kernel = &gil_kernel<NT, V>;
    if (int rc = job.raise_lds_limit(reinterpret_cast<const void *>(kernel), lds)) return rc;
    job.ev.start();
    hipLaunchKernelGGL(kernel, dim3((unsigned)S), dim3(NT), lds, nullptr, a);
    job.ev.stop();
    return 0;
}

template <GilKind V>
int gil_launch(OneShot &job, int NT, int S, size_t lds, const typename GilKernelArgs<V>::type &a) {
    return NT == 64 ? gil_launch_nt<V, 64>(job, S, lds, a) : gil_launch_nt<V, 256>(job, S, lds, a);
}

// The one host driver of the batch kernel for the launches of one variant.  A resumable launch (ex.rs) reads no start state from
// io.  The callers have checked their required pointers.
int batch_run(const char *who, std::string &err, const gil_params *p, const GilIo &io, const GilExtras &ex) {
    auto bad = [&](const std::string &m) { err = std::string(who) + ": " + m; return GIL_ERR_ARG; };
    if (p->L < 2 || p->L > GIL_MAX_L) return bad("L must be in [2, GIL_MAX_L]");
    if (p->K < 1 || p->K > 32) return bad("site capacity K must be in [1, 32]");
    if (p->n_systems < 1 || p->n_cap < 1 || p->n_cap > GIL_MAX_N || p->n_obs < 1 || p->max_events < 0) return bad("bad n_systems / n_cap / n_obs / max_events");
    const int S = p->n_systems, L = p->L, ncap = p->n_cap;
    const GilcCall *cap = ex.cap; const GilpCall *prof = ex.prof;
    if (!ex.rs) { const std::string why = gil_check_start(p, io, "n0 outside [0, n_cap]"); if (!why.empty()) return bad(why); }
    if (const char *why = gil_check_flip_table(p)) return bad(why);
    OneShot job{who, err, true, GIL_ERR_NODEVICE, GIL_ERR_ARG, GIL_ERR_HIP};   // zero-fill: a run may record fewer observations than it has room for
    if (int rc = job.select_device(p->device)) return rc;
    if (ex.structure_obs || cap || prof) {
        const int64_t work = prof ? (int64_t)S * 4 : cap ? (cap->n_groups > 0 ? (int64_t)L * 4 : 0) : (int64_t)L * 16,
                      outb = prof ? gilp_output_bytes(p, prof->n_groups, prof->n_bins, io.states(), prof->profile_obs != nullptr)
                             : cap ? gilc_output_bytes(p, *cap, io.states())
                                 : gils_output_bytes(p, ex.k_max, io.states(), io.scalars_obs != nullptr);
        if (int rc = gil_refuse_device_bytes(job, work, outb)) return rc;
    }

    std::vector<double> table; int tlen = 0, q = 0;
    weight_table(p->sigma_grid, L, p->K, p->periodic != 0, table, tlen, q);
    GilpBatchArgs a{};
    int NT; size_t lds; bool phase_in_lds = false;
    batch_shape(L, ncap, tlen, ex.structure_obs != nullptr, NT, lds, &phase_in_lds, cap, prof ? gilp_lds_bytes(prof->n_bins, prof->want_field != 0) : 0);
    a.p = *p; a.tlen = tlen; a.chunk = (ncap + NT - 1) / NT;
    a.m = gil_model(p);
    if (int rc = gil_stage_common(job, a, p, io, table, (size_t)S * ncap, true, p->block_table, (size_t)(p->K + 1) * (p->K + 1))) return rc;
    if (lds > 160 * 1024) return bad("system does not fit the 160 KB of LDS");
    GilprBatchArgs b{};                                         // the resumable launches' arguments: a's own, the checkpoint and (gilpr_run) the profile's
    int rc = ex.structure_obs ? gil_stage_structure(job, a, p, ex.k_max, ex.first_obs, true, phase_in_lds)
             : cap            ? gil_stage_capture(job, a, p, *cap, false)
             : prof           ? gil_stage_profile(job, a, p, *prof) : 0;
    if (rc) return rc;
    if (ex.rs && (rc = gil_stage_checkpoint(job, b.rs, p, *ex.rs, true))) return rc;
    if ((rc = job.create_events())) return rc;
    static_cast<GilArgs &>(b) = a; b.pf = a.pf;
    rc = ex.structure_obs ? gil_launch<GilKind::Structure>(job, NT, S, lds, a)
         : cap            ? gil_launch<GilKind::Capture>(job, NT, S, lds, a)
         : prof && ex.rs  ? gil_launch<GilKind::ProfileResume>(job, NT, S, lds, b)
         : prof           ? gil_launch<GilKind::Profile>(job, NT, S, lds, a)
         : ex.rs          ? gil_launch<GilKind::Resume>(job, NT, S, lds, b) : gil_launch<GilKind::Plain>(job, NT, S, lds, a);
    if (rc) return rc;
    if ((rc = job.finish(hipGetLastError(), "gil_kernel", io.kernel_ms))) return rc;
    if ((rc = gil_fetch_common(job, a, p, io))) return rc;
    if (ex.structure_obs) rc = gil_fetch_structure(job, a, p, ex.structure_obs);
    else if (cap) rc = gil_fetch_capture(job, a, p, *cap);
    else if (prof) rc = gil_fetch_profile(job, a, p, *prof);
    if (!rc && ex.rs) rc = gil_fetch_checkpoint(job, *ex.rs, p, b.rs.pos_out, b.rs.ref_out, b.rs.flg_out);
    return rc ? rc : GIL_OK;
}

std::string g_gilr_err, g_gilpr_err;

// defined with the profile plans below
int gilp_decide(const char *who, const gil_params *p, const GilpCall &c, bool states, gilp_plan_info &info, std::string *err, bool byte_limit);
int gilp_slice(std::string &err, const char *who, const GilpCall &run, int32_t obs_first, int32_t n_obs, GilpCall &slice);

// gilr_run and gilrm_run: the start state is checked and laid out here, the launch is the shape's own driver.  With `prof`
// (gilpr_run of include/gillespie_profile_resume.h; its first_obs is ABSOLUTE, errors go to g_gilpr_err) the launch also takes the
// profiles of the slice and the shape is gilp_run's, whatever `large` says: the profile call's refusals, then the segment's, then
// the plan's byte limit.
int gilr_drive(bool large, const char *who, const gil_params *p, const GilIo &io, int32_t obs_first, const gil_checkpoint *from,
               gil_checkpoint *to, const GilpCall *prof = nullptr) {
    std::string &err = prof ? g_gilpr_err : g_gilr_err;
    auto bad = [&](const std::string &m) { err = std::string(who) + ": " + m; return GIL_ERR_ARG; };
    if (!p || !p->beta || !p->times_obs || (!from && (!io.n0 || !io.pos0 || !io.sigma0)) || (prof && (!prof->ensemble_sums || !prof->members)))
        return bad("null argument");
    if (p->n_systems < 1 || p->n_cap < 1 || p->n_obs < 1 || p->max_events < 0 || p->L < 2 || p->K < 1) return bad("bad n_systems / n_cap / n_obs / max_events / L / K");
    if (large && p->n_systems > GILM_MAX_SYSTEMS) return bad("n_systems must be in [1, GILM_MAX_SYSTEMS]");
    const size_t S = (size_t)p->n_systems;
    GilpCall slice{};                                          // the profiles start at row first_obs - obs_first of this slice, within [0, n_obs]
    gilp_plan_info pinfo{};
    if (prof) {
        if (int rc = gilp_slice(err, who, *prof, obs_first, p->n_obs, slice)) return rc;
        if (int rc = gilp_decide(who, p, slice, io.states(), pinfo, &err, false)) return rc;
        large = pinfo.shape == GILS_SHAPE_LARGE;
    }
    if (!from) { const std::string why = gil_check_start(p, io, "n0 outside [0, n_cap]"); if (!why.empty()) return bad(why); }
    GilrCall call;
    const std::string why = gilr_prepare(p, io.n0, io.pos0, io.sigma0, io.bound0, obs_first, from, to, call);
    if (!why.empty()) return bad(why);
    if (prof) if (int rc = gil_refuse_plan_bytes(who, err, pinfo.work_bytes, pinfo.output_bytes)) return rc;
    std::vector<int32_t> nrec(S, 0);                           // the checkpoint needs these three whether or not the caller wants them
    std::vector<int64_t> nev(S, 0);
    std::vector<double> tfin(S, 0.0);
    GilIo run = io;                                            // the launch's own record: no start state, the three outputs here
    run.n0 = run.pos0 = nullptr; run.sigma0 = nullptr; run.bound0 = nullptr;
    run.n_recorded = nrec.data(); run.n_events = nev.data(); run.t_final = tfin.data();
    GilExtras ex; ex.rs = &call;
    if (prof) ex.prof = &slice;
    if (int rc = large ? gil_large_run(who, err, p, run, ex) : batch_run(who, err, p, run, ex)) return rc;
    gilr_finish(p, call, nrec.data(), nev.data(), tfin.data());
    for (size_t s = 0; s < S; ++s) {
        if (io.n_recorded) io.n_recorded[s] = nrec[s];
        if (io.n_events) io.n_events[s] = nev[s];
        if (io.t_final) io.t_final[s] = tfin[s];
    }
    return GIL_OK;
}

// What the plans with two shapes (gils, gilc, gilp) check alike: nullptr, or the text of the complaint
const char *gil_check_plan_params(const gil_params *p) {
    if (p->L < 2) return "L must be at least 2";
    if (p->n_systems < 1 || p->n_cap < 1 || p->n_obs < 1 || p->max_events < 0) return "bad n_systems / n_cap / n_obs / max_events";
    return nullptr;
}

// The shape such a plan chooses: the batch shape where a system with its extras (batch_shape's st, cap, prof_bytes) fits the
// 160 KB of LDS, else the large shape with large_lds bytes of slots behind the kernel's own.  large_work: the large shape's
// scratch, 0 in the batch shape.  0, or GIL_ERR_ARG with the text in `err`.
struct GilShape { int32_t shape, threads, lds_bytes, phase_in_lds; int64_t large_work; };
int gil_choose_shape(const char *who, std::string &err, const gil_params *p, bool st, const GilcCall *cap, size_t prof_bytes,
                     int32_t large_lds, GilShape &sh) {
    sh = GilShape{GILS_SHAPE_LARGE, 1024, 0, 0, 0};
    if (p->L <= GIL_MAX_L && p->n_cap <= GIL_MAX_N) {
        if (p->K < 1 || p->K > 32) { err = std::string(who) + ": site capacity K must be in [1, 32]"; return GIL_ERR_ARG; }
        std::vector<double> table; int tlen = 0, q = 0, NT = 0; size_t lds = 0;
        weight_table(p->sigma_grid, p->L, p->K, p->periodic != 0, table, tlen, q);
        bool phase_in_lds = false;
        batch_shape(p->L, p->n_cap, tlen, st, NT, lds, &phase_in_lds, cap, prof_bytes);
        if (lds <= 160 * 1024) { sh = GilShape{GILS_SHAPE_BATCH, NT, (int32_t)lds, phase_in_lds ? 1 : 0, 0}; return GIL_OK; }
    }
    return gil_large_plan(who, err, p, large_lds, &sh.lds_bytes, &sh.large_work);
}

std::string g_gils_err;

// the checks gils_plan and gils_run share, and the shape: 0 with `info` filled, or GIL_ERR_ARG with the text in g_gils_err
int gils_decide(const char *who, const gil_params *p, int k_max, int first_obs, bool states, bool scalars, gils_plan_info &info) {
    auto bad = [&](const std::string &m) { g_gils_err = std::string(who) + ": " + m; return GIL_ERR_ARG; };
    if (const char *why = gil_check_plan_params(p)) return bad(why);
    if (k_max < 1 || k_max > std::min(p->L, GILS_MAX_K)) return bad("k_max must be in [1, min(L, GILS_MAX_K)]");
    if (first_obs < 0 || first_obs > p->n_obs) return bad("first_obs must be in [0, n_obs]");
    GilShape sh;
    if (int rc = gil_choose_shape(who, g_gils_err, p, true, nullptr, 0, (int32_t)(gils_lds_doubles(1024) * sizeof(double)), sh)) return rc;
    info = gils_plan_info{};
    info.row_len = 4 + 2 * k_max;
    info.output_bytes = gils_output_bytes(p, k_max, states, scalars);
    info.shape = sh.shape; info.threads = sh.threads; info.lds_bytes = sh.lds_bytes; info.phase_in_lds = sh.phase_in_lds;
    info.work_bytes = sh.large_work + (int64_t)p->L * 16;
    return gil_refuse_plan_bytes(who, g_gils_err, info.work_bytes, info.output_bytes);
}

std::string g_gilc_err;

// the checks gilc_plan and gilc_run share, and the shape: 0 with `info` filled, or GIL_ERR_ARG with the text in g_gilc_err
int gilc_decide(const char *who, const gil_params *p, const GilcCall &c, bool states, gilc_plan_info &info) {
    auto bad = [&](const std::string &m) { g_gilc_err = std::string(who) + ": " + m; return GIL_ERR_ARG; };
    if (const char *why = gil_check_plan_params(p)) return bad(why);
    if (c.n_groups < 0 || c.n_groups > GILC_MAX_GROUPS) return bad("n_groups = " + std::to_string(c.n_groups) + " is outside [0, " + std::to_string(GILC_MAX_GROUPS) + "]");
    if (c.c_bins < 2 || c.c_bins > GILC_MAX_CBINS) return bad("c_bins = " + std::to_string(c.c_bins) + " is outside [2, " + std::to_string(GILC_MAX_CBINS) + "]");
    if (c.h_bins < 1 || c.h_bins > GILC_MAX_HBINS) return bad("h_bins = " + std::to_string(c.h_bins) + " is outside [1, " + std::to_string(GILC_MAX_HBINS) + "]");
    if (!(c.h_dt > 0.0) || !std::isfinite(c.h_dt)) return bad("h_dt = " + std::to_string(c.h_dt) + " must be positive and finite");
    if (c.first_obs < 0 || c.first_obs > p->n_obs) return bad("first_obs = " + std::to_string(c.first_obs) + " is outside [0, n_obs = " + std::to_string(p->n_obs) + "]");
    if (c.group_of_site)
        for (int x = 0; x < p->L; ++x) {
            const int g = c.group_of_site[x];
            if (g < -1 || g >= c.n_groups) return bad("group id " + std::to_string(g) + " at site " + std::to_string(x) + " is outside [-1, n_groups = " + std::to_string(c.n_groups) + ")");
            if (g >= 0 && !(p->anchor_mask && p->anchor_mask[x])) return bad("site " + std::to_string(x) + " carries group " + std::to_string(g) + " but anchor_mask does not mark it");
        }
    GilShape sh;
    if (int rc = gil_choose_shape(who, g_gilc_err, p, false, &c, 0, (int32_t)(gilc_lds_slots(1024, c.n_groups, c.c_bins, c.h_bins) * 8), sh)) return rc;
    info = gilc_plan_info{};
    info.row_len = GILC_NFIXED + c.n_groups + c.c_bins;
    info.output_bytes = gilc_output_bytes(p, c, states);
    info.shape = sh.shape; info.threads = sh.threads; info.lds_bytes = sh.lds_bytes;
    info.work_bytes = (c.n_groups > 0 ? (int64_t)p->L * 4 : 0);   // the group table; large shape: the bind times too
    if (sh.shape == GILS_SHAPE_LARGE) info.work_bytes += sh.large_work + (int64_t)p->n_systems * p->n_cap * 8;
    return gil_refuse_plan_bytes(who, g_gilc_err, info.work_bytes, info.output_bytes);
}

std::string g_gilp_err;

// the checks gilp_plan and gilp_run share, and the shape: 0 with `info` filled, or GIL_ERR_ARG with the text in g_gilp_err
// what gilp_decide and gilxp_decide refuse of a profile call on its own numbers: empty, or the text of the complaint
std::string gilp_check_call(const gil_params *p, const GilpCall &c) {
    const int max_bins = std::min(p->L, GILP_MAX_BINS);
    if (c.n_bins < 1 || c.n_bins > max_bins) return "n_bins = " + std::to_string(c.n_bins) + " is outside [1, min(L, GILP_MAX_BINS) = " + std::to_string(max_bins) + "]";
    if (c.n_groups < 1 || c.n_groups > GILP_MAX_GROUPS) return "n_groups = " + std::to_string(c.n_groups) + " is outside [1, " + std::to_string(GILP_MAX_GROUPS) + "]";
    if (c.first_obs < 0 || c.first_obs > p->n_obs) return "first_obs = " + std::to_string(c.first_obs) + " is outside [0, n_obs = " + std::to_string(p->n_obs) + "]";
    if (c.want_field != 0 && c.want_field != 1) return "want_field = " + std::to_string(c.want_field) + " is neither 0 nor 1";
    if (c.want_field && (int64_t)p->L * p->n_systems >= (1ll << 31))
        return "want_field with L * n_systems = " + std::to_string((int64_t)p->L * p->n_systems) + " >= 2^31: the fixed-point field sum could overflow 64 bits";
    if (c.group_of_system)
        for (int s = 0; s < p->n_systems; ++s) {
            const int g = c.group_of_system[s];
            if (g < 0 || g >= c.n_groups) return "group id " + std::to_string(g) + " of system " + std::to_string(s) + " is outside [0, n_groups = " + std::to_string(c.n_groups) + ")";
        }
    return "";
}

// `err`: where the text goes (null: g_gilp_err); byte_limit false: the caller asks gil_refuse_plan_bytes itself, after checks of
// its own (a segment's)
int gilp_decide(const char *who, const gil_params *p, const GilpCall &c, bool states, gilp_plan_info &info, std::string *err = nullptr,
                bool byte_limit = true) {
    std::string &text = err ? *err : g_gilp_err;
    auto bad = [&](const std::string &m) { text = std::string(who) + ": " + m; return GIL_ERR_ARG; };
    if (const char *why = gil_check_plan_params(p)) return bad(why);
    { const std::string why = gilp_check_call(p, c); if (!why.empty()) return bad(why); }
    const size_t prof_lds = gilp_lds_bytes(c.n_bins, c.want_field != 0);
    GilShape sh;
    if (int rc = gil_choose_shape(who, text, p, false, nullptr, prof_lds, (int32_t)prof_lds, sh)) return rc;
    info = gilp_plan_info{};
    info.bin_width = (p->L + c.n_bins - 1) / c.n_bins;
    info.n_bins_used = (p->L + info.bin_width - 1) / info.bin_width;
    info.output_bytes = gilp_output_bytes(p, c.n_groups, c.n_bins, states, c.profile_obs != nullptr);
    info.shape = sh.shape; info.threads = sh.threads; info.lds_bytes = sh.lds_bytes;
    info.work_bytes = sh.large_work + (int64_t)p->n_systems * 4;
    return byte_limit ? gil_refuse_plan_bytes(who, text, info.work_bytes, info.output_bytes) : GIL_OK;
}

// The profile call of one segment (include/gillespie_profile_resume.h) from the run's: first_obs is absolute there and counts
// within the slice here, clamp(first_obs - obs_first, 0, n_obs).  0, or GIL_ERR_ARG with the text in `err`.
int gilp_slice(std::string &err, const char *who, const GilpCall &run, int32_t obs_first, int32_t n_obs, GilpCall &slice) {
    if (run.first_obs < 0) {
        err = std::string(who) + ": first_obs = " + std::to_string(run.first_obs) + " must not be negative: it is an index on the run's observation grid";
        return GIL_ERR_ARG;
    }
    slice = run;
    slice.first_obs = (int)std::min<int64_t>(std::max<int64_t>((int64_t)run.first_obs - obs_first, 0), std::max(n_obs, 0));
    return GIL_OK;
}

std::string g_gilx_err;

// the checks gilx_plan and gilx_run share, the tables and the shape: 0 with `info` and `tb` filled, or GIL_ERR_ARG with the
// text in g_gilx_err
int gilx_decide(const char *who, const gil_params *p, const gilx_variants *v, bool states, gilx_plan_info &info, GilxTables &tb,
                std::string &err = g_gilx_err) {
    auto bad = [&](const std::string &m) { err = std::string(who) + ": " + m; return GIL_ERR_ARG; };
    if (p->L < 2) return bad("L must be at least 2");
    if (p->L > GIL_MAX_L)
        return bad("L = " + std::to_string(p->L) + " is beyond GIL_MAX_L = " + std::to_string(GIL_MAX_L) + ": the large-system shape takes no mixed batches");
    if (p->K < 1 || p->K > 32) return bad("site capacity K must be in [1, 32]");
    if (p->n_systems < 1 || p->n_cap < 1 || p->n_obs < 1 || p->max_events < 0) return bad("bad n_systems / n_cap / n_obs / max_events");
    if (p->n_cap > GIL_MAX_N)
        return bad("n_cap = " + std::to_string(p->n_cap) + " is beyond GIL_MAX_N = " + std::to_string(GIL_MAX_N) + ": the large-system shape takes no mixed batches");
    { const std::string why = gilx_check_variants(p, v); if (!why.empty()) return bad(why); }
    gilx_build_tables(p, v, tb);                                // gillespie_mixed.hpp: shared with the large shape's gilxm_decide
    const int S = p->n_systems;
    int NT = 0; size_t lds = 0;
    batch_shape(p->L, p->n_cap, tb.max_tlen, false, NT, lds);
    if (lds > 160 * 1024)
        return bad("the launch needs " + std::to_string(lds) + " bytes of LDS per system (L = " + std::to_string(p->L) + ", n_cap = " + std::to_string(p->n_cap) +
                   ", longest table " + std::to_string(tb.max_tlen) + "), more than the " + std::to_string(160 * 1024) + " bytes (160 KB) of a workgroup");
    info = gilx_plan_info{};
    info.threads = NT; info.lds_bytes = (int32_t)lds; info.max_tlen = tb.max_tlen; info.systems_per_cu = (int32_t)((size_t)160 * 1024 / lds);
    info.table_doubles = (int64_t)tb.table.size();
    const int64_t O = p->n_obs, N = p->n_cap;
    info.output_bytes = (int64_t)S * ((states ? O * N * 6 : 0) + O * GIL_NSCALARS * 8 + N * 24 + 24);
    return GIL_OK;
}

std::string g_gilxs_err, g_gilxr_err;

// the checks gilxs_plan and gilxs_run share, the tables and the shape: 0 with `info` and `tb` filled, or GIL_ERR_ARG with the
// text in g_gilxs_err.  gilx_decide's refusals first, then gils_decide's.
int gilxs_decide(const char *who, std::string &err, const gil_params *p, const gilx_variants *v, int k_max, int first_obs, bool states,
                 bool rows, gilxs_plan_info &info, GilxTables &tb) {
    auto bad = [&](const std::string &m) { err = std::string(who) + ": " + m; return GIL_ERR_ARG; };
    gilx_plan_info xi;
    if (int rc = gilx_decide(who, p, v, states, xi, tb, err)) return rc;
    const int max_k = std::min(p->L, GILS_MAX_K);
    if (k_max < 1 || k_max > max_k) return bad("k_max = " + std::to_string(k_max) + " is outside [1, min(L, GILS_MAX_K) = " + std::to_string(max_k) + "]");
    if (first_obs < 0 || first_obs > p->n_obs) return bad("first_obs = " + std::to_string(first_obs) + " is outside [0, n_obs = " + std::to_string(p->n_obs) + "]");
    int NT = 0; size_t lds = 0; bool phase_in_lds = false;
    batch_shape(p->L, p->n_cap, tb.max_tlen, true, NT, lds, &phase_in_lds);
    if (lds > 160 * 1024)
        return bad("the launch needs " + std::to_string(lds) + " bytes of LDS per system with the structure sums (L = " + std::to_string(p->L) +
                   ", n_cap = " + std::to_string(p->n_cap) + ", longest table " + std::to_string(tb.max_tlen) + "), more than the " +
                   std::to_string(160 * 1024) + " bytes (160 KB) of a workgroup");
    info = gilxs_plan_info{};
    info.threads = NT; info.lds_bytes = (int32_t)lds; info.phase_in_lds = phase_in_lds ? 1 : 0; info.max_tlen = tb.max_tlen;
    info.systems_per_cu = (int32_t)((size_t)160 * 1024 / lds); info.row_len = 4 + 2 * k_max;
    info.work_bytes = (int64_t)p->L * 16;
    const int64_t S = p->n_systems, O = p->n_obs;
    info.output_bytes = xi.output_bytes + S * (O * 32 + (int64_t)k_max * 24 + 8) + (rows ? S * O * info.row_len * 8 : 0);
    return gil_refuse_plan_bytes(who, err, info.work_bytes, info.output_bytes);
}

std::string g_gilxp_err;

// the checks gilxp_plan and gilxp_run share, and the shape: 0 with `info` filled, or GIL_ERR_ARG with the text in g_gilxp_err.
// The mixed launch's refusals first (gilx_decide's where the batch shape takes the launch, else gilxm_decide's), then
// gilp_decide's.  The shape rule is gilp_run's with the longest table of the batch: the batch shape where gilx_run takes the
// launch and the profile slots fit the 160 KB behind it, else the large shape.
// `err`, byte_limit: as in gilp_decide.
int gilxp_decide(const char *who, const gil_params *p, const gilx_variants *v, const GilpCall &c, bool states, gilxp_plan_info &info,
                 std::string *err = nullptr, bool byte_limit = true) {
    std::string &text = err ? *err : g_gilxp_err;
    auto bad = [&](const std::string &m) { text = std::string(who) + ": " + m; return GIL_ERR_ARG; };
    gilx_plan_info xi{}; GilxTables tb;
    bool batch = p->L <= GIL_MAX_L && p->n_cap <= GIL_MAX_N && gilx_decide(who, p, v, states, xi, tb, text) == GIL_OK;
    int32_t large_lds = 0, large_tlen = 0; int64_t large_work = 0, large_doubles = 0;
    bool planned_large = false;
    auto plan_large = [&]() {                                  // the profile slots enter once the call's numbers are checked
        planned_large = true;
        return gil_large_mixed_plan(who, text, p, v, states, 0, &large_lds, &large_work, &large_tlen, &large_doubles);
    };
    if (!batch) if (int rc = plan_large()) return rc;
    { const std::string why = gilp_check_call(p, c); if (!why.empty()) return bad(why); }
    const size_t prof_lds = gilp_lds_bytes(c.n_bins, c.want_field != 0);
    int NT = 0; size_t lds = 0;
    if (batch) {
        batch_shape(p->L, p->n_cap, tb.max_tlen, false, NT, lds, nullptr, nullptr, prof_lds);
        batch = lds <= 160 * 1024;
    }
    if (!batch && !planned_large) if (int rc = plan_large()) return rc;
    info = gilxp_plan_info{};
    info.bin_width = (p->L + c.n_bins - 1) / c.n_bins;
    info.n_bins_used = (p->L + info.bin_width - 1) / info.bin_width;
    info.output_bytes = gilp_output_bytes(p, c.n_groups, c.n_bins, states, c.profile_obs != nullptr);
    info.work_bytes = (int64_t)p->n_systems * 4;
    if (batch) {
        info.shape = GILS_SHAPE_BATCH; info.threads = NT; info.lds_bytes = (int32_t)lds; info.max_tlen = tb.max_tlen;
        info.table_doubles = (int64_t)tb.table.size();
    } else {
        info.shape = GILS_SHAPE_LARGE; info.threads = 1024; info.lds_bytes = large_lds + (int32_t)prof_lds; info.max_tlen = large_tlen;
        info.table_doubles = large_doubles; info.work_bytes += large_work;
        if (info.lds_bytes > 160 * 1024)
            return bad("the launch needs " + std::to_string(info.lds_bytes) + " bytes of LDS per system with the profile slots (n_bins = " +
                       std::to_string(c.n_bins) + "), more than the " + std::to_string(160 * 1024) + " bytes (160 KB) of a workgroup");
    }
    return byte_limit ? gil_refuse_plan_bytes(who, text, info.work_bytes, info.output_bytes) : GIL_OK;
}

// gilx_run's driver, with ex.xs gilxs_run's and with ex.prof gilxp_run's (batch shape; gilxp_decide has accepted the call): the
// variant tables, the launch order, the seeds and streams and the window outputs are its own, the rest is the staging path
// batch_run takes.  With ex.rs (gilxr_run, gilxsr_run; with ex.prof as well gilxpr_run, whose first_obs counts within the slice) the launch is a segment:
// the start state, the slot counts and the window sums so far are the checkpoint's (gilxr_prepare has checked them), no start
// state is read from io, and xs->first_obs counts within the slice.
int mixed_run(const gil_params *p, const gilx_variants *v, const GilIo &io, const GilExtras &ex) {
    const GilxsCall *xs = ex.xs;
    const GilpCall *prof = ex.prof;
    GilrCall *rs = ex.rs;
    const char *who = rs ? (xs ? "gilxsr_run" : prof ? "gilxpr_run" : "gilxr_run") : xs ? "gilxs_run" : prof ? "gilxp_run" : "gilx_run";
    std::string &err = rs ? (prof ? g_gilpr_err : g_gilxr_err) : xs ? g_gilxs_err : prof ? g_gilxp_err : g_gilx_err;
    auto bad = [&](const std::string &m) { err = std::string(who) + ": " + m; return GIL_ERR_ARG; };
    gilx_plan_info info; GilxTables tb;
    gilxs_plan_info sinfo{};
    if (xs) {
        if (int rc = gilxs_decide(who, err, p, v, xs->k_max, xs->first_obs, io.states(), xs->structure_obs != nullptr, sinfo, tb)) return rc;
        info = gilx_plan_info{};
        info.threads = sinfo.threads; info.lds_bytes = sinfo.lds_bytes;
    } else if (int rc = gilx_decide(who, p, v, io.states(), info, tb, err)) return rc;
    if (prof) {                                                // the profile slots behind the launch's layout: gilxp_plan's lds_bytes
        int nt = 0; size_t with_slots = 0;
        batch_shape(p->L, p->n_cap, tb.max_tlen, false, nt, with_slots, nullptr, nullptr, gilp_lds_bytes(prof->n_bins, prof->want_field != 0));
        info.lds_bytes = (int32_t)with_slots;
    }
    const int S = p->n_systems, V = v->n_variants, NT = info.threads;
    if (!rs) { const std::string why = gil_check_start(p, io, nullptr); if (!why.empty()) return bad(why); }
    if (const char *why = gil_check_flip_table(p)) return bad(why);
    const int32_t *slots = rs ? rs->n_slots.data() : io.n0;    // every system's slot count
    std::vector<int32_t> order((size_t)S), stream((size_t)S);
    std::vector<uint64_t> seed((size_t)S);
    for (int s = 0; s < S; ++s) { order[(size_t)s] = v->order ? v->order[s] : s; stream[(size_t)s] = v->stream ? v->stream[s] : s; seed[(size_t)s] = v->seed ? v->seed[s] : p->seed; }
    if (!v->order) std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return slots[x] > slots[y]; });   // long systems first
    OneShot job{who, err, true, GIL_ERR_NODEVICE, GIL_ERR_ARG, GIL_ERR_HIP};   // zero-fill: slots beyond n0 and rows never reached stay zero
    if (int rc = job.select_device(p->device)) return rc;
    if (xs) if (int rc = gil_refuse_device_bytes(job, sinfo.work_bytes, sinfo.output_bytes)) return rc;
    if (prof) if (int rc = gil_refuse_device_bytes(job, (int64_t)S * 4, gilp_output_bytes(p, prof->n_groups, prof->n_bins, io.states(), prof->profile_obs != nullptr))) return rc;
    GilxDriverArgs a{};                                         // the driver's one struct: every mixed launch's arguments are in it
    a.p = *p; a.p.sigma_grid = 0.0; a.p.block_table = nullptr;
    a.tlen = tb.max_tlen; a.chunk = (p->n_cap + NT - 1) / NT;    // the layout's table length; the kernel takes every system's own chunk
    a.m = gil_model(p);
    const size_t lds = (size_t)info.lds_bytes, SO = (size_t)S * p->n_obs, KK = (size_t)(p->K + 1) * (p->K + 1);
    if (int rc = gil_stage_common(job, a, p, io, tb.table, (size_t)S * p->n_cap, true, v->block_table, (size_t)V * KK)) return rc;
    a.mx.has_block = v->block_table ? 1 : 0;
    UP(mx.order, order.data(), (size_t)S); UP(mx.variant_of_system, v->variant_of_system, (size_t)S); UP(mx.variants, tb.var.data(), (size_t)V);
    UP(mx.seed, seed.data(), (size_t)S); UP(mx.stream, stream.data(), (size_t)S);
    if (rs) {                                                  // io has no start state: the slot counts take n0's place
        UP(n0, slots, (size_t)S);
        if (int rc = gil_stage_checkpoint(job, a.rs, p, *rs, true)) return rc;
    }
    const bool carried = rs && xs && rs->xfrom;                // the window sums so far, instead of zeros
    if (xs) {
        if (int rc = gil_stage_structure(job, a, p, xs->k_max, xs->first_obs, xs->structure_obs != nullptr, sinfo.phase_in_lds != 0)) return rc;
        WORK(wn.head, SO * 4);
        if (carried) { UP(wn.window, rs->xfrom->window, (size_t)S * 3 * xs->k_max); UP(wn.n_window, rs->xfrom->n_window, (size_t)S); UP(wn.n_empty, rs->xfrom->n_empty, (size_t)S); }
        else { WORK(wn.window, (size_t)S * 3 * xs->k_max); WORK(wn.n_window, (size_t)S); WORK(wn.n_empty, (size_t)S); }
    }
    if (prof) if (int rc = gil_stage_profile(job, a, p, *prof)) return rc;   // sums and members are zero-filled
    if (int rc = job.create_events()) return rc;
    GilxrBatchArgs b{};                                         // gilxr_run's arguments: the mixed launch's own and the checkpoint
    static_cast<GilxBatchArgs &>(b) = a; b.rs = a.rs;
    GilxpBatchArgs d{};                                         // gilxp_run's: the mixed launch's own and the profile's
    static_cast<GilxBatchArgs &>(d) = a; d.pf = a.pf;
    GilxprBatchArgs e{};                                        // gilxpr_run's: gilxr_run's and the profile's
    static_cast<GilxrBatchArgs &>(e) = b; e.pf = a.pf;
    if (int rc = prof && rs ? gil_launch<GilKind::MixedProfileResume>(job, NT, S, lds, e) : prof ? gil_launch<GilKind::MixedProfile>(job, NT, S, lds, d) : rs ? (xs ? gil_launch<GilKind::MixedStructureResume>(job, NT, S, lds, a) : gil_launch<GilKind::MixedResume>(job, NT, S, lds, b))
                    : (xs ? gil_launch<GilKind::MixedStructure>(job, NT, S, lds, a) : gil_launch<GilKind::Mixed>(job, NT, S, lds, a))) return rc;
    if (int rc = job.finish(hipGetLastError(), "gil_kernel (mixed)", io.kernel_ms)) return rc;
    if (int rc = gil_fetch_common(job, a, p, io)) return rc;
    if (rs) if (int rc = gil_fetch_checkpoint(job, *rs, p, a.rs.pos_out, a.rs.ref_out, a.rs.flg_out)) return rc;
    if (prof) if (int rc = gil_fetch_profile(job, a, p, *prof)) return rc;
    if (xs) {
        if (int rc = gil_fetch_structure(job, a, p, xs->structure_obs)) return rc;
        if (int rc = job.download(xs->head_obs, a.wn.head, SO * 4 * 8, "head_obs")) return rc;
        if (int rc = job.download(xs->window, a.wn.window, (size_t)S * 3 * xs->k_max * 8, "window")) return rc;
        if (int rc = job.download(xs->n_window, a.wn.n_window, (size_t)S * 4, "n_window")) return rc;
        if (int rc = job.download(xs->n_empty, a.wn.n_empty, (size_t)S * 4, "n_empty")) return rc;
    }
    return GIL_OK;
}

// gilxr_run, gilxmr_run (large) and gilxsr_run (xs: k_max, the ABSOLUTE first_obs, structure_obs, head_obs; its window outputs are
// filled in here): the start state is checked and laid out here (gilxr_prepare), the launch is the shape's own mixed driver
// With `prof` (gilxpr_run of include/gillespie_profile_resume.h; its first_obs is ABSOLUTE, errors go to g_gilpr_err) the launch
// also takes the profiles of the slice and the shape is the mixed profile plan's, whatever `large` says: the mixed launch's
// refusals, then the profile call's, then the segment's, then the plan's byte limit.
int gilxr_drive(bool large, const char *who, const gil_params *p, const gilx_variants *v, const GilIo &io, const GilxsCall *xs,
                int32_t obs_first, const gilx_checkpoint *from, gilx_checkpoint *to, const GilpCall *prof = nullptr) {
    std::string &err = prof ? g_gilpr_err : g_gilxr_err;
    auto bad = [&](const std::string &m) { err = std::string(who) + ": " + m; return GIL_ERR_ARG; };
    if (!p || !v || !p->beta || !p->times_obs || !v->variant_of_system || (!from && (!io.n0 || !io.pos0 || !io.sigma0)) || (xs && !xs->head_obs) ||
        (prof && (!prof->ensemble_sums || !prof->members)))
        return bad("null argument");
    if (p->n_systems < 1 || p->n_cap < 1 || p->n_obs < 1 || p->max_events < 0 || p->L < 2 || p->K < 1) return bad("bad n_systems / n_cap / n_obs / max_events / L / K");
    const size_t S = (size_t)p->n_systems;
    if (xs && xs->first_obs < 0) return bad("first_obs = " + std::to_string(xs->first_obs) + " must not be negative: it is an index on the run's observation grid");
    GilpCall pslice{};                                         // the profiles start at row first_obs - obs_first of this slice, within [0, n_obs]
    gilxp_plan_info pinfo{};
    if (prof) {
        if (int rc = gilp_slice(err, who, *prof, obs_first, p->n_obs, pslice)) return rc;
        if (int rc = gilxp_decide(who, p, v, pslice, io.states(), pinfo, &err, false)) return rc;
        large = pinfo.shape == GILS_SHAPE_LARGE;
        for (const gilx_checkpoint *c : {from, (const gilx_checkpoint *)to})
            if (c && (c->window || c->n_window || c->n_empty))
                return bad(std::string("the checkpoint `") + (c == from ? "from" : "to") + "` has " + (c->window ? "window" : c->n_window ? "n_window" : "n_empty") +
                           " set: a profile launch carries no window sums, the three must be NULL");
    }
    if (!from) { const std::string why = gil_check_start(p, io, nullptr); if (!why.empty()) return bad(why); }
    GilrCall call;
    const std::string why = gilxr_prepare(p, xs ? xs->k_max : 0, io.n0, io.pos0, io.sigma0, io.bound0, obs_first, from, to, call);
    if (!why.empty()) return bad(why);
    if (prof) if (int rc = gil_refuse_plan_bytes(who, err, pinfo.work_bytes, pinfo.output_bytes)) return rc;
    std::vector<int32_t> nrec(S, 0);                           // the checkpoint needs these three whether or not the caller wants them
    std::vector<int64_t> nev(S, 0);
    std::vector<double> tfin(S, 0.0);
    GilIo run = io;                                            // the launch's own record: no start state, the three outputs here
    run.n0 = run.pos0 = nullptr; run.sigma0 = nullptr; run.bound0 = nullptr;
    run.n_recorded = nrec.data(); run.n_events = nev.data(); run.t_final = tfin.data();
    GilExtras ex; ex.rs = &call;
    GilxsCall slice{};                                         // the window starts at row first_obs - obs_first of this slice, within [0, n_obs]
    if (xs) {
        slice = *xs;
        slice.first_obs = (int)std::min<int64_t>(std::max<int64_t>((int64_t)xs->first_obs - obs_first, 0), p->n_obs);
        slice.window = to ? to->window : nullptr; slice.n_window = to ? to->n_window : nullptr; slice.n_empty = to ? to->n_empty : nullptr;
        ex.xs = &slice;
    }
    if (prof) ex.prof = &pslice;
    if (large) ex.mx = v;
    if (int rc = large ? gil_large_run(who, err, p, run, ex) : mixed_run(p, v, run, ex)) return rc;
    gilxr_finish(p, call, nrec.data(), nev.data(), tfin.data());
    for (size_t s = 0; s < S; ++s) {
        if (io.n_recorded) io.n_recorded[s] = nrec[s];
        if (io.n_events) io.n_events[s] = nev[s];
        if (io.t_final) io.t_final[s] = tfin[s];
    }
    return GIL_OK;
}

}  // namespace

extern "C" {

const char *gilxr_last_error(void) { return g_gilxr_err.c_str(); }

int gilxr_run(const gil_params *p, const gilx_variants *v, const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0,
              const double *uniforms, int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs,
              int32_t *n_recorded, int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, double *kernel_ms,
              int32_t obs_first, const gilx_checkpoint *from, gilx_checkpoint *to) {
    const GilIo io{n0, pos0, sigma0, bound0, uniforms, pos_obs, sigma_obs, flags_obs, scalars_obs, n_recorded, n_events, t_final, exits, n_exits, kernel_ms};
    return gilxr_drive(false, "gilxr_run", p, v, io, nullptr, obs_first, from, to);
}

int gilxmr_run(const gil_params *p, const gilx_variants *v, const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0,
               const double *uniforms, int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs,
               int32_t *n_recorded, int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, double *kernel_ms,
               int32_t obs_first, const gilx_checkpoint *from, gilx_checkpoint *to) {
    const GilIo io{n0, pos0, sigma0, bound0, uniforms, pos_obs, sigma_obs, flags_obs, scalars_obs, n_recorded, n_events, t_final, exits, n_exits, kernel_ms};
    return gilxr_drive(true, "gilxmr_run", p, v, io, nullptr, obs_first, from, to);
}

int gilxsr_run(const gil_params *p, const gilx_variants *v, int32_t k_max, int32_t first_obs,
               const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0, const double *uniforms,
               int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs, int32_t *n_recorded,
               int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, double *structure_obs, double *head_obs,
               double *kernel_ms, int32_t obs_first, const gilx_checkpoint *from, gilx_checkpoint *to) {
    const GilIo io{n0, pos0, sigma0, bound0, uniforms, pos_obs, sigma_obs, flags_obs, scalars_obs, n_recorded, n_events, t_final, exits, n_exits, kernel_ms};
    const GilxsCall xs{k_max, first_obs, structure_obs, head_obs, nullptr, nullptr, nullptr};
    return gilxr_drive(false, "gilxsr_run", p, v, io, &xs, obs_first, from, to);
}

const char *gilx_last_error(void) { return g_gilx_err.c_str(); }

int gilx_plan(const gil_params *p, const gilx_variants *v, int32_t want_states, gilx_plan_info *out) {
    if (!p || !v || !out) { g_gilx_err = "gilx_plan: null argument"; return GIL_ERR_ARG; }
    gilx_plan_info info; GilxTables tb;
    if (int rc = gilx_decide("gilx_plan", p, v, want_states != 0, info, tb)) return rc;
    *out = info;
    return GIL_OK;
}

int gilx_run(const gil_params *p, const gilx_variants *v, const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0,
             const double *uniforms, int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs,
             int32_t *n_recorded, int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, double *kernel_ms) {
    if (!p || !v || !n0 || !pos0 || !sigma0 || !p->beta || !p->times_obs || !v->variant_of_system) { g_gilx_err = "gilx_run: null argument"; return GIL_ERR_ARG; }
    const GilIo io{n0, pos0, sigma0, bound0, uniforms, pos_obs, sigma_obs, flags_obs, scalars_obs, n_recorded, n_events, t_final, exits, n_exits, kernel_ms};
    return mixed_run(p, v, io, GilExtras{});
}

const char *gilxs_last_error(void) { return g_gilxs_err.c_str(); }

int gilxs_plan(const gil_params *p, const gilx_variants *v, int32_t k_max, int32_t first_obs, int32_t want_states, int32_t want_rows,
               gilxs_plan_info *out) {
    if (!p || !v || !out) { g_gilxs_err = "gilxs_plan: null argument"; return GIL_ERR_ARG; }
    gilxs_plan_info info; GilxTables tb;
    if (int rc = gilxs_decide("gilxs_plan", g_gilxs_err, p, v, k_max, first_obs, want_states != 0, want_rows != 0, info, tb)) return rc;
    *out = info;
    return GIL_OK;
}

int gilxs_run(const gil_params *p, const gilx_variants *v, int32_t k_max, int32_t first_obs,
              const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0, const double *uniforms,
              int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs, int32_t *n_recorded,
              int64_t *n_events, double *t_final, double *exits, int32_t *n_exits,
              double *structure_obs, double *head_obs, double *window, int32_t *n_window, int32_t *n_empty, double *kernel_ms) {
    if (!p || !v || !n0 || !pos0 || !sigma0 || !p->beta || !p->times_obs || !v->variant_of_system || !head_obs || !window || !n_window || !n_empty) {
        g_gilxs_err = "gilxs_run: null argument"; return GIL_ERR_ARG;
    }
    const GilIo io{n0, pos0, sigma0, bound0, uniforms, pos_obs, sigma_obs, flags_obs, scalars_obs, n_recorded, n_events, t_final, exits, n_exits, kernel_ms};
    const GilxsCall xs{k_max, first_obs, structure_obs, head_obs, window, n_window, n_empty};
    GilExtras ex; ex.xs = &xs;
    return mixed_run(p, v, io, ex);
}

const char *gilxp_last_error(void) { return g_gilxp_err.c_str(); }

int gilxp_plan(const gil_params *p, const gilx_variants *v, int32_t n_bins, int32_t n_groups, int32_t first_obs, int32_t want_field,
               int32_t want_states, int32_t want_per_system, gilxp_plan_info *out) {
    if (!p || !v || !out) { g_gilxp_err = "gilxp_plan: null argument"; return GIL_ERR_ARG; }
    int32_t some = 0;                                          // a plan has no buffers: only whether the per-system rows are wanted
    const GilpCall c{nullptr, n_groups, n_bins, first_obs, want_field, nullptr, nullptr, want_per_system ? &some : nullptr};
    gilxp_plan_info info;
    if (int rc = gilxp_decide("gilxp_plan", p, v, c, want_states != 0, info)) return rc;
    *out = info;
    return GIL_OK;
}

int gilxp_run(const gil_params *p, const gilx_variants *v, int32_t n_bins, int32_t first_obs, int32_t want_field,
              const int32_t *group_of_system, int32_t n_groups,
              const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0, const double *uniforms,
              int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs, int32_t *n_recorded,
              int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, int64_t *ensemble_sums, int32_t *members,
              int32_t *profile_obs, double *kernel_ms) {
    if (!p || !v || !n0 || !pos0 || !sigma0 || !p->beta || !p->times_obs || !v->variant_of_system || !ensemble_sums || !members) {
        g_gilxp_err = "gilxp_run: null argument"; return GIL_ERR_ARG;
    }
    const GilIo io{n0, pos0, sigma0, bound0, uniforms, pos_obs, sigma_obs, flags_obs, scalars_obs, n_recorded, n_events, t_final, exits, n_exits, kernel_ms};
    const GilpCall c{group_of_system, n_groups, n_bins, first_obs, want_field, ensemble_sums, members, profile_obs};
    gilxp_plan_info info;
    if (int rc = gilxp_decide("gilxp_run", p, v, c, io.states(), info)) return rc;
    GilExtras ex; ex.prof = &c;
    if (info.shape == GILS_SHAPE_BATCH) return mixed_run(p, v, io, ex);
    ex.mx = v;
    return gil_large_run("gilxp_run", g_gilxp_err, p, io, ex);
}

const char *gilp_last_error(void) { return g_gilp_err.c_str(); }

int gilp_plan(const gil_params *p, int32_t n_bins, int32_t n_groups, int32_t first_obs, int32_t want_field, int32_t want_states,
              int32_t want_per_system, gilp_plan_info *out) {
    if (!p || !out) { g_gilp_err = "gilp_plan: null argument"; return GIL_ERR_ARG; }
    int32_t some = 0;                                          // a plan has no buffers: only whether the per-system rows are wanted
    const GilpCall c{nullptr, n_groups, n_bins, first_obs, want_field, nullptr, nullptr, want_per_system ? &some : nullptr};
    gilp_plan_info info;
    if (int rc = gilp_decide("gilp_plan", p, c, want_states != 0, info)) return rc;
    *out = info;
    return GIL_OK;
}

int gilp_run(const gil_params *p, int32_t n_bins, int32_t first_obs, int32_t want_field, const int32_t *group_of_system, int32_t n_groups,
             const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0, const double *uniforms,
             int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs, int32_t *n_recorded,
             int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, int64_t *ensemble_sums, int32_t *members,
             int32_t *profile_obs, double *kernel_ms) {
    if (!p || !n0 || !pos0 || !sigma0 || !p->beta || !p->times_obs || !ensemble_sums || !members) { g_gilp_err = "gilp_run: null argument"; return GIL_ERR_ARG; }
    const GilIo io{n0, pos0, sigma0, bound0, uniforms, pos_obs, sigma_obs, flags_obs, scalars_obs, n_recorded, n_events, t_final, exits, n_exits, kernel_ms};
    const GilpCall c{group_of_system, n_groups, n_bins, first_obs, want_field, ensemble_sums, members, profile_obs};
    gilp_plan_info info;
    if (int rc = gilp_decide("gilp_run", p, c, io.states(), info)) return rc;
    GilExtras ex; ex.prof = &c;
    return info.shape == GILS_SHAPE_BATCH ? batch_run("gilp_run", g_gilp_err, p, io, ex) : gil_large_run("gilp_run", g_gilp_err, p, io, ex);
}

const char *gilpr_last_error(void) { return g_gilpr_err.c_str(); }

int gilpr_run(const gil_params *p, int32_t n_bins, int32_t first_obs, int32_t want_field, const int32_t *group_of_system, int32_t n_groups,
              const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0, const double *uniforms,
              int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs, int32_t *n_recorded,
              int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, int64_t *ensemble_sums, int32_t *members,
              int32_t *profile_obs, double *kernel_ms, int32_t obs_first, const gil_checkpoint *from, gil_checkpoint *to) {
    const GilIo io{n0, pos0, sigma0, bound0, uniforms, pos_obs, sigma_obs, flags_obs, scalars_obs, n_recorded, n_events, t_final, exits, n_exits, kernel_ms};
    const GilpCall c{group_of_system, n_groups, n_bins, first_obs, want_field, ensemble_sums, members, profile_obs};
    return gilr_drive(false, "gilpr_run", p, io, obs_first, from, to, &c);
}

int gilxpr_run(const gil_params *p, const gilx_variants *v, int32_t n_bins, int32_t first_obs, int32_t want_field,
               const int32_t *group_of_system, int32_t n_groups,
               const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0, const double *uniforms,
               int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs, int32_t *n_recorded,
               int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, int64_t *ensemble_sums, int32_t *members,
               int32_t *profile_obs, double *kernel_ms, int32_t obs_first, const gilx_checkpoint *from, gilx_checkpoint *to) {
    const GilIo io{n0, pos0, sigma0, bound0, uniforms, pos_obs, sigma_obs, flags_obs, scalars_obs, n_recorded, n_events, t_final, exits, n_exits, kernel_ms};
    const GilpCall c{group_of_system, n_groups, n_bins, first_obs, want_field, ensemble_sums, members, profile_obs};
    return gilxr_drive(false, "gilxpr_run", p, v, io, nullptr, obs_first, from, to, &c);
}

const char *gilc_last_error(void) { return g_gilc_err.c_str(); }

int gilc_plan(const gil_params *p, int32_t n_groups, int32_t c_bins, int32_t h_bins, int32_t first_obs, int32_t want_states, gilc_plan_info *out) {
    if (!p || !out) { g_gilc_err = "gilc_plan: null argument"; return GIL_ERR_ARG; }
    const GilcCall c{nullptr, n_groups, c_bins, h_bins, first_obs, 1.0, nullptr, nullptr, nullptr};
    gilc_plan_info info;
    if (int rc = gilc_decide("gilc_plan", p, c, want_states != 0, info)) return rc;
    *out = info;
    return GIL_OK;
}

int gilc_run(const gil_params *p, const int32_t *group_of_site, int32_t n_groups, int32_t c_bins, int32_t h_bins, double h_dt, int32_t first_obs,
             const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0, const double *uniforms,
             int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs, int32_t *n_recorded,
             int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, int64_t *capture_obs, int64_t *life_hist,
             double *life_sums, double *kernel_ms) {
    if (!p || !n0 || !pos0 || !sigma0 || !p->beta || !p->times_obs || !capture_obs || !life_hist || !life_sums) { g_gilc_err = "gilc_run: null argument"; return GIL_ERR_ARG; }
    const GilIo io{n0, pos0, sigma0, bound0, uniforms, pos_obs, sigma_obs, flags_obs, scalars_obs, n_recorded, n_events, t_final, exits, n_exits, kernel_ms};
    const GilcCall c{group_of_site, n_groups, c_bins, h_bins, first_obs, h_dt, capture_obs, life_hist, life_sums};
    gilc_plan_info info;
    if (int rc = gilc_decide("gilc_run", p, c, io.states(), info)) return rc;
    GilExtras ex; ex.cap = &c;
    return info.shape == GILS_SHAPE_BATCH ? batch_run("gilc_run", g_gilc_err, p, io, ex) : gil_large_run("gilc_run", g_gilc_err, p, io, ex);
}

const char *gil_last_error(void) { return g_gil_err.c_str(); }

int gil_run_batch(const gil_params *p, const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0,
                  const double *uniforms, int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs,
                  int32_t *n_recorded, int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, double *kernel_ms) {
    if (!p || !n0 || !pos0 || !sigma0 || !p->beta || !p->times_obs) { g_gil_err = "gil_run_batch: null argument"; return GIL_ERR_ARG; }
    const GilIo io{n0, pos0, sigma0, bound0, uniforms, pos_obs, sigma_obs, flags_obs, scalars_obs, n_recorded, n_events, t_final, exits, n_exits, kernel_ms};
    return batch_run("gil_run_batch", g_gil_err, p, io, GilExtras{});
}

const char *gilr_last_error(void) { return g_gilr_err.c_str(); }

int gilr_run(const gil_params *p, const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0,
             const double *uniforms, int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs,
             int32_t *n_recorded, int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, double *kernel_ms,
             int32_t obs_first, const gil_checkpoint *from, gil_checkpoint *to) {
    const GilIo io{n0, pos0, sigma0, bound0, uniforms, pos_obs, sigma_obs, flags_obs, scalars_obs, n_recorded, n_events, t_final, exits, n_exits, kernel_ms};
    return gilr_drive(false, "gilr_run", p, io, obs_first, from, to);
}

int gilrm_run(const gil_params *p, const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0,
              const double *uniforms, int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs,
              int32_t *n_recorded, int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, double *kernel_ms,
              int32_t obs_first, const gil_checkpoint *from, gil_checkpoint *to) {
    const GilIo io{n0, pos0, sigma0, bound0, uniforms, pos_obs, sigma_obs, flags_obs, scalars_obs, n_recorded, n_events, t_final, exits, n_exits, kernel_ms};
    return gilr_drive(true, "gilrm_run", p, io, obs_first, from, to);
}

const char *gils_last_error(void) { return g_gils_err.c_str(); }

int gils_plan(const gil_params *p, int32_t k_max, int32_t first_obs, int32_t want_states, gils_plan_info *out) {
    if (!p || !out) { g_gils_err = "gils_plan: null argument"; return GIL_ERR_ARG; }
    gils_plan_info info;
    if (int rc = gils_decide("gils_plan", p, k_max, first_obs, want_states != 0, true, info)) return rc;
    *out = info;
    return GIL_OK;
}

int gils_run(const gil_params *p, int32_t k_max, int32_t first_obs,
             const int32_t *n0, const int32_t *pos0, const int8_t *sigma0, const uint8_t *bound0, const double *uniforms,
             int32_t *pos_obs, int8_t *sigma_obs, uint8_t *flags_obs, int64_t *scalars_obs, int32_t *n_recorded,
             int64_t *n_events, double *t_final, double *exits, int32_t *n_exits, double *structure_obs, double *kernel_ms) {
    if (!p || !n0 || !pos0 || !sigma0 || !p->beta || !p->times_obs || !structure_obs) { g_gils_err = "gils_run: null argument"; return GIL_ERR_ARG; }
    const GilIo io{n0, pos0, sigma0, bound0, uniforms, pos_obs, sigma_obs, flags_obs, scalars_obs, n_recorded, n_events, t_final, exits, n_exits, kernel_ms};
    gils_plan_info info;
    if (int rc = gils_decide("gils_run", p, k_max, first_obs, io.states(), scalars_obs != nullptr, info)) return rc;
    GilExtras ex; ex.k_max = k_max; ex.first_obs = first_obs; ex.structure_obs = structure_obs;
    return info.shape == GILS_SHAPE_BATCH ? batch_run("gils_run", g_gils_err, p, io, ex) : gil_large_run("gils_run", g_gils_err, p, io, ex);
}

}  // extern "C"
