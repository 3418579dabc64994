// gillespie_structure.hpp -- device side of include/gillespie_structure.h: the structure observables of
// PARTICLE_solver_BIOLOGY_local_structure.py:55-103 reduced inside the exact event loop, at an observation, from what the
// loop holds anyway (positions, flags, site occupancy, the smoothed histograms W and S).  One function, called by the
// structure instantiations of both loop kernels (gillespie_hip.hip: the system in LDS, 64 or 256 threads;
// gillespie_big_hip.hip: the state in global memory, 1024 threads).  It writes one row of 4 + 2 k_max doubles, laid out as
// aps_observe_structure lays out its `out`:
//   [0] live particles  [1] sum_x occ[x]^2  [2] sum_x m(x)  [3] sum_x m(x)^2  [4 + 2k, 5 + 2k] sum_live exp(-2 pi i k pos / L)
// Fourier sums: the phase index r = (k pos) mod L is an integer (exact argument reduction, as structure_dft of aps_hip.hip);
// the L values (cos, sin)(-2 pi r / L) are tabulated once per launch (gils_phase_table) and gathered by r -- from a copy in
// LDS where a system in LDS leaves room for it (a lone wavefront gathering from L2 waits out every load); only the modes
// k <= L / 2 are summed, the others are their conjugates (z[L - k] = conj z[k], the summand being real); a thread owns
// modes and walks the particle slots, so no sum crosses lanes unless there are fewer modes than threads, when the slots are
// split over the spare wavefronts and the partial sums meet in LDS.  No atomics; one thread stores a value.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace {

constexpr int GILS_ALIVE = 4;                  // F_ALIVE of the loop kernels' flag byte

struct GilsArgs {                              // what a structure instantiation gets on top of the loop's own arguments
    double *rows;                              // [n_systems][n_obs][4 + 2 k_max], zero-filled: rows nobody writes stay zero
    const double *phase;                       // [L][2] cos, sin of -2 pi r / L
    int k_max, first_obs;
    int phase_in_lds;                          // systems in LDS: every workgroup keeps a copy of the table behind its sums' slots
};

// doubles of LDS gils_record_row needs: four sums per wavefront, and (more than one wavefront) two partial sums per thread
constexpr size_t gils_lds_doubles(int nt) { return (size_t)4 * (nt / 64) + (nt > 64 ? (size_t)2 * nt : 0); }

__global__ __launch_bounds__(256) void gils_phase_table(double *phase, int L) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= L) return;
    double sn, cs;
    sincospi(-2.0 * ((double)r / (double)L), &sn, &cs);
    phase[2 * r] = cs; phase[2 * r + 1] = sn;
}

// (k p) mod L for 0 <= k < 4096, 0 <= p < L <= 2^25: the quotient from a binary64 product (off by one at most), the
// remainder in integers.  Systems in LDS have L <= 4096, so their product fits 32 bits.
template <bool WIDE>
__device__ __forceinline__ int gils_phase_index(int k, int p, int L, double inv_L) {
    if (WIDE) {
        const long long kp = (long long)k * p;
        long long r = kp - (long long)((double)kp * inv_L) * L;
        r = r < 0 ? r + L : r;
        return (int)(r >= L ? r - L : r);
    }
    const int kp = k * p;
    int r = kp - (int)((double)kp * inv_L) * L;
    r = r < 0 ? r + L : r;
    return r >= L ? r - L : r;
}

// The default of gils_record_row's last argument: the sums go to the row and nowhere else.
struct GilsNoSink { static constexpr bool active = false; };

// Every thread of the workgroup calls it (it holds barriers).  occ: particles per site; W, S: the smoothed histograms
// (field_mode) or unused, when every site carries m_global; red: gils_lds_doubles(NT) doubles of LDS; step: ncap ints
// of scratch (the loop's work list, which every event rebuilds from nothing).
// sink: a second destination for the sums (gillespie_window.hpp); with an active sink `row` may be null (no row is stored) and
// k_max may be 0 (the four site sums only).  Without one, the callers' code is what it was before the argument existed.
template <int NT, typename Occ, class Sink = GilsNoSink>
__device__ inline void gils_record_row(double *row, int k_max, int L, int ncap, const int *pos, const uint8_t *flg, const Occ *occ,
                                       const double *W, const double *S, bool field_mode, double m_global, const double *phase,
                                       double *red, int *step, const Sink &sink = Sink{}) {
    constexpr int NW = NT / 64;
    const int t = threadIdx.x;
    // ---- the four sums over sites: m(x) = clip(S / W) where W > 0, the expression of the rate evaluation
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int x = t; x < L; x += NT) {
        const double c = (double)occ[x];
        double m = m_global;
        if (field_mode) {
            const double w = W[x];
            m = 0.0;
            if (w > 0.0) { m = S[x] / w; m = m > 1.0 ? 1.0 : (m < -1.0 ? -1.0 : m); }
        }
        v[0] += c; v[1] += c * c; v[2] += m; v[3] += m * m;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_xor(v[q], off);
    __syncthreads();
    if ((t & 63) == 0)
#pragma unroll
        for (int q = 0; q < 4; ++q) red[4 * (t >> 6) + q] = v[q];
    __syncthreads();
    if (t < 4) {
        double s = red[t];
#pragma unroll
        for (int w = 1; w < NW; ++w) s += red[4 * w + t];
        if constexpr (!Sink::active) row[t] = s;
        else { if (row) row[t] = s; sink.site_sum(t, s); }
    }
    double n_live = 0.0;                                       // an active sink divides by it: entry 0, summed in the same order
    if constexpr (Sink::active) {
        n_live = red[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) n_live += red[4 * w];
    }
    // ---- Fourier sums: thread = (mode within a pass, slice of the particle slots).  A thread keeps the sums of PT modes,
    // kw apart, in registers while it walks the slots: the phase index of the first comes from one product per slot, the
    // others follow by adding step[i] = (kw pos[i]) mod L -- an add and a conditional subtract instead of a product each.
    const int kk = min(k_max, L / 2 + 1);                      // modes summed; the rest are conjugates
    int kw = 64;                                               // modes per pass: a power of two, whole wavefronts
    while (kw < NT && kw < kk) kw <<= 1;
    const int G = NT / kw, kl = t & (kw - 1), g = t / kw;      // G slices of the slots; g is uniform over a wavefront
    double *part = red + 4 * NW;                               // [NT][2], NT > 64 only
    const double inv_L = 1.0 / (double)L;
    constexpr bool WIDE = NT > 256;
    constexpr int PT = WIDE ? 2 : 8;
    for (int i = t; i < ncap; i += NT) step[i] = gils_phase_index<WIDE>(kw, pos[i], L, inv_L);
    __syncthreads();
    for (int k0 = 0; k0 < kk; k0 += PT * kw) {
        const int kb = k0 + kl, npass = min(PT, (kk - k0 + kw - 1) / kw);   // kb < kk + kw <= 4096
        double re[PT], im[PT];
#pragma unroll
        for (int q = 0; q < PT; ++q) { re[q] = 0.0; im[q] = 0.0; }
        for (int i = g; i < ncap; i += G) {
            if (!(flg[i] & GILS_ALIVE)) continue;              // the whole wavefront skips an empty or departed slot
            int r = gils_phase_index<WIDE>(kb, pos[i], L, inv_L);
            const int d = step[i];
#pragma unroll
            for (int q = 0; q < PT; ++q)
                if (q < npass) {
#ifdef GILS_DIRECT_PHASE                                      // measurement build: no table, one sincospi per term
                    double sn, cs;
                    sincospi(-2.0 * ((double)r / (double)L), &sn, &cs);
#else
                    const double cs = phase[2 * r], sn = phase[2 * r + 1];
#endif
                    re[q] += cs; im[q] += sn;
                    r += d; r = r >= L ? r - L : r;
                }
        }
        if (NT > 64 && G > 1) {                                // uniform over the workgroup; kw >= kk, so one pass
            __syncthreads();
            part[2 * t] = re[0]; part[2 * t + 1] = im[0];
            __syncthreads();
            if (g == 0)
                for (int q = 1; q < G; ++q) { re[0] += part[2 * (q * kw + kl)]; im[0] += part[2 * (q * kw + kl) + 1]; }
        }
#pragma unroll
        for (int q = 0; q < PT; ++q) {
            const int k = kb + q * kw;
            if (g == 0 && k < kk) {
                if constexpr (!Sink::active) {
                    row[4 + 2 * k] = re[q]; row[5 + 2 * k] = im[q];
                    const int kc = L - k;                      // kc >= kk unless kc == k: no other thread writes it
                    if (k > 0 && kc != k && kc < k_max) { row[4 + 2 * kc] = re[q]; row[5 + 2 * kc] = -im[q]; }
                } else {                                       // the same stores where there is a row, and the sink's
                    const int kc = L - k;
                    const bool conj = k > 0 && kc != k && kc < k_max;
                    if (row) {
                        row[4 + 2 * k] = re[q]; row[5 + 2 * k] = im[q];
                        if (conj) { row[4 + 2 * kc] = re[q]; row[5 + 2 * kc] = -im[q]; }
                    }
                    sink.mode(k, re[q], im[q], n_live);
                    if (conj) sink.mode(kc, re[q], im[q], n_live);
                }
            }
        }
    }
    __syncthreads();
}

}  // namespace
