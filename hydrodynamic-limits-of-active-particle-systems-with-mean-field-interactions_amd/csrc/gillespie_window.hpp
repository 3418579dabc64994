// gillespie_window.hpp -- device side of include/gillespie_mixed_structure.h: the WINDOW reduction of the structure sums.  Of
// every row gils_record_row forms, the host keeps the time mean and the spread of each Fourier amplitude over the window of
// observations; here the thread that owns a mode adds the amplitude to three accumulators in global memory as soon as it has
// the mode's sums, so that nothing of size observations x modes has to leave the device:
//   window[s][k][0] = a0_k        the amplitude a_k = sqrt(re^2 + im^2) / n at the first observation the window took
//   window[s][k][1] = sum_t d_k   d_k(t) = a_k(t) - a0_k
//   window[s][k][2] = sum_t d_k^2
// Shifted by a0: the mean a0 + sum d / M and the spread (sum d^2 - (sum d)^2 / M) / (M - 1) do not subtract two numbers of the
// size of M a^2, and a mode that never changes (mode 0, n / n dx) has d = 0 and spread 0 exactly.  gils_record_row gives every
// mode k <= L / 2 to one thread, which also holds the conjugate L - k: that thread does the read-modify-write of both, in
// observation order.  No atomics.  Included by gillespie_hip.hip only, instantiated by the mixed structure kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace {

struct GilwArgs {                              // what a window instantiation gets on top of the structure arguments
    double *head;                              // [n_systems][n_obs][4] n, sum occ^2, sum m, sum m^2 of every recorded observation
    double *window;                            // [n_systems][k_max][3], zero-filled
    int32_t *n_window, *n_empty;               // [n_systems] observations accumulated; observations of the window without a live particle
};

// the sink of one observation of one system (gils_record_row's last argument)
struct GilwSink {
    static constexpr bool active = true;
    double *head;                              // the observation's four site sums
    double *acc;                               // the system's accumulators; used only when the call sums modes
    int first;                                 // the window has taken no observation yet

    __device__ __forceinline__ void site_sum(int q, double s) const { head[q] = s; }
    // mode k of an observation with n live particles; the caller stores to k from one thread only
    __device__ __forceinline__ void mode(int k, double re, double im, double n) const {
        if (!(n > 0.0)) return;                // an empty observation adds nothing (counted in n_empty)
        const double a = sqrt(re * re + im * im) / n;
        double *w = acc + 3 * (size_t)k;
        if (first) { w[0] = a; return; }       // d = 0: the sums stay what they are
        const double d = a - w[0];
        w[1] += d; w[2] += d * d;
    }
};

// the live count of the observation gils_record_row<NT> has just reduced: the sum it stored as entry 0, in its order
template <int NT>
__device__ __forceinline__ double gilw_live(const double *red) {
    double s = red[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) s += red[4 * w];
    return s;
}

}  // namespace
