// pde_sweep_fft.hpp -- the Gaussian-kernel magnetisation of the one-workgroup shape by the convolution theorem, entirely in
// the workgroup's LDS inside the persistent step loop (included by pde_hip.hip; C ABI: include/pde_sweep.h).
//
// Hot path replaced: the direct circular sum of pde_kernel (kernel_mode 1), O(L * reach) per step; the reference multiplies rffts
// (IMEX_PDE_solver_class.py:164-165).  As in pde_spectral.hpp ONE complex transform carries both signals: z = s + i tot
// (s = rho_plus - rho_minus, tot = rho_plus + rho_minus), the taps are real, the real part of the result is num, the imaginary
// part den.  Window: z[(i - kt) mod L] for i < L + 2 kt, zero up to M = 2^m; taps placed circularly, h[j mod M] = ktab[|j|];
// outputs kt .. kt + L - 1 are kept, mf[i] = Re / (Im + 1e-12).  One block: the whole ring is one window (M >= L + 2 kt).
//
// Transform: M = 2^m words (double2), PDEK_MIN_LOG2 <= m <= PDEK_MAX_LOG2, m read per system at run time.  Register passes of
// three or two levels per LDS round trip (m = 3 a + 2 b: 8 = 3+3+2, 9 = 3+3+3, 10 = 3+3+2+2, 11 = 3+3+3+2): a thread holds the
// 2^B words  base + (tt << q)  of a pass whose lowest pair distance is 2^q.  Decimation in frequency going forward (natural order
// in, slot r holds frequency brev(r)), decimation in time coming back (slot order in, natural order out): nothing is un-permuted,
// the spectrum of the taps is kept in slot order, the product is slot by slot.  The first forward pass reads the window straight
// from the state, the last inverse pass writes mf; the last forward pass, the product and the first inverse pass touch the same
// words of the same thread and are one pass.  Round trips per convolution: 2 P - 1 for P passes (7 at m = 11, 5 at m = 8 and 9),
// one barrier each.  Work items beyond M / 2^B idle through a pass; every barrier is reached by all threads.
// Twiddles: w_M^e = exp(-2 pi i e / M), e < M / 2, from a host table built entry by entry (cosl / sinl), copied to LDS once.
// LDS: word i of the buffer sits at i + (i >> 4) (one word of padding in sixteen): the 16 consecutive 16-byte accesses of a
// quarter wave fall on distinct bank groups in the passes with q >= 4 and q = 0; the pass with q = 2 (m = 11) or q = 2, 3 (m = 10, 8)
// meets two-way conflicts.  binary64 throughout, fma() explicit, no atomics, a fixed order of every operation.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <vector>

#include "pde_sweep.h"

namespace pdek {

constexpr int THREADS = 256;          // the workgroup of pde_kernel (NT of pde_common.hpp; pde_hip.hip asserts that they agree)

// ---- host
inline int log2_for(long long words) { int m = PDEK_MIN_LOG2; while ((1ll << m) < words) ++m; return m; }
inline size_t padded_words(int m) { return ((size_t)1 << m) + ((size_t)1 << (m - 4)); }
// LDS of the transform for a largest m: buffer, twiddles, spectrum
inline size_t lds_bytes(int m) { return m ? padded_words(m) * sizeof(double2) + ((size_t)1 << (m - 1)) * sizeof(double2) + ((size_t)1 << m) * sizeof(double) : 0; }
// the tables of m = PDEK_MIN_LOG2 .. m_max lie one after another: where the table of m begins (host layout, device lookup)
__host__ __device__ inline int twiddle_offset(int m) { return (1 << (m - 1)) - (1 << (PDEK_MIN_LOG2 - 1)); }
inline void build_twiddles(int m_max, std::vector<double2> &tw) {
    tw.clear();
    for (int m = PDEK_MIN_LOG2; m <= m_max; ++m) {
        const long long M = 1ll << m;
        for (long long e = 0; e < M / 2; ++e) {
            const long double ang = -6.283185307179586476925286766559L * (long double)e / (long double)M;
            tw.push_back(make_double2((double)cosl(ang), (double)sinl(ang)));
        }
    }
}

// ---- device
struct Ctx {
    double2 *buf;              // [M + M / 16] the window, transformed in place
    double2 *tw;               // [M / 2] twiddles of this system's M
    double *spec;              // [M] spectrum of the taps in slot order, times 1 / M
    const double *rp, *rm;     // the state
    double *mf;                // the magnetisation
    int m, L, kt, t;
};

__device__ __forceinline__ int pad(const int i) { return i + (i >> 4); }
__device__ __forceinline__ double2 mul(const double2 a, const double2 w) {            // a w
    return make_double2(fma(a.x, w.x, -(a.y * w.y)), fma(a.x, w.y, a.y * w.x));
}
__device__ __forceinline__ double2 mulc(const double2 a, const double2 w) {           // a conj(w)
    return make_double2(fma(a.x, w.x, a.y * w.y), fma(a.y, w.x, -(a.x * w.y)));
}

// B butterfly levels s0 .. s0 + B - 1 on the 2^B words of one work item, word tt at index base + (tt << q), lo = base mod 2^q.
// Level l pairs words h = M >> (l + 1) apart; the twiddle of the pair whose upper word is i is w_M^((i mod h) << l).
// Inverse: the same pairs, conjugate twiddle before the butterfly, levels descending (inverse after forward multiplies by 2^B).
template <int B, bool INV>
__device__ __forceinline__ void levels(double2 (&x)[1 << B], const double2 *tw, const int lo, const int q, const int s0) {
    constexpr int NV = 1 << B;
#pragma unroll
    for (int ss = 0; ss < B; ++ss) {
        const int s = INV ? B - 1 - ss : ss;
        const int ht = NV >> (s + 1);
#pragma unroll
        for (int pr = 0; pr < NV / 2; ++pr) {
            const int j = pr & (ht - 1), u = ((pr - j) << 1) + j, v = u + ht;
            const double2 w = tw[(lo + (j << q)) << (s0 + s)];                     // exponent < M / 2
            const double2 xa = x[u];
            if (!INV) {
                const double2 xb = x[v];
                x[u] = make_double2(xa.x + xb.x, xa.y + xb.y);
                x[v] = mul(make_double2(xa.x - xb.x, xa.y - xb.y), w);
            } else {
                const double2 xb = mulc(x[v], w);
                x[u] = make_double2(xa.x + xb.x, xa.y + xb.y);
                x[v] = make_double2(xa.x - xb.x, xa.y - xb.y);
            }
        }
    }
}

enum Mode { FWD, FWD_STATE, TAIL, INV, INV_MF };
// One pass over levels s0 .. s0 + B - 1.  FWD / INV: buffer to buffer.  FWD_STATE (s0 = 0): the window is read from the state.
// INV_MF (s0 = 0): the kept outputs go to mf, nothing is stored back.  TAIL (q = 0): forward, product with the spectrum, inverse.
// Ends with a barrier.
template <int B, Mode MODE>
__device__ __forceinline__ void pass(const Ctx &c, const int s0) {
    constexpr int NV = 1 << B;
    const int q = c.m - s0 - B;
    for (int w = c.t; w < (1 << (c.m - B)); w += THREADS) {
        const int lo = w & ((1 << q) - 1), base = ((w >> q) << (q + B)) | lo;
        double2 x[NV];
        if (MODE == FWD_STATE) {
            double vp[NV], vm[NV];
#pragma unroll
            for (int tt = 0; tt < NV; ++tt) {
                const int i = base + (tt << q);
                vp[tt] = 0.0; vm[tt] = 0.0;
                if (i < c.L + 2 * c.kt) {
                    int v = i - c.kt;                                             // in [-kt, L + kt), kt <= L / 2
                    if (v < 0) v += c.L; else if (v >= c.L) v -= c.L;
                    vp[tt] = c.rp[v]; vm[tt] = c.rm[v];
                }
            }
#pragma unroll
            for (int tt = 0; tt < NV; ++tt) x[tt] = make_double2(vp[tt] - vm[tt], vp[tt] + vm[tt]);
        } else {
#pragma unroll
            for (int tt = 0; tt < NV; ++tt) x[tt] = c.buf[pad(base + (tt << q))];
        }
        if (MODE == FWD || MODE == FWD_STATE || MODE == TAIL) levels<B, false>(x, c.tw, lo, q, s0);
        if (MODE == TAIL) {
#pragma unroll
            for (int tt = 0; tt < NV; ++tt) { const double sp = c.spec[base + tt]; x[tt] = make_double2(x[tt].x * sp, x[tt].y * sp); }
        }
        if (MODE == INV || MODE == INV_MF || MODE == TAIL) levels<B, true>(x, c.tw, lo, q, s0);
        if (MODE == INV_MF) {
#pragma unroll
            for (int tt = 0; tt < NV; ++tt) {
                const int i = base + (tt << q) - c.kt;                            // word kt + i is site i
                if (i >= 0 && i < c.L) c.mf[i] = x[tt].x / (x[tt].y + 1e-12);
            }
        } else {
#pragma unroll
            for (int tt = 0; tt < NV; ++tt) c.buf[pad(base + (tt << q))] = x[tt];
        }
    }
    __syncthreads();
}

// the passes of m: n3 of three levels, then n2 of two
__device__ __forceinline__ void split(const int m, int &n3, int &n2) { n3 = (m & 1) ? 3 : 2; n2 = (m - 3 * n3) >> 1; }

// forward passes 1 .. P - 2 (the middle ones) in order, or backwards for the inverse
template <bool INVERSE>
__device__ __forceinline__ void middle(const Ctx &c, const int n3, const int n2) {
    const int P = n3 + n2;
    for (int kk = 1; kk < P - 1; ++kk) {
        const int k = INVERSE ? P - 1 - kk : kk;
        const int s0 = k < n3 ? 3 * k : 3 * n3 + 2 * (k - n3);
        if (k < n3) pass<3, INVERSE ? INV : FWD>(c, s0); else pass<2, INVERSE ? INV : FWD>(c, s0);
    }
}

// mf of every site from the state (c.spec holds the taps' spectrum).  The caller has a barrier behind the last write of the state.
__device__ __forceinline__ void convolve(const Ctx &c) {
    int n3, n2;
    split(c.m, n3, n2);
    pass<3, FWD_STATE>(c, 0);
    middle<false>(c, n3, n2);
    if (n2) pass<2, TAIL>(c, c.m - 2); else pass<3, TAIL>(c, c.m - 3);
    middle<true>(c, n3, n2);
    pass<3, INV_MF>(c, 0);
}

// the taps' spectrum by the device's own forward transform, once per system: ktab[0 .. kt] (LDS or global) -> c.spec
__device__ __forceinline__ void build_spectrum(const Ctx &c, const double *ktab) {
    const int M = 1 << c.m;
    for (int i = c.t; i < M; i += THREADS) c.buf[pad(i)] = make_double2(0.0, 0.0);
    __syncthreads();
    for (int j = c.t; j <= c.kt; j += THREADS) {                                   // h[j mod M] = ktab[|j|]; M >= 2 kt + 1: no two taps meet
        c.buf[pad(j)].x = ktab[j];
        if (j) c.buf[pad(M - j)].x = ktab[j];
    }
    __syncthreads();
    int n3, n2;
    split(c.m, n3, n2);
    pass<3, FWD>(c, 0);
    middle<false>(c, n3, n2);
    if (n2) pass<2, FWD>(c, c.m - 2); else pass<3, FWD>(c, c.m - 3);
    const double scale = 1.0 / (double)M;
    for (int i = c.t; i < M; i += THREADS) c.spec[i] = c.buf[pad(i)].x * scale;
    __syncthreads();
}

}  // namespace pdek
