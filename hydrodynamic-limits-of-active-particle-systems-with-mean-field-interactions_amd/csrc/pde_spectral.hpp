// pde_spectral.hpp -- the Gaussian-kernel magnetisation of the wide shape by the convolution theorem (included by
// pde_wide_hip.hip inside its anonymous namespace; C ABI of the plan rule: include/pde_spectral.h).
//
// Hot path replaced: the direct circular convolution of pdew_mag (kernel_mode 1), O(L * reach); the reference multiplies
// rffts (IMEX_PDE_solver_class.py:164-165).  Per step and site x the solver needs  num[x] = sum_j ktab[|j|] s[(x + j) mod L]  and
// den[x], the same sum over tot (s = rho_plus - rho_minus, tot = rho_plus + rho_minus).  The taps are real, so ONE complex
// transform carries both: z = s + i tot, convolved with the taps; the real part is num, the imaginary part den.
//
// Blocks (overlap-save, the rule of pdes_plan_blocks): block b owns the sites [b S, min(L, (b + 1) S)), transforms the window
// z[(b S - kt + i) mod L], i < n + 2 kt (zero beyond, up to M = 2^m), and keeps the outputs kt .. kt + n - 1: the blocks
// partition [0, L), every site of mf is written once.  The taps are placed circularly, h[j mod M] = ktab[|j|]; their spectrum
// (real: the sequence is even) is built once per solve by the same forward sweeps, times 1 / M, and kept in slot order.
//
// Transform, as in ntt_conv.hpp: M = R2 R1 R0 (R0 = 128 along memory, R1, R2 <= 128), index i = i0 + R0 i1 + R0 R1 i2.  Three
// sweeps of short transforms held in LDS and registers (radix-16 then radix-8 passes), decimation in frequency going forward
// (natural order in, slot r of an axis holds frequency brev(r)), decimation in time coming back (slot order in, natural order
// out): nothing is un-permuted anywhere, the product with the spectrum is slot by slot.  Between sweeps the twiddle
// w_M^(k_axis * i_below << (m - A - sh)) is multiplied in where the strided sweep stores (forward) or loads (inverse); it is the
// product of two host-computed table entries, w^e = hi[e >> 10] lo[e & 1023], each from cos / sin of its own angle.
// The forward sweep over i0, the product and the inverse sweep over i0 touch the same 128 contiguous words: one kernel.
// Launches per convolution: 5 (m >= 15), 3 (m <= 14).  No fused middle: a 128 x 128 complex slab is 256 KB and does not fit
// LDS.  A complex word is a double2; a tile is 2048 words (32 KB), rows padded by one word, so a wave's
// 16-byte LDS accesses fall on distinct bank groups.  binary64 throughout, fma() explicit, no atomics, no workgroup waits on
// another.
#pragma once

constexpr int PDES_MAX_LOG2 = 21, PDES_MIN_LOG2 = 8;
constexpr int PDES_A0 = 7;                       // R0 = 128
constexpr int PDES_THREADS = 256;
constexpr int PDES_LG_TILE = 11, PDES_TILE = 1 << PDES_LG_TILE;      // complex words a workgroup holds in LDS
constexpr int PDES_NI = PDES_TILE / PDES_THREADS;                    // words per thread
constexpr size_t PDES_LDS_BYTES = (size_t)(PDES_TILE + 128 + 64) * sizeof(double2);

// ---- host: the blocks of one grid (pdes_plan; no device).  nullptr or the complaint.
inline const char *pdes_plan_blocks(int64_t L, int64_t kt, int max_log2, int &blocks, int &m, int &block_sites) {
    blocks = 0; m = 0; block_sites = 0;
    if (L < 1 || kt < 0 || 2 * kt > L) return "L >= 1 and 0 <= ktaps <= L / 2 required";
    const int cap = std::min(max_log2, PDES_MAX_LOG2);
    if (cap < PDES_MIN_LOG2) return "max_log2 must be at least 8";
    const int64_t full = (int64_t)1 << cap;
    int64_t B = 1, S = L;
    if (L + 2 * kt > full) {
        if (4 * kt > full) return "the kernel's reach is more than a quarter of the largest transform (2 ktaps > 2^cap / 2): not eligible for the spectral convolution";
        const int64_t usable = full - 2 * kt;
        B = (L + usable - 1) / usable;
        S = (L + B - 1) / B;
        B = (L + S - 1) / S;                                 // (no empty block at the end)
    }
    m = PDES_MIN_LOG2;
    while (((int64_t)1 << m) < S + 2 * kt) ++m;              // <= cap: S <= usable
    blocks = (int)B; block_sites = (int)S;
    return nullptr;
}
inline void pdes_split(int m, int &a1, int &a2) { a1 = std::min(7, m - PDES_A0); a2 = m - PDES_A0 - a1; }
inline int pdes_launches(int m) { return m - PDES_A0 > 7 ? 5 : 3; }
inline int pdes_lg_nc(int A, int sh) { return std::min(PDES_LG_TILE - A, sh); }                  // columns of a strided tile

// ---- host: tables.  w128[j] = exp(-2 pi i j / 128), j < 64; hi[j] = exp(-2 pi i 1024 j / M), lo[j] = exp(-2 pi i j / M), j < 1024
struct SpecTables { std::vector<double2> w128, hi, lo, taps; };
inline double2 pdes_root(unsigned long long j, unsigned long long n) {       // exp(-2 pi i j / n) from the angle itself
    const long double ang = -6.283185307179586476925286766559L * (long double)(j % n) / (long double)n;
    return make_double2((double)cosl(ang), (double)sinl(ang));
}
inline void pdes_build_tables(int m, int kt, const std::vector<double> &ktab, SpecTables &T) {
    const unsigned long long M = 1ull << m;
    T.w128.resize(64);
    for (int j = 0; j < 64; ++j) T.w128[j] = pdes_root(j, 128);
    const size_t nhi = std::max<size_t>(M >> 10, 1);
    T.hi.resize(nhi); T.lo.resize(1024);
    for (size_t j = 0; j < nhi; ++j) T.hi[j] = pdes_root(1024ull * j, M);
    for (size_t j = 0; j < 1024; ++j) T.lo[j] = pdes_root(j, M);
    T.taps.assign(M, make_double2(0.0, 0.0));                // h[j mod M] = ktab[|j|]   (M >= 2 kt + 1: no two taps meet)
    for (int j = -kt; j <= kt; ++j) T.taps[(size_t)((j + (long long)M) % (long long)M)].x = ktab[j < 0 ? -j : j];
}

struct SpecPlan {
    int m, a1, a2;                         // M = 2^m = R2 R1 R0, R_x = 2^a_x, a0 = 7 (a2 = 0: two sweeps only)
    int L, kt, S, B;                       // grid sites, reach, sites a block owns, blocks
    const double *rp, *rm;                 // [n_systems][L] the state
    double *mf;                            // [n_systems][L] the magnetisation
    double2 *data;                         // [n_systems][B][M] the blocks' windows, transformed in place
    const double *spec;                    // [M] spectrum of the taps in slot order, times 1 / M
    const double2 *w128, *thi, *tlo;
};

// ---- device
__device__ __forceinline__ double2 pdes_mul(const double2 a, const double2 w) {           // a w
    return make_double2(fma(a.x, w.x, -(a.y * w.y)), fma(a.x, w.y, a.y * w.x));
}
__device__ __forceinline__ double2 pdes_mulc(const double2 a, const double2 w) {          // a conj(w)
    return make_double2(fma(a.x, w.x, a.y * w.y), fma(a.y, w.x, -(a.x * w.y)));
}
__device__ __forceinline__ int pdes_bitrev(int v, int bits) { return (int)(__brev((unsigned)v) >> (32 - bits)); }

// B butterfly levels on the 2^B values of one thread: rows n + (t << lo_shift) of a transform of size 2^A = 128 >> tsh whose levels
// s0 .. s0 + B - 1 they carry out (pair distance 2^(A - 1 - level) rows); the twiddle of the pair whose upper row is i is
// w_R^((i mod h) << level) = w128[... << tsh].  Forward: decimation in frequency, levels ascending; inverse: the same pairs with the
// conjugate twiddle before the butterfly, levels descending (the exact mirror: inverse after forward multiplies by 2^B).
// N0: n is known to be zero, the pairs with j = 0 need no product.
template <int B, bool INV, bool N0>
__device__ __forceinline__ void pdes_reg_levels(double2 (&x)[1 << B], const double2 *__restrict__ wtab, const int n, const int lo_shift, const int s0, const int tsh) {
    constexpr int NV = 1 << B;
#pragma unroll
    for (int ss = 0; ss < B; ++ss) {
        const int s = INV ? B - 1 - ss : ss;
        const int ht = NV >> (s + 1);
#pragma unroll
        for (int pr = 0; pr < NV / 2; ++pr) {
            const int j = pr & (ht - 1), u = ((pr - j) << 1) + j, v = u + ht;
            const int e = ((n + (j << lo_shift)) << (s0 + s)) << tsh;                  // < 64
            const double2 xa = x[u];
            if (!INV) {
                const double2 xb = x[v];
                x[u] = make_double2(xa.x + xb.x, xa.y + xb.y);
                const double2 d = make_double2(xa.x - xb.x, xa.y - xb.y);
                if (N0 && j == 0) x[v] = d; else x[v] = pdes_mul(d, wtab[e]);
            } else {
                double2 xb = x[v];
                if (!(N0 && j == 0)) xb = pdes_mulc(xb, wtab[e]);
                x[u] = make_double2(xa.x + xb.x, xa.y + xb.y);
                x[v] = make_double2(xa.x - xb.x, xa.y - xb.y);
            }
        }
    }
}

// Transform of size 2^A of the NC = 2^lg_nc columns held in LDS, element (row r, column c) at buf[r * ld + c]: two register
// passes (2^AH = 16 rows a thread, then 2^AL = 8), in the opposite order coming back.  Ends with a barrier.
template <int A, bool INV>
__device__ __forceinline__ void pdes_lds_transform(double2 *buf, const int lg_nc, const int ld, const double2 *__restrict__ wtab, const int t) {
    constexpr int AH = A < 4 ? A : 4, AL = A - AH, TSH = 7 - A;
    const int NC = 1 << lg_nc;
    auto pass1 = [&]() {                                                   // rows n + (tt << AL): levels 0 .. AH - 1
        for (int w = t; w < (NC << AL); w += PDES_THREADS) {
            const int c = w & (NC - 1), n = w >> lg_nc;
            double2 x[1 << AH];
#pragma unroll
            for (int tt = 0; tt < (1 << AH); ++tt) x[tt] = buf[(n + (tt << AL)) * ld + c];
            pdes_reg_levels<AH, INV, false>(x, wtab, n, AL, 0, TSH);
#pragma unroll
            for (int tt = 0; tt < (1 << AH); ++tt) buf[(n + (tt << AL)) * ld + c] = x[tt];
        }
        __syncthreads();
    };
    auto pass2 = [&]() {                                                   // rows (u << AL) + v: levels AH .. A - 1
        if constexpr (AL > 0) {
            for (int w = t; w < (NC << AH); w += PDES_THREADS) {
                const int c = w & (NC - 1), u = w >> lg_nc;
                double2 x[1 << AL];
#pragma unroll
                for (int v = 0; v < (1 << AL); ++v) x[v] = buf[((u << AL) + v) * ld + c];
                pdes_reg_levels<AL, INV, true>(x, wtab, 0, 0, AH, TSH);
#pragma unroll
                for (int v = 0; v < (1 << AL); ++v) buf[((u << AL) + v) * ld + c] = x[v];
            }
            __syncthreads();
        }
    };
    if (!INV) { pass1(); pass2(); } else { pass2(); pass1(); }
}

// ---- sweep along a strided axis (axis 2: stride R0 R1, or axis 1: stride R0): a workgroup takes NC consecutive words (same other
// digits) for all R = 2^A values of the axis digit; blockIdx.y = system * B + block.
// Forward: transform, then the twiddle w_M^((k i_below) << lm) on the way out (slot r holds k = brev(r), i_below = the digits below
// the axis); inverse: the conjugate twiddle on the way in, then the transform.
// edge, forward (the first sweep): the input is the block's window of z = s + i tot, read from the state;
// edge, inverse (the last sweep): the output is  mf = num / (den + 1e-12)  of the block's own sites.
template <int A, bool INV>
__global__ __launch_bounds__(PDES_THREADS) void pdes_strided(const SpecPlan pl, const int axis, const int edge) {
    __shared__ double2 buf[PDES_TILE + 128];
    __shared__ double2 wtab[64];
    const int t = threadIdx.x;
    const int sh = axis == 2 ? PDES_A0 + pl.a1 : PDES_A0;           // log2 of the axis digit's stride
    const int lg_nc = min(PDES_LG_TILE - A, sh), NC = 1 << lg_nc, ld = NC + 1, words = NC << A;
    const int lm = pl.m - A - sh, lg_po = sh - lg_nc;               // tiles per value of the digits above the axis: 2^lg_po
    const int outer = (int)(blockIdx.x >> lg_po), inner0 = (int)(blockIdx.x & ((1u << lg_po) - 1u)) << lg_nc;
    const int base = (outer << (sh + A)) + inner0;                  // word index of (axis digit 0, first column)
    const int sys = __builtin_amdgcn_readfirstlane((int)blockIdx.y / pl.B), blk = (int)blockIdx.y - sys * pl.B;
    double2 *const sig = pl.data + ((size_t)blockIdx.y << pl.m);
    const bool first = !INV && edge, last = INV && edge;
    if (t < 64) wtab[t] = pl.w128[t];
    // ---- load (row r = axis digit, column c); all loads are issued before the first is used
    {
        double2 x[PDES_NI];
        if (first) {
            const double *rp = pl.rp + (size_t)sys * pl.L, *rm = pl.rm + (size_t)sys * pl.L;
            const int w0 = blk * pl.S - pl.kt, nwin = min(pl.S, pl.L - blk * pl.S) + 2 * pl.kt;
            double vp[PDES_NI], vm[PDES_NI];
#pragma unroll
            for (int u = 0; u < PDES_NI; ++u) {
                const int w = t + u * PDES_THREADS, c = w & (NC - 1), r = w >> lg_nc, g = base + (r << sh) + c;
                vp[u] = 0.0; vm[u] = 0.0;
                if (w < words && g < nwin) {
                    int v = (w0 + g) % pl.L;                         // the window wraps around the ring
                    if (v < 0) v += pl.L;
                    vp[u] = rp[v]; vm[u] = rm[v];
                }
            }
#pragma unroll
            for (int u = 0; u < PDES_NI; ++u) x[u] = make_double2(vp[u] - vm[u], vp[u] + vm[u]);
        } else {
            double2 hi[INV ? PDES_NI : 1], lo[INV ? PDES_NI : 1];
#pragma unroll
            for (int u = 0; u < PDES_NI; ++u) {
                const int w = t + u * PDES_THREADS, c = w & (NC - 1), r = w >> lg_nc, g = base + (r << sh) + c;
                x[u] = make_double2(0.0, 0.0);
                if (w < words) {
                    x[u] = sig[g];
                    if constexpr (INV) {
                        const unsigned e = ((unsigned)pdes_bitrev(r, A) * (unsigned)(inner0 + c)) << lm;     // < M
                        hi[u] = pl.thi[e >> 10]; lo[u] = pl.tlo[e & 1023u];
                    }
                }
            }
            if constexpr (INV) {
#pragma unroll
                for (int u = 0; u < PDES_NI; ++u)
                    if (t + u * PDES_THREADS < words) x[u] = pdes_mulc(x[u], pdes_mul(hi[u], lo[u]));
            }
        }
#pragma unroll
        for (int u = 0; u < PDES_NI; ++u) {
            const int w = t + u * PDES_THREADS, c = w & (NC - 1), r = w >> lg_nc;
            if (w < words) buf[r * ld + c] = x[u];
        }
    }
    __syncthreads();
    pdes_lds_transform<A, INV>(buf, lg_nc, ld, wtab, t);
    // ---- store
    if constexpr (!INV) {
        double2 hi[PDES_NI], lo[PDES_NI];
#pragma unroll
        for (int u = 0; u < PDES_NI; ++u) {
            const int w = t + u * PDES_THREADS, c = w & (NC - 1), r = w >> lg_nc;
            const unsigned e = w < words ? ((unsigned)pdes_bitrev(r, A) * (unsigned)(inner0 + c)) << lm : 0u;
            hi[u] = pl.thi[e >> 10]; lo[u] = pl.tlo[e & 1023u];
        }
#pragma unroll
        for (int u = 0; u < PDES_NI; ++u) {
            const int w = t + u * PDES_THREADS, c = w & (NC - 1), r = w >> lg_nc, g = base + (r << sh) + c;
            if (w < words) sig[g] = pdes_mul(buf[r * ld + c], pdes_mul(hi[u], lo[u]));
        }
    } else {
        double *mf = pl.mf + (size_t)sys * pl.L;
        const int n = min(pl.S, pl.L - blk * pl.S);
#pragma unroll
        for (int u = 0; u < PDES_NI; ++u) {
            const int w = t + u * PDES_THREADS, c = w & (NC - 1), r = w >> lg_nc, g = base + (r << sh) + c;
            if (w >= words) continue;
            const double2 v = buf[r * ld + c];
            if (!last) sig[g] = v;
            else if (g >= pl.kt && g < pl.kt + n) mf[blk * pl.S + g - pl.kt] = v.x / (v.y + 1e-12);   // word g is site b S - kt + g
        }
    }
}

// ---- the contiguous axis (i0, R0 = 128): forward sweep, product with the taps' spectrum (real, slot by slot), inverse sweep: one
// kernel, a workgroup takes 16 rows of 128 contiguous words.  FWD_ONLY: the real part of the forward sweep over M goes to spec_out
// (building the taps' spectrum).
template <bool FWD_ONLY>
__global__ __launch_bounds__(PDES_THREADS) void pdes_contig(const SpecPlan pl, double *__restrict__ spec_out) {
    __shared__ double2 buf[PDES_TILE + 128];
    __shared__ double2 wtab[64];
    const int t = threadIdx.x;
    const int lg_nr = min(PDES_LG_TILE - PDES_A0, pl.m - PDES_A0), NR = 1 << lg_nr, ld = NR + 1, words = NR << PDES_A0;
    const int row0 = (int)blockIdx.x << lg_nr;
    double2 *const sig = pl.data + ((size_t)blockIdx.y << pl.m);
    if (t < 64) wtab[t] = pl.w128[t];
    double sp[PDES_NI];                                          // the spectrum at this thread's slots: asked for now, used after the forward sweep
    {
        double2 x[PDES_NI];
#pragma unroll
        for (int u = 0; u < PDES_NI; ++u) {
            const int w = t + u * PDES_THREADS, i0 = w & 127, r = w >> PDES_A0, g = ((row0 + r) << PDES_A0) + i0;
            x[u] = make_double2(0.0, 0.0); sp[u] = 0.0;
            if (w < words) { x[u] = sig[g]; if (!FWD_ONLY) sp[u] = pl.spec[g]; }
        }
#pragma unroll
        for (int u = 0; u < PDES_NI; ++u) {
            const int w = t + u * PDES_THREADS, i0 = w & 127, r = w >> PDES_A0;
            if (w < words) buf[i0 * ld + r] = x[u];
        }
    }
    __syncthreads();
    pdes_lds_transform<PDES_A0, false>(buf, lg_nr, ld, wtab, t);
    if (FWD_ONLY) {
        const double scale = 1.0 / (double)(1ull << pl.m);
#pragma unroll
        for (int u = 0; u < PDES_NI; ++u) {
            const int w = t + u * PDES_THREADS, i0 = w & 127, r = w >> PDES_A0, g = ((row0 + r) << PDES_A0) + i0;
            if (w < words) spec_out[g] = buf[i0 * ld + r].x * scale;
        }
        return;
    }
#pragma unroll
    for (int u = 0; u < PDES_NI; ++u) {                          // every thread its own slots: no barrier before, one after
        const int w = t + u * PDES_THREADS, i0 = w & 127, r = w >> PDES_A0;
        if (w < words) { const double2 v = buf[i0 * ld + r]; buf[i0 * ld + r] = make_double2(v.x * sp[u], v.y * sp[u]); }
    }
    __syncthreads();
    pdes_lds_transform<PDES_A0, true>(buf, lg_nr, ld, wtab, t);
#pragma unroll
    for (int u = 0; u < PDES_NI; ++u) {
        const int w = t + u * PDES_THREADS, i0 = w & 127, r = w >> PDES_A0, g = ((row0 + r) << PDES_A0) + i0;
        if (w < words) sig[g] = buf[i0 * ld + r];
    }
}

// ---- launches
template <bool INV>
inline void pdes_launch_strided(int A, int axis, int edge, const SpecPlan &pl, unsigned nz) {
    const int sh = axis == 2 ? PDES_A0 + pl.a1 : PDES_A0;
    const dim3 grid(1u << (pl.m - pdes_lg_nc(A, sh) - A), nz), block(PDES_THREADS);
#define PDES_CASE(AA) case AA: hipLaunchKernelGGL((pdes_strided<AA, INV>), grid, block, 0, nullptr, pl, axis, edge); break;
    switch (A) { PDES_CASE(1) PDES_CASE(2) PDES_CASE(3) PDES_CASE(4) PDES_CASE(5) PDES_CASE(6) PDES_CASE(7) default: break; }
#undef PDES_CASE
}
inline dim3 pdes_contig_grid(const SpecPlan &pl, unsigned nz) {
    return dim3(1u << (pl.m - PDES_A0 - std::min(PDES_LG_TILE - PDES_A0, pl.m - PDES_A0)), nz);
}
// the forward sweeps over the strided axes; from_state: the first one reads the blocks' windows from the state
inline void pdes_forward_strided(const SpecPlan &pl, unsigned nz, bool from_state) {
    if (pl.a2) pdes_launch_strided<false>(pl.a2, 2, from_state ? 1 : 0, pl, nz);
    pdes_launch_strided<false>(pl.a1, 1, from_state && !pl.a2 ? 1 : 0, pl, nz);
}
// mf of every block of every system from the state: 3 or 5 launches on the null stream
inline void pdes_convolve(const SpecPlan &pl, unsigned nz) {
    pdes_forward_strided(pl, nz, true);
    hipLaunchKernelGGL(pdes_contig<false>, pdes_contig_grid(pl, nz), dim3(PDES_THREADS), 0, nullptr, pl, (double *)nullptr);
    pdes_launch_strided<true>(pl.a1, 1, pl.a2 ? 0 : 1, pl, nz);
    if (pl.a2) pdes_launch_strided<true>(pl.a2, 2, 1, pl, nz);
}
// the taps' spectrum: pl.data holds the M taps (one block, one system), spec receives M doubles
inline void pdes_build_spectrum(const SpecPlan &pl, double *spec) {
    pdes_forward_strided(pl, 1u, false);
    hipLaunchKernelGGL(pdes_contig<true>, pdes_contig_grid(pl, 1u), dim3(PDES_THREADS), 0, nullptr, pl, spec);
}
