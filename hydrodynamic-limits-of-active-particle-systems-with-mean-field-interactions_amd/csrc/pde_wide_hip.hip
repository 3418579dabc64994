// pde_wide_hip.hip -- MI355X (gfx950) implementation of the C ABI in include/pde_wide.h: the hydrodynamic-limit solver of
// pde_hip.hip with ONE system spread over many workgroups; and of its resumable form pdewr_solve (include/pde_resume.h).
// A resumed launch takes the checkpoint's fields through the `init` form of pdew_renorm_fwd: the per-slab sums and forward
// maps it forms from them are, operation for operation, those the fused form left when it stored these same values, so the
// chain has the single launch's bits (for the same number of slabs).
//
// Same scheme and order of operations as pde_kernel (ref IMEX_PDE_solver_class.py:187-290): magnetisation -> observables ->
// tracers -> implicit diffusion -> reaction / upwind advection / clip -> mass renormalisation, binary64 throughout.
// The L sites are cut into G contiguous slabs, one workgroup each; a batch is a grid of (G, n_systems).  The five fields
// live in global memory; LDS is working storage inside a kernel.  Whatever crosses slabs crosses at a KERNEL BOUNDARY: a
// time step is a chain of launches on one stream, all steps enqueued without a host synchronisation, no workgroup ever
// waits on another.
//
//   mag        magnetisation of the slab (local ratio | direct circular convolution | global mean), partial sums of the
//              observables, Fourier partials, snapshots
//   tracers    Euler-Maruyama tracers, spread over workgroups by index                            (only with tracers)
//   obs        one workgroup per system: combines the partials into the series, tracer window statistics
//   fwd_bwd    forward sweep of the slab from its entry value, composes the slab's backward map
//   bwd        backward sweep of the slab from its entry value, leaves x[0], x[L-1] for the periodic corner correction
//   react      corner correction, reaction, upwind advection, clip; partial masses before / after
//   renorm_fwd mass renormalisation, partial sums of the new state, composes the slab's forward map of the next step
//
// The sweeps of the Thomas solve are scans of affine maps in two levels: a slab composes its map (thread chunks, then the
// workgroup scan of pde_common.hpp), every workgroup scans the <= G slab maps before its own redundantly in the same
// fixed order, then replays its sweep from the entry value.  Sums are per-slab partials in global memory, combined in a
// fixed order by whoever needs them: no floating-point atomics, the same call gives the same bits, and a system's bits do
// not depend on its index in the batch.
//
// The convolution (kernel_mode 1) is where the time goes: R = 8 consecutive sites per thread with a sliding register window,
// so a tap and a source value read from LDS feed 16 fused multiply-adds; when a slab has fewer than 256 groups of 8 sites
// the spare threads take a share of the tap range each and the shares are added in a fixed order.  Source window and
// taps are staged through LDS in chunks of TB taps; window slots are padded by one per 8 so that lanes 8 sites apart hit
// different banks.  fma() is explicit here (the build has -ffp-contract=off).
// With pde_params.convolution = 1 the convolution is evaluated by the convolution theorem instead (pde_spectral.hpp): 3 or 5
// launches in front of pdew_mag write the magnetisation field, and pdew_mag does the rest (sums, snapshots, Fourier partials).

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pde_wide.h"
#include "pde_spectral.h"
#include "pde_common.hpp"
#include "dev_mem.hpp"

namespace {

using namespace pde_common;
std::string g_err, g_spec_err, g_err_r;

#include "pde_spectral.hpp"

constexpr int R = 8;                    // consecutive sites per thread in the convolution
constexpr int TB = 128;                 // taps per staged chunk, a multiple of R
constexpr int NTP_MAX = 8;              // most shares of the tap range
constexpr int SUB = NT * R;             // a slab is convolved in sub-slabs of at most this many sites

enum { P_ST = 0, P_SS, P_SMF, P_SV, P_M0, P_M1, NSLOT };   // per-slab partial sums: tot, s, m field, (tot - mean)^2, mass before / after

struct WArgs {
    pde_params p;
    PdeSpan span;                       // the absolute steps this launch runs and the rows it records (pde_common.hpp)
    int G, q, r;                        // slab g: q + (g < r) sites from g * q + min(g, r)
    int n_snap, ktaps;
    int spectral;                       // the kernel_mode 1 convolution comes from the transforms of pde_spectral.hpp (sp)
    SpecPlan sp;
    double dx, sm_coef, sm_denom;
    const double *beta, *rho_p0, *rho_m0, *tracer_x0;
    const int8_t *tracer_s0;
    const double *rand_u, *rand_n;
    const double *fw, *finv, *fu, *fz, *ktab, *twc, *tws;
    double *m_series, *var_series, *v_eff, *D_eff, *snapshots, *m_snapshots, *fft_re, *fft_im;    // outputs (null: not wanted)
    double *rp, *rm, *xp, *xm, *mf;     // [n_systems][L] each
    double *part;                       // [n_systems][NSLOT][G]
    double *fpart;                      // [n_systems][2 * n_fft_modes][G]
    double *fmap, *bmap;                // [n_systems][G][3]  slab maps (A, B of rho_plus, B of rho_minus)
    double *corner;                     // [n_systems][4]     x_plus[0], x_minus[0], x_plus[L-1], x_minus[L-1] before the corner correction
    double *hist;                       // [n_systems][window][n_tracers]
    double *trx; int8_t *trs;           // [n_systems][n_tracers]
};

struct ConvShape { int ng, ntp, tb, tpl, nch, W, WP; };

// how a sub-slab of nsub sites is convolved: ng groups of R sites, ntp shares of the tap range of tpl taps each, staged in
// nch chunks of tb taps; W window slots per share (WP with the padding)
__host__ __device__ inline ConvShape conv_shape(int nsub, int ktaps) {
    ConvShape c;
    const int ntaps = 2 * ktaps + 1;
    c.ng = (nsub + R - 1) / R;
    c.ntp = NT / c.ng;
    if (c.ntp > NTP_MAX) c.ntp = NTP_MAX;
    if (c.ntp > (ntaps + R - 1) / R) c.ntp = (ntaps + R - 1) / R;
    if (c.ntp < 1) c.ntp = 1;
    c.tpl = (ntaps + c.ntp - 1) / c.ntp;
    c.tb = (c.tpl + R - 1) / R * R;
    if (c.tb > TB) c.tb = TB;
    c.nch = (c.tpl + c.tb - 1) / c.tb;
    c.W = c.tb + c.ng * R;
    c.WP = c.W + c.W / R + 1;
    return c;
}
__host__ __device__ inline size_t conv_lds_doubles(const ConvShape &c) { return (size_t)c.ntp * c.WP * 2 + (size_t)c.ntp * c.tb; }

__device__ inline void slab_of(const WArgs &a, int g, int &a0, int &n) { a0 = g * a.q + (g < a.r ? g : a.r); n = a.q + (g < a.r ? 1 : 0); }

// sum of G partials in a fixed order; every thread gets it
__device__ inline double combine(const double *v, int G, double *red) {
    double s = 0.0;
    for (int i = threadIdx.x; i < G; i += NT) s += v[i];
    return block_sum(s, red);
}

// the value entering slab g's sweep: the maps of the slabs before it (in sweep order) composed and applied to 0
__device__ inline void slab_entry(const double *maps, int G, int g, bool backward, double4 *scan, double &ep, double &em) {
    const int count = backward ? G - 1 - g : g;
    if (count == 0) { ep = 0.0; em = 0.0; return; }
    const int cg = (count + NT - 1) / NT, e0 = threadIdx.x * cg, e1 = min(count, e0 + cg);
    double A = 1.0, Bp = 0.0, Bm = 0.0;
    for (int e = e0; e < e1; ++e) {
        const double *m = maps + (size_t)(backward ? G - 1 - e : e) * 3;
        const double mA = m[0];
        Bp = mA * Bp + m[1]; Bm = mA * Bm + m[2]; A = mA * A;
    }
    const double4 *all = scan_affine2_all(A, Bp, A, Bm, scan, false);
    ep = all[NT - 1].y; em = all[NT - 1].w;
}

#define WIDE_PROLOGUE                                                                                                   \
    const int L = a.p.L, t = threadIdx.x, g = blockIdx.x, sys = blockIdx.y;                                            \
    int a0, n;                                                                                                          \
    slab_of(a, g, a0, n);                                                                                               \
    const size_t fo = (size_t)sys * L;                                                                                  \
    double *rp = a.rp + fo, *rm = a.rm + fo, *xp = a.xp + fo, *xm = a.xm + fo, *mf = a.mf + fo;                         \
    double *part = a.part + (size_t)sys * NSLOT * a.G;                                                                  \
    (void)rp; (void)rm; (void)xp; (void)xm; (void)mf; (void)part; (void)t; (void)L

// ---- renormalise (or take the initial state), partial sums of the new state, forward map of the slab
__global__ __launch_bounds__(NT) void pdew_renorm_fwd(const WArgs a, const int init) {
    __shared__ double red[NT / 64];
    __shared__ double4 scan[2 * NT];
    WIDE_PROLOGUE;
    double sc = 1.0;
    if (!init) {
        const double m0 = combine(part + (size_t)P_M0 * a.G, a.G, red), m1 = combine(part + (size_t)P_M1 * a.G, a.G, red);
        sc = m0 / m1;
    } else {
        const int ntr = a.p.n_tracers;
        for (int i = g * NT + t; i < ntr; i += a.G * NT) {
            a.trx[(size_t)sys * ntr + i] = a.tracer_x0[(size_t)sys * ntr + i];
            a.trs[(size_t)sys * ntr + i] = a.tracer_s0[(size_t)sys * ntr + i];
        }
    }
    const int chunk = (n + NT - 1) / NT, c0 = a0 + t * chunk, c1 = min(a0 + n, c0 + chunk);
    double A = 1.0, Bp = 0.0, Bm = 0.0, ss = 0.0, st = 0.0;
    for (int i = c0; i < c1; ++i) {
        double vp, vm;
        if (init) { vp = a.rho_p0[fo + i]; vm = a.rho_m0[fo + i]; }
        else { vp = rp[i] * sc; vm = rm[i] * sc; }
        rp[i] = vp; rm[i] = vm;
        const double w = a.fw[i];
        Bp = vp - w * Bp; Bm = vm - w * Bm; A = -w * A;
        ss += vp - vm; st += vp + vm;
    }
    const double4 *all = scan_affine2_all(A, Bp, A, Bm, scan, false);
    if (t == 0) {
        const double4 tot = all[NT - 1];
        double *m = a.fmap + ((size_t)sys * a.G + g) * 3;
        m[0] = tot.x; m[1] = tot.y; m[2] = tot.w;
    }
    ss = block_sum(ss, red); st = block_sum(st, red);
    if (t == 0) { part[(size_t)P_SS * a.G + g] = ss; part[(size_t)P_ST * a.G + g] = st; }
}

// ---- forward sweep y_i = d_i - w_i y_{i-1} of the slab (into xp, xm), then the slab's map of the backward sweep
__global__ __launch_bounds__(NT) void pdew_fwd_bwd(const WArgs a) {
    __shared__ double4 scan[2 * NT];
    WIDE_PROLOGUE;
    double ep, em;
    slab_entry(a.fmap + (size_t)sys * a.G * 3, a.G, g, false, scan, ep, em);
    const int chunk = (n + NT - 1) / NT, c0 = a0 + t * chunk, c1 = min(a0 + n, c0 + chunk);
    double A = 1.0, Bp = 0.0, Bm = 0.0;
    for (int i = c0; i < c1; ++i) { const double w = a.fw[i]; Bp = rp[i] - w * Bp; Bm = rm[i] - w * Bm; A = -w * A; }
    const double4 *all = scan_affine2_all(A, Bp, A, Bm, scan, false);
    double yp = ep, ym = em;
    if (t > 0) { const double4 pv = all[t - 1]; yp = pv.x * ep + pv.y; ym = pv.z * em + pv.w; }
    for (int i = c0; i < c1; ++i) { const double w = a.fw[i]; yp = rp[i] - w * yp; ym = rm[i] - w * ym; xp[i] = yp; xm[i] = ym; }
    // backward: x_i = inv_i y_i - (u_i inv_i) x_{i+1}; this thread re-reads only what it stored itself
    A = 1.0; Bp = 0.0; Bm = 0.0;
    for (int i = c1 - 1; i >= c0; --i) { const double iv = a.finv[i], q = -a.fu[i] * iv; Bp = xp[i] * iv + q * Bp; Bm = xm[i] * iv + q * Bm; A = q * A; }
    all = scan_affine2_all(A, Bp, A, Bm, scan, true);
    if (t == 0) {
        const double4 tot = all[NT - 1];
        double *m = a.bmap + ((size_t)sys * a.G + g) * 3;
        m[0] = tot.x; m[1] = tot.y; m[2] = tot.w;
    }
}

// ---- backward sweep of the slab, in place in xp, xm
__global__ __launch_bounds__(NT) void pdew_bwd(const WArgs a) {
    __shared__ double4 scan[2 * NT];
    WIDE_PROLOGUE;
    double ep, em;
    slab_entry(a.bmap + (size_t)sys * a.G * 3, a.G, g, true, scan, ep, em);
    const int chunk = (n + NT - 1) / NT, c0 = a0 + t * chunk, c1 = min(a0 + n, c0 + chunk);
    double A = 1.0, Bp = 0.0, Bm = 0.0;
    for (int i = c1 - 1; i >= c0; --i) { const double iv = a.finv[i], q = -a.fu[i] * iv; Bp = xp[i] * iv + q * Bp; Bm = xm[i] * iv + q * Bm; A = q * A; }
    const double4 *all = scan_affine2_all(A, Bp, A, Bm, scan, true);
    const int j = NT - 1 - t;
    double vp = ep, vm = em;
    if (j > 0) { const double4 pv = all[j - 1]; vp = pv.x * ep + pv.y; vm = pv.z * em + pv.w; }
    for (int i = c1 - 1; i >= c0; --i) {
        const double iv = a.finv[i], q = -a.fu[i] * iv;
        vp = xp[i] * iv + q * vp; vm = xm[i] * iv + q * vm;
        xp[i] = vp; xm[i] = vm;
        if (i == 0) { a.corner[(size_t)sys * 4 + 0] = vp; a.corner[(size_t)sys * 4 + 1] = vm; }
        if (i == L - 1) { a.corner[(size_t)sys * 4 + 2] = vp; a.corner[(size_t)sys * 4 + 3] = vm; }
    }
}

// ---- corner correction, reaction, upwind advection, clip (ref :195-233); partial masses before and after
__global__ __launch_bounds__(NT) void pdew_react(const WArgs a) {
    __shared__ double red[NT / 64];
    WIDE_PROLOGUE;
    const double beta = a.beta[sys], dx = a.dx, dt = a.p.dt, lam = a.p.lam;
    const int per = a.p.periodic;
    double fp = 0.0, fm = 0.0;
    if (per) {                                                 // Sherman-Morrison correction for the two corner entries
        const double *c = a.corner + (size_t)sys * 4;
        fp = (c[0] + a.sm_coef * c[2]) / a.sm_denom; fm = (c[1] + a.sm_coef * c[3]) / a.sm_denom;
    }
    // the diffused fields at site i (a neighbour across the slab edge is one cell read from global memory)
    auto XP = [&](int i) { return per ? xp[i] - a.fz[i] * fp : xp[i]; };
    auto XM = [&](int i) { return per ? xm[i] - a.fz[i] * fm : xm[i]; };
    double m0 = 0.0, m1 = 0.0;
    for (int i = a0 + t; i < a0 + n; i += NT) {
        const double vp = XP(i), vm = XM(i), m = mf[i];
        m0 += vp + vm;
        const double Rp = cw_rate(beta, -1.0, m) * vm - cw_rate(beta, 1.0, m) * vp;
        double np_, nm_;
        if (!a.p.anchored_minus) {
            const double dpl = i > 0 ? (vp - XP(i - 1)) / dx : (per ? (vp - XP(L - 1)) / dx : 0.0);       // right-moving: backward difference
            const double dmr = i < L - 1 ? (XM(i + 1) - vm) / dx : (per ? (XM(0) - vm) / dx : 0.0);       // left-moving: forward difference
            np_ = vp + dt * (-lam * dpl + Rp); nm_ = vm + dt * (lam * dmr + (-Rp));
            np_ = np_ < 0.0 ? 0.0 : np_;
        } else {                                               // reaction first (star), then advection of star_plus
            double sp_ = vp + dt * Rp;
            sp_ = sp_ < 0.0 ? 0.0 : sp_;
            nm_ = vm + dt * (-Rp);
            double dpl = 0.0;
            if (i > 0 || per) {
                const int k = i > 0 ? i - 1 : L - 1;
                const double wp = XP(k), wm = XM(k), mk = mf[k];
                const double Rk = cw_rate(beta, -1.0, mk) * wm - cw_rate(beta, 1.0, mk) * wp;
                double sk = wp + dt * Rk;
                sk = sk < 0.0 ? 0.0 : sk;
                dpl = (sp_ - sk) / dx;
            }
            np_ = sp_ + dt * (-lam * dpl);
            np_ = np_ < 0.0 ? 0.0 : np_;
        }
        nm_ = nm_ < 0.0 ? 0.0 : nm_;
        rp[i] = np_; rm[i] = nm_;
        m1 += np_ + nm_;
    }
    m0 = block_sum(m0, red); m1 = block_sum(m1, red);
    if (t == 0) { part[(size_t)P_M0 * a.G + g] = m0; part[(size_t)P_M1 * a.G + g] = m1; }
}

// ---- magnetisation of the current state (ref :156-168), partial sums of the observables (ref :243-255), snapshots
__global__ __launch_bounds__(NT) void pdew_mag(const WArgs a, const int nstep) {
    extern __shared__ double lds[];
    __shared__ double red[NT / 64];
    WIDE_PROLOGUE;
    const double mean_t = combine(part + (size_t)P_ST * a.G, a.G, red) / L;
    if (a.p.kernel_mode == 0) {
        for (int i = a0 + t; i < a0 + n; i += NT) mf[i] = (rp[i] - rm[i]) / (rp[i] + rm[i] + 1e-12);
    } else if (a.p.kernel_mode == 2) {
        const double s = combine(part + (size_t)P_SS * a.G, a.G, red), w = combine(part + (size_t)P_ST * a.G, a.G, red);
        const double m_global = s / (w + 1e-12);
        for (int i = a0 + t; i < a0 + n; i += NT) mf[i] = m_global;
    } else if (a.spectral) {                                   // mf of every site was written by the transforms launched before this kernel
    } else {
        for (int sub0 = 0; sub0 < n; sub0 += SUB) {
            const int nsub = min(SUB, n - sub0), s0 = a0 + sub0;
            const ConvShape c = conv_shape(nsub, a.ktaps);
            double *winS = lds, *winT = winS + (size_t)c.ntp * c.WP, *taps = winT + (size_t)c.ntp * c.WP;
            const bool active = t < c.ng * c.ntp;
            const int sg = t % c.ng, tp = active ? t / c.ng : 0;
            const double *ws = winS + (size_t)tp * c.WP, *wt = winT + (size_t)tp * c.WP, *tk = taps + (size_t)tp * c.tb;
            double num[R], den[R];
#pragma unroll
            for (int k = 0; k < R; ++k) { num[k] = 0.0; den[k] = 0.0; }
            for (int ch = 0; ch < c.nch; ++ch) {
                __syncthreads();
                // stage: share p's window slot x holds s, tot of site s0 + jlo_p + ch * tb + x (mod L); its tap jj is that of
                // distance |jlo_p + ch * tb + jj|, zero beyond the share's end
                for (int e = t; e < c.ntp * c.W; e += NT) {
                    const int p = e / c.W, x = e - p * c.W;
                    int v = s0 - a.ktaps + p * c.tpl + ch * c.tb + x;      // in (-L, 3 L]
                    if (v < 0) v += L;
                    if (v >= L) { v -= L; if (v >= L) v %= L; }
                    const double vp = rp[v], vm = rm[v];
                    const int pi = p * c.WP + x + x / R;
                    winS[pi] = vp - vm; winT[pi] = vp + vm;
                }
                for (int e = t; e < c.ntp * c.tb; e += NT) {
                    const int p = e / c.tb, jj = e - p * c.tb;
                    const int jl = ch * c.tb + jj, j = -a.ktaps + p * c.tpl + jl;
                    taps[e] = (jl < c.tpl && j <= a.ktaps) ? a.ktab[j < 0 ? -j : j] : 0.0;
                }
                __syncthreads();
                if (active) {
                    // ring: window slot sg * R + y lives in sw[y % R]; tap jj needs y = jj .. jj + R - 1
                    double sw[R], tw[R];
#pragma unroll
                    for (int y = 0; y < R - 1; ++y) { sw[y] = ws[sg * (R + 1) + y]; tw[y] = wt[sg * (R + 1) + y]; }
                    const int nb = c.tb / R;
                    for (int b = 0; b < nb; ++b) {
                        const int x0 = (sg + b) * (R + 1);
                        double ns[R], nt_[R], kv[R];
                        ns[0] = ws[x0 + R - 1]; nt_[0] = wt[x0 + R - 1];
#pragma unroll
                        for (int u = 1; u < R; ++u) { ns[u] = ws[x0 + R + u]; nt_[u] = wt[x0 + R + u]; }
#pragma unroll
                        for (int u = 0; u < R; ++u) kv[u] = tk[b * R + u];
#pragma unroll
                        for (int u = 0; u < R; ++u) {
                            sw[(u + R - 1) % R] = ns[u]; tw[(u + R - 1) % R] = nt_[u];
#pragma unroll
                            for (int k = 0; k < R; ++k) { num[k] = fma(kv[u], sw[(u + k) % R], num[k]); den[k] = fma(kv[u], tw[(u + k) % R], den[k]); }
                        }
                    }
                }
            }
            if (c.ntp == 1) {
                if (active)
#pragma unroll
                    for (int k = 0; k < R; ++k) if (sg * R + k < nsub) mf[s0 + sg * R + k] = num[k] / (den[k] + 1e-12);
            } else {                                           // add the shares of the tap range in a fixed order
                __syncthreads();
                double *pn = lds, *pd = lds + (size_t)c.ntp * c.ng * R;
                if (active)
#pragma unroll
                    for (int k = 0; k < R; ++k) { pn[(size_t)tp * c.ng * R + sg * R + k] = num[k]; pd[(size_t)tp * c.ng * R + sg * R + k] = den[k]; }
                __syncthreads();
                for (int x = t; x < nsub; x += NT) {
                    double sn = 0.0, sd = 0.0;
                    for (int p = 0; p < c.ntp; ++p) { sn += pn[(size_t)p * c.ng * R + x]; sd += pd[(size_t)p * c.ng * R + x]; }
                    mf[s0 + x] = sn / (sd + 1e-12);
                }
            }
        }
    }
    __syncthreads();
    double smf = 0.0, sv = 0.0;
    const bool snap = nstep % a.p.snapshot_interval == 0 && nstep >= a.span.row0;   // a resumed launch records nothing of its checkpoint's step
    const size_t so = ((size_t)sys * a.n_snap + (snap ? nstep / a.p.snapshot_interval - a.span.snap0 : 0)) * L;
    for (int i = a0 + t; i < a0 + n; i += NT) {
        const double vp = rp[i], vm = rm[i], d = vp + vm - mean_t;
        smf += mf[i]; sv += d * d;
        if (snap) {
            if (a.snapshots) a.snapshots[so + i] = vp + vm;
            if (a.m_snapshots) a.m_snapshots[so + i] = vp - vm;
        }
    }
    smf = block_sum(smf, red); sv = block_sum(sv, red);
    if (t == 0) { part[(size_t)P_SMF * a.G + g] = smf; part[(size_t)P_SV * a.G + g] = sv; }
    if (a.fft_re) {                                            // this slab's share of sum total_i (cos - i sin)(2 pi k i / L): a wave per mode
        const int lane = t & 63, nf = a.p.n_fft_modes;
        double *fpart = a.fpart + (size_t)sys * 2 * nf * a.G;
        for (int k = t >> 6; k < nf; k += NT / 64) {
            double re = 0.0, im = 0.0;
            int ph = (int)(((long long)k * (a0 + lane)) % L);
            const int stp = (int)(((long long)k * 64) % L);
            for (int i = a0 + lane; i < a0 + n; i += 64) {
                const double v = rp[i] + rm[i];
                re += v * a.twc[ph]; im -= v * a.tws[ph];
                ph += stp; if (ph >= L) ph -= L;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { re += __shfl_xor(re, off); im += __shfl_xor(im, off); }
            if (lane == 0) { fpart[(size_t)(2 * k) * a.G + g] = re; fpart[(size_t)(2 * k + 1) * a.G + g] = im; }
        }
    }
}

// ---- tracers (ref :257-287), one thread per tracer
__global__ __launch_bounds__(NT) void pdew_tracers(const WArgs a, const int nstep) {
    const int L = a.p.L, sys = blockIdx.y, ntr = a.p.n_tracers, i = blockIdx.x * NT + threadIdx.x;
    if (i >= ntr) return;
    const double *mf = a.mf + (size_t)sys * L;
    double *trx = a.trx + (size_t)sys * ntr, *hist = a.hist + (size_t)sys * a.p.window * ntr;
    int8_t *trs = a.trs + (size_t)sys * ntr;
    const double beta = a.beta[sys], dt = a.p.dt, noise_amp = sqrt(2.0 * a.p.gamma * dt);
    double xu = trx[i];
    double xw = fmod(xu, a.p.xlim);                            // numpy's % : floor modulo
    if (xw != 0.0 && xw < 0.0) xw += a.p.xlim;
    const int idx = (int)(xw / a.dx) % L;
    const double m_loc = mf[idx];
    int s = trs[i];
    double u, gn;
    if (a.rand_u) {
        const size_t o = ((size_t)sys * a.span.n_rows + (nstep - a.span.row0)) * ntr + i;
        u = a.rand_u[o]; gn = a.rand_n[o];
    } else {
        tracer_noise(a.p.seed, nstep, i, sys, u, gn);
    }
    const double rate = cw_rate(beta, (double)s, m_loc);
    if (u < rate * dt) s = -s;
    xu += a.p.lam * (double)s * dt + noise_amp * gn;
    trx[i] = xu; trs[i] = (int8_t)s;
    hist[(size_t)(nstep % a.p.window) * ntr + i] = xu;
}

// ---- one workgroup per system: the series of this step from the partials, the tracers' window statistics
__global__ __launch_bounds__(NT) void pdew_obs(const WArgs a, const int nstep) {
    __shared__ double red[NT / 64];
    const int L = a.p.L, t = threadIdx.x, sys = blockIdx.y, G = a.G, ntr = a.p.n_tracers;
    const size_t row = (size_t)sys * a.span.n_rows + (nstep - a.span.row0);
    const double *part = a.part + (size_t)sys * NSLOT * G;
    if (a.m_series) {
        double m;
        if (a.p.kernel_mode == 2) {
            const double s = combine(part + (size_t)P_SS * G, G, red), w = combine(part + (size_t)P_ST * G, G, red);
            m = s / (w + 1e-12);
        } else {
            m = combine(part + (size_t)P_SMF * G, G, red) / L;
        }
        if (t == 0) a.m_series[row] = m;
    }
    if (a.var_series) {
        const double sv = combine(part + (size_t)P_SV * G, G, red);
        if (t == 0) a.var_series[row] = sv / L;
    }
    if (a.fft_re) {
        const int nf = a.p.n_fft_modes;
        const double *fpart = a.fpart + (size_t)sys * 2 * nf * G;
        for (int e = t; e < 2 * nf; e += NT) {
            double s = 0.0;
            for (int g = 0; g < G; ++g) s += fpart[(size_t)e * G + g];
            double *out = (e & 1) ? a.fft_im : a.fft_re;
            out[row * nf + (e >> 1)] = s / L;
        }
    }
    if (ntr > 0 && (a.v_eff || a.D_eff)) {
        const double dt = a.p.dt;
        if (nstep >= a.p.window) {                             // dr = x_n - x_{n - window + 1}  (ref: history[-window])
            const double *trx = a.trx + (size_t)sys * ntr;
            const double *old = a.hist + (size_t)sys * a.p.window * ntr + (size_t)((nstep + 1) % a.p.window) * ntr;
            double sdr = 0.0;
            for (int i = t; i < ntr; i += NT) sdr += trx[i] - old[i];
            const double mean_dr = block_sum(sdr, red) / ntr;
            double sv = 0.0;
            for (int i = t; i < ntr; i += NT) { const double d = trx[i] - old[i] - mean_dr; sv += d * d; }
            sv = block_sum(sv, red) / ntr;
            if (t == 0) {
                if (a.v_eff) a.v_eff[row] = mean_dr / (a.p.window * dt);
                if (a.D_eff) a.D_eff[row] = sv / (2 * a.p.window * dt);
            }
        } else if (t == 0) {
            const double nan = __longlong_as_double(0x7ff8000000000000ll);
            if (a.v_eff) a.v_eff[row] = nan;
            if (a.D_eff) a.D_eff[row] = nan;
        }
    }
}

struct Plan { int G, q, r, ktaps, launches; size_t lds; long long work_bytes; int spectral, conv_m, conv_B, conv_S; };

// PDE_SPECTRAL_MAX_LOG2 of the environment bounds the transform of the spectral convolution (default and most: 21)
int spectral_cap() {
    const char *e = std::getenv("PDE_SPECTRAL_MAX_LOG2");
    return e && *e ? std::atoi(e) : PDES_MAX_LOG2;
}

// the checks and choices shared by pdew_plan and pdew_solve; nullptr or the complaint
const char *make_plan(const pde_params *p, int32_t n_systems, int32_t workgroups, int ktaps, Plan &pl) {
    if (n_systems > 65535) return "n_systems must be <= 65535";
    if (p->convolution != 0 && p->convolution != 1) return "convolution must be 0 (direct) or 1 (spectral)";
    if (workgroups < 0) return "workgroups must be >= 1 (or 0: chosen by the library)";
    int G = workgroups;
    if (G == 0) {
        G = (p->L + PDEW_AUTO_SLAB - 1) / PDEW_AUTO_SLAB;
        G = std::max(1, std::min(G, std::min(PDEW_MAX_WORKGROUPS, PDEW_MAX_GRID / n_systems)));
    }
    if (G > PDEW_MAX_WORKGROUPS) return "workgroups must be <= PDEW_MAX_WORKGROUPS";
    if (p->L / G < PDEW_MIN_SLAB) return "too many workgroups: the shortest slab, floor(L / workgroups), must have at least PDEW_MIN_SLAB sites";
    if ((long long)G * n_systems > PDEW_MAX_GRID) return "workgroups * n_systems must be <= PDEW_MAX_GRID";
    pl.G = G; pl.q = p->L / G; pl.r = p->L % G; pl.ktaps = ktaps;
    pl.launches = 6 + (p->n_tracers > 0 ? 1 : 0);
    pl.lds = 0;
    if (p->kernel_mode == 1)
        for (int n : {pl.q, pl.q + (pl.r ? 1 : 0)})
            for (int nsub : {std::min(n, SUB), n % SUB})
                if (nsub > 0) pl.lds = std::max(pl.lds, conv_lds_doubles(conv_shape(nsub, ktaps)) * sizeof(double));
    const long long S = n_systems, L = p->L, ntr = p->n_tracers;
    pl.work_bytes = 8 * (5 * S * L + S * NSLOT * G + S * 2 * p->n_fft_modes * G + 2 * S * G * 3 + 4 * S + S * p->window * ntr + S * ntr) + S * ntr;
    pl.spectral = p->kernel_mode == 1 && p->convolution == 1 && ktaps > 0;   // a kernel of one tap is its direct sum: nothing to transform
    pl.conv_m = pl.conv_B = pl.conv_S = 0;
    if (pl.spectral) {                                         // no fall-back: a shape the transforms cannot take is refused
        if (const char *why = pdes_plan_blocks(L, ktaps, spectral_cap(), pl.conv_B, pl.conv_m, pl.conv_S)) return why;
        if ((long long)pl.conv_B * n_systems > 65535) return "spectral convolution: blocks * n_systems must be <= 65535";
        const long long M = 1ll << pl.conv_m;
        pl.launches += pdes_launches(pl.conv_m);
        pl.lds = PDES_LDS_BYTES;
        pl.work_bytes += 16 * S * pl.conv_B * M + 8 * M + 16 * (64 + std::max(M >> 10, 1ll) + 1024);   // windows, spectrum, tables
    }
    return nullptr;
}

int wide_entry(const char *who, std::string &err, const pde_params *p, int32_t n_systems, int32_t workgroups, PdeIo io);

}  // namespace

extern "C" {

const char *pdew_last_error(void) { return g_err.c_str(); }
const char *pdes_last_error(void) { return g_spec_err.c_str(); }

int pdes_plan(int32_t L, int32_t ktaps, int32_t max_log2, int32_t *blocks, int32_t *log2_m, int32_t *block_sites) {
    auto bad = [&](const char *m) { g_spec_err = std::string("pdes_plan: ") + m; return PDE_ERR_ARG; };
    if (!blocks || !log2_m || !block_sites) return bad("null argument");
    int B, m, S;
    if (const char *why = pdes_plan_blocks(L, ktaps, max_log2, B, m, S)) return bad(why);
    *blocks = B; *log2_m = m; *block_sites = S;
    return PDE_OK;
}

int pdew_plan(const pde_params *p, int32_t n_systems, int32_t workgroups, pdew_plan_info *out) {
    auto bad = [&](const char *m) { g_err = std::string("pdew_plan: ") + m; return PDE_ERR_ARG; };
    if (!p || !out || n_systems < 1) return bad("null argument or n_systems < 1");
    if (p->L < 4 || p->L > PDE_MAX_L) return bad("L must be in [4, PDE_MAX_L]");
    if (p->kernel_mode < 0 || p->kernel_mode > 2) return bad("kernel_mode must be 0, 1 or 2");
    if (!(p->xlim > 0.0) || p->n_tracers < 0 || p->n_fft_modes < 0 || p->window < 0) return bad("xlim > 0, n_tracers >= 0, n_fft_modes >= 0, window >= 0 required");
    std::vector<double> ktab;
    const int ktaps = kernel_taps(p, p->xlim / p->L, ktab);
    Plan pl;
    if (const char *why = make_plan(p, n_systems, workgroups, ktaps, pl)) return bad(why);
    std::memset(out, 0, sizeof *out);
    out->workgroups = pl.G; out->slab_len = pl.q + (pl.r ? 1 : 0); out->slab_len_min = pl.q; out->n_long_slabs = pl.r;
    out->ktaps = pl.ktaps; out->launches_per_step = pl.launches; out->lds_bytes = (int32_t)pl.lds; out->work_bytes = pl.work_bytes;
    out->conv_log2 = pl.conv_m;
    return PDE_OK;
}

int pdew_solve(const pde_params *p, int32_t n_systems, int32_t workgroups, const double *beta, const double *rho_p0,
               const double *rho_m0, const double *tracer_x0, const int8_t *tracer_s0, const double *rand_u, const double *rand_n,
               double *rho_p, double *rho_m, double *m_series, double *var_series, double *v_eff_series,
               double *D_eff_series, double *snapshots, double *m_snapshots, double *fft_re, double *fft_im,
               double *tracer_x, int8_t *tracer_s, double *kernel_ms) {
    const PdeIo io{beta, rho_p0, rho_m0, tracer_x0, tracer_s0, rand_u, rand_n, rho_p, rho_m, m_series, var_series, v_eff_series,
                   D_eff_series, snapshots, m_snapshots, fft_re, fft_im, tracer_x, tracer_s, kernel_ms};
    return wide_entry("pdew_solve", g_err, p, n_systems, workgroups, io);
}

const char *pdewr_last_error(void) { return g_err_r.c_str(); }

int pdewr_solve(const pde_params *p, int32_t n_systems, int32_t workgroups, const double *beta, const double *rho_p0,
                const double *rho_m0, const double *tracer_x0, const int8_t *tracer_s0, const double *rand_u, const double *rand_n,
                double *rho_p, double *rho_m, double *m_series, double *var_series, double *v_eff_series,
                double *D_eff_series, double *snapshots, double *m_snapshots, double *fft_re, double *fft_im,
                double *tracer_x, int8_t *tracer_s, double *kernel_ms, const pde_checkpoint *from, pde_checkpoint *to) {
    const PdeIo io{beta, rho_p0, rho_m0, tracer_x0, tracer_s0, rand_u, rand_n, rho_p, rho_m, m_series, var_series, v_eff_series,
                   D_eff_series, snapshots, m_snapshots, fft_re, fft_im, tracer_x, tracer_s, kernel_ms, from, to};
    return wide_entry("pdewr_solve", g_err_r, p, n_systems, workgroups, io);
}

}  // extern "C"

namespace {

// The checks and the launches behind pdew_solve and pdewr_solve, worded by the entry's name.
int wide_entry(const char *who, std::string &g_err, const pde_params *p, int32_t n_systems, int32_t workgroups, PdeIo io) {
    auto bad = [&](const char *m) { g_err = std::string(who) + ": " + m; return PDE_ERR_ARG; };
    PdeSpan span;
    if (const char *why = adopt_checkpoint(p, io, span)) return bad(why);
    if (const char *why = check_args(p, n_systems, io)) return bad(why);
    const int L = p->L, ntr = p->n_tracers;
    std::vector<double> ktab;
    const int ktaps = kernel_taps(p, p->xlim / L, ktab);
    Plan pl;
    if (const char *why = make_plan(p, n_systems, workgroups, ktaps, pl)) return bad(why);
    OneShot job{who, g_err, false, PDE_ERR_NODEVICE, PDE_ERR_ARG, PDE_ERR_HIP};   // no zero-fill: the kernels write every buffer before it is read
    if (int rc = job.select_device(p->device)) return rc;

    const PdeExtents x(p, n_systems, span);
    const size_t S = x.S, SL = x.SL;
    const int G = pl.G;
    WArgs a{};
    a.G = pl.G; a.q = pl.q; a.r = pl.r;
    if (int rc = pde_stage_inputs(job, a, p, x, io, ktaps, ktab)) return rc;   // the factorisation, taps and twiddles pde_solve_batch uses
    WORK(rp, SL); WORK(rm, SL); WORK(xp, SL); WORK(xm, SL); WORK(mf, SL);
    WORK(part, S * NSLOT * G); WORK(fmap, S * G * 3); WORK(bmap, S * G * 3); WORK(corner, S * 4);
    if (io.fft_re) WORK(fpart, S * 2 * (size_t)p->n_fft_modes * G);
    a.spectral = pl.spectral;
    double2 *taps_dev = nullptr;
    double *spec_dev = nullptr;
    if (pl.spectral) {
        SpecTables tab;
        pdes_build_tables(pl.conv_m, ktaps, ktab, tab);
        const size_t M = (size_t)1 << pl.conv_m;
        a.sp.m = pl.conv_m; pdes_split(pl.conv_m, a.sp.a1, a.sp.a2);
        a.sp.L = L; a.sp.kt = ktaps; a.sp.S = pl.conv_S; a.sp.B = pl.conv_B;
        UP(sp.w128, tab.w128.data(), tab.w128.size()); UP(sp.thi, tab.hi.data(), tab.hi.size()); UP(sp.tlo, tab.lo.data(), tab.lo.size());
        WORK(sp.data, S * pl.conv_B * M);
        if (int rc = job.upload(&taps_dev, tab.taps.data(), M, "taps")) return rc;
        if (int rc = job.alloc(&spec_dev, M, "spec")) return rc;
        a.sp.spec = spec_dev; a.sp.rp = a.rp; a.sp.rm = a.rm; a.sp.mf = a.mf;
    }
    const bool tracer_series = ntr > 0;                        // v_eff / D_eff only with tracers: no kernel here writes them otherwise
    if (int rc = pde_stage_outputs(job, a, p, x, io, tracer_series)) return rc;
    const size_t mag_lds = pl.spectral ? 0 : pl.lds;            // (spectral: pl.lds is the transforms' static LDS)
    if (int rc = job.raise_lds_limit(reinterpret_cast<const void *>(&pdew_mag), mag_lds)) return rc;
    if (int rc = job.create_events()) return rc;
    // the whole run is one chain of launches on the null stream: nothing here waits for the device until the end
    const dim3 grid((unsigned)G, (unsigned)n_systems), one(1, (unsigned)n_systems), tgrid((unsigned)((ntr + NT - 1) / NT), (unsigned)n_systems);
    const bool want_obs = a.m_series || a.var_series || a.fft_re || a.v_eff || a.D_eff;
    const unsigned nz = (unsigned)(n_systems * std::max(pl.conv_B, 1));
    if (pl.spectral) {                                         // once per solve: the taps' spectrum by the device's own forward sweeps
        SpecPlan one_block = a.sp;
        one_block.B = 1; one_block.data = taps_dev;
        pdes_build_spectrum(one_block, spec_dev);
    }
    job.ev.start();
    hipLaunchKernelGGL(pdew_renorm_fwd, grid, dim3(NT), 0, nullptr, a, 1);
    hipError_t err = hipGetLastError();
    for (int n = span.n_begin; err == hipSuccess; ++n) {        // absolute step numbers; the kernels make the rows launch-relative
        const bool record = n >= span.row0;                        // a resumed launch starts behind the row of its checkpoint's step
        if (pl.spectral) pdes_convolve(a.sp, nz);
        hipLaunchKernelGGL(pdew_mag, grid, dim3(NT), mag_lds, nullptr, a, n);
        if (ntr && record) hipLaunchKernelGGL(pdew_tracers, tgrid, dim3(NT), 0, nullptr, a, n);
        if (want_obs && record) hipLaunchKernelGGL(pdew_obs, one, dim3(NT), 0, nullptr, a, n);
        if (n < span.n_end) {
            hipLaunchKernelGGL(pdew_fwd_bwd, grid, dim3(NT), 0, nullptr, a);
            hipLaunchKernelGGL(pdew_bwd, grid, dim3(NT), 0, nullptr, a);
            hipLaunchKernelGGL(pdew_react, grid, dim3(NT), 0, nullptr, a);
            hipLaunchKernelGGL(pdew_renorm_fwd, grid, dim3(NT), 0, nullptr, a, 0);
        }
        err = hipGetLastError();
        if (n == span.n_end) break;
    }
    job.ev.stop();
    if (int rc = job.finish(err, who, io.kernel_ms)) return rc;
    DOWN(io.rho_p, rp, SL * 8); DOWN(io.rho_m, rm, SL * 8);         // the fields end in their work buffers
    if (int rc = pde_fetch_outputs(job, a, p, x, io, tracer_series)) return rc;
    if (ntr) { DOWN(io.tracer_x, trx, x.ST * 8); DOWN(io.tracer_s, trs, x.ST); }   // and the tracers in theirs
    return pde_fetch_checkpoint(job, a, p, x, io, a.rp, a.rm);
}

}  // namespace
