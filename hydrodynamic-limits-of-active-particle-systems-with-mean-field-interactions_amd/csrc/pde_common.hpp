// pde_common.hpp -- what the two execution shapes of the hydrodynamic-limit solver share: pde_hip.hip (one workgroup per
// system, include/pde.h) and pde_wide_hip.hip (one system over many workgroups, include/pde_wide.h).
//
// Host side: the call record of the solves and its checks, the Thomas factorisation of the constant diffusion matrix with its
// Sherman-Morrison vector, the normalised kernel taps, the Fourier twiddles, the staging both shapes share.  Device side: the
// Curie-Weiss rate, Philox4x32-10, the workgroup sum and the workgroup scan of affine maps.  One copy, so both shapes solve
// with the same numbers.
#pragma once

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "pde.h"
#include "pde_resume.h"
#include "dev_mem.hpp"                    // OneShot and the UP / WORK / OUT / DOWN of the staging

namespace pde_common {

constexpr int NT = 256;                 // threads per workgroup = chunks of the recurrences

// ---------------------------------------------------------------------------------------------------------------- host

// The call record: the seven inputs, twelve outputs (null: not wanted) and kernel time every solve of include/pde.h takes
struct PdeIo {
    const double *beta, *rho_p0, *rho_m0, *tracer_x0; const int8_t *tracer_s0; const double *rand_u, *rand_n;
    double *rho_p, *rho_m, *m_series, *var_series, *v_eff_series, *D_eff_series, *snapshots, *m_snapshots, *fft_re, *fft_im, *tracer_x;
    int8_t *tracer_s; double *kernel_ms;
    const pde_checkpoint *from; pde_checkpoint *to;   // the resumable entry points (include/pde_resume.h); null: a fresh start, no checkpoint left
};

// The steps and rows of one launch (include/pde_resume.h): the loop runs n = n_begin .. n_end in absolute step numbers and
// records rows row0 .. n_end, n_rows of them, at launch-relative offsets; snap0 is the run's number of the launch's first
// snapshot.  A fresh start is 0 .. nsteps, a resumed one (resume = 1) skips the recording part of iteration n_begin.
struct PdeSpan { int n_begin, n_end, row0, n_rows, snap0, n_snap, resume; };

// nullptr, or why no launch has these rows
inline const char *pde_span(const pde_params *p, int32_t from_step, PdeSpan &sp) {
    if (from_step < -1) return "from->step must be >= 0";
    if (from_step >= 0 && p->nsteps < 1) return "a resumed launch needs nsteps >= 1";
    if (p->nsteps < 0) return "nsteps >= 0 required";
    if (p->snapshot_interval < 1) return "snapshot_interval must be >= 1";
    if (from_step >= 0 && (long long)from_step + p->nsteps > INT32_MAX) return "from->step + nsteps exceeds INT32_MAX";
    const int every = p->snapshot_interval;
    sp.resume = from_step >= 0;
    sp.n_begin = sp.resume ? from_step : 0;
    sp.n_end = sp.n_begin + p->nsteps;
    sp.row0 = sp.resume ? from_step + 1 : 0;
    sp.n_rows = sp.n_end - sp.row0 + 1;
    sp.snap0 = sp.resume ? from_step / every + 1 : 0;
    sp.n_snap = sp.n_end / every - sp.snap0 + 1;
    return nullptr;
}

// The checks of `from` and `to`; a resumed launch then starts from the checkpoint's arrays in place of the initial state.
// nullptr, or the text of the complaint.
inline const char *adopt_checkpoint(const pde_params *p, PdeIo &io, PdeSpan &sp) {
    if (!p) return "null argument or n_systems < 1";
    if (io.from && io.from->step < 0) return "from->step must be >= 0";
    if (const char *why = pde_span(p, io.from ? io.from->step : -1, sp)) { if (io.from) return why; sp = PdeSpan{}; }   // a fresh start's own faults are check_args'
    for (const pde_checkpoint *c : {io.from, (const pde_checkpoint *)io.to}) {
        if (!c) continue;
        if (!c->rho_p || !c->rho_m) return c == io.from ? "from: rho_p and rho_m are required" : "to: rho_p and rho_m are required";
        if (p->n_tracers > 0 && (!c->tracer_x || !c->tracer_s || !c->hist))
            return c == io.from ? "from: tracer_x, tracer_s and hist are required with n_tracers > 0" : "to: tracer_x, tracer_s and hist are required with n_tracers > 0";
    }
    if (io.from) { io.rho_p0 = io.from->rho_p; io.rho_m0 = io.from->rho_m; io.tracer_x0 = io.from->tracer_x; io.tracer_s0 = io.from->tracer_s; }
    if (sp.n_snap == 0) io.snapshots = io.m_snapshots = nullptr;   // no snapshot row in this launch: the pointers are ignored
    return nullptr;
}

// nullptr when the arguments of a solve are acceptable, else the text of the complaint
inline const char *check_args(const pde_params *p, int32_t n_systems, const PdeIo &io) {
    if (!p || !io.beta || !io.rho_p0 || !io.rho_m0 || n_systems < 1) return "null argument or n_systems < 1";
    if (p->L < 4 || p->L > PDE_MAX_L) return "L must be in [4, PDE_MAX_L]";
    if (p->nsteps < 0 || !(p->dt > 0.0) || !(p->xlim > 0.0)) return "nsteps >= 0, dt > 0, xlim > 0 required";
    if (p->snapshot_interval < 1) return "snapshot_interval must be >= 1";
    if (p->kernel_mode < 0 || p->kernel_mode > 2) return "kernel_mode must be 0, 1 or 2";
    if (p->n_tracers < 0 || (p->n_tracers > 0 && (!io.tracer_x0 || !io.tracer_s0 || p->window < 1))) return "tracers need initial positions, states and window >= 1";
    if ((io.rand_u == nullptr) != (io.rand_n == nullptr)) return "rand_u and rand_n come together";
    if (p->n_fft_modes < 0 || p->n_fft_modes > p->L / 2 + 1 || ((io.fft_re == nullptr) != (io.fft_im == nullptr))) return "bad fft request";
    return nullptr;
}

struct PdeExtents {        // systems, and systems times sites, recorded rows, tracers; snapshots per system; the launch's span
    size_t S, SL, SN, ST; int n_snap; PdeSpan sp;
    PdeExtents(const pde_params *p, int32_t n, const PdeSpan &span)
        : S((size_t)n), SL(S * p->L), SN(S * span.n_rows), ST(S * p->n_tracers), n_snap(span.n_snap), sp(span) {}
};

struct Factor {            // (I - gamma dt Lap / dx^2) = L U, and the Sherman-Morrison data of the periodic corners
    std::vector<double> up, fw, finv, fz;     // upper diagonal, multipliers, 1/pivots, S-M vector z   [L]
    double sm_coef = 0.0, sm_denom = 1.0;     // x = y - z * (y_0 + sm_coef y_{L-1}) / sm_denom
};

inline void factorise(const pde_params *p, double dx, Factor &f) {
    const int L = p->L;
    const double av = p->gamma * p->dt / (dx * dx), bv = 1.0 + 2.0 * av;
    std::vector<double> lo(L, -av), di(L, bv);
    f.up.assign(L, -av); f.fw.assign(L, 0.0); f.finv.assign(L, 0.0); f.fz.assign(L, 0.0);
    std::vector<double> &up = f.up, &fw = f.fw, &finv = f.finv, &fz = f.fz;
    lo[0] = 0.0; up[L - 1] = 0.0;
    double sm_coef = 0.0, sm_denom = 1.0;
    if (!p->periodic) { up[0] = -2.0 * av; lo[L - 1] = -2.0 * av; }
    else {
        const double corner = -av, gam = -bv;
        di[0] = bv - gam; di[L - 1] = bv - corner * corner / gam;
        sm_coef = corner / gam;
    }
    std::vector<double> piv(L);
    piv[0] = di[0];
    for (int i = 1; i < L; ++i) { fw[i] = lo[i] / piv[i - 1]; piv[i] = di[i] - fw[i] * up[i - 1]; }
    for (int i = 0; i < L; ++i) finv[i] = 1.0 / piv[i];
    if (p->periodic) {                                         // A' z = u,  u = (gam, 0, ..., 0, corner)
        const double corner = -av, gam = -bv;
        std::vector<double> y(L, 0.0);
        y[0] = gam; y[L - 1] = corner;
        for (int i = 1; i < L; ++i) y[i] -= fw[i] * y[i - 1];
        fz[L - 1] = y[L - 1] * finv[L - 1];
        for (int i = L - 2; i >= 0; --i) fz[i] = (y[i] - up[i] * fz[i + 1]) * finv[i];
        sm_denom = 1.0 + fz[0] + sm_coef * fz[L - 1];
    }
    f.sm_coef = sm_coef; f.sm_denom = sm_denom;
}

// kernel taps (ref :84-93), normalised over the whole ring, cut where negligible; returns ktaps, ktab[0..ktaps]
inline int kernel_taps(const pde_params *p, double dx, std::vector<double> &ktab) {
    const int L = p->L;
    ktab.assign(1, 1.0);
    int ktaps = 0;
    if (p->kernel_mode == 1) {
        std::vector<double> full(L);
        double sum = 0.0;
        for (int i = 0; i < L; ++i) { const double d = std::min(i, L - i) * dx / p->kernel_sigma; full[i] = std::exp(-0.5 * d * d); sum += full[i]; }
        ktaps = 0;
        for (int i = 0; i <= L / 2; ++i) if (full[i] >= 1e-17 * full[0]) ktaps = i;
        ktab.assign(ktaps + 1, 0.0);
        for (int i = 0; i <= ktaps; ++i) ktab[i] = full[i] / sum;
        if (L % 2 == 0 && ktaps == L / 2) ktab[ktaps] *= 0.5;  // the antipodal site is met from both sides of the sweep
    }
    return ktaps;
}

inline void twiddles(int L, std::vector<double> &twc, std::vector<double> &tws) {
    twc.resize(L); tws.resize(L);
    for (int j = 0; j < L; ++j) { const double ang = 6.283185307179586476925 * (double)j / (double)L; twc[j] = std::cos(ang); tws[j] = std::sin(ang); }
}

// The staging both shapes share, into the driver's argument struct `a` (PdeArgs, WArgs: the same member names), in two halves:
// a shape allocates its own work memory between them.  First what the kernels read; `ktab` are the taps, reaching `ktaps` sites.
template <class Args>
int pde_stage_inputs(OneShot &job, Args &a, const pde_params *p, const PdeExtents &x, const PdeIo &io, int ktaps, const std::vector<double> &ktab) {
    const size_t L = (size_t)p->L;
    a.p = *p; a.dx = p->xlim / p->L; a.ktaps = ktaps; a.n_snap = x.n_snap; a.span = x.sp;
    Factor fac;
    factorise(p, a.dx, fac);
    a.sm_coef = fac.sm_coef; a.sm_denom = fac.sm_denom;
    std::vector<double> twc, tws;
    twiddles(p->L, twc, tws);
    UP(beta, io.beta, x.S); UP(rho_p0, io.rho_p0, x.SL); UP(rho_m0, io.rho_m0, x.SL);
    UP(fw, fac.fw.data(), L); UP(finv, fac.finv.data(), L); UP(fu, fac.up.data(), L); UP(fz, fac.fz.data(), L);
    UP(ktab, ktab.data(), ktab.size()); UP(twc, twc.data(), L); UP(tws, tws.data(), L);
    return 0;
}

// Then the tracer block and the series, snapshot and Fourier outputs the caller asked for (tracer_series: v_eff / D_eff among
// them).  The final fields and tracers are each shape's own.
template <class Args>
int pde_stage_outputs(OneShot &job, Args &a, const pde_params *p, const PdeExtents &x, const PdeIo &io, bool tracer_series) {
    const size_t L = (size_t)p->L, ntr = (size_t)p->n_tracers;
    if (ntr) {
        UP(tracer_x0, io.tracer_x0, x.ST); UP(tracer_s0, io.tracer_s0, x.ST);
        if (io.rand_u) { UP(rand_u, io.rand_u, x.SN * ntr); UP(rand_n, io.rand_n, x.SN * ntr); }
        if (io.from) UP(hist, io.from->hist, x.S * p->window * ntr); else WORK(hist, x.S * p->window * ntr);   // the ring goes on from the checkpoint's
        WORK(trx, x.ST); WORK(trs, x.ST);
    }
    OUT(m_series, io.m_series, x.SN); OUT(var_series, io.var_series, x.SN);
    if (tracer_series) { OUT(v_eff, io.v_eff_series, x.SN); OUT(D_eff, io.D_eff_series, x.SN); }
    OUT(snapshots, io.snapshots, x.S * x.n_snap * L); OUT(m_snapshots, io.m_snapshots, x.S * x.n_snap * L);
    OUT(fft_re, io.fft_re, x.SN * p->n_fft_modes); OUT(fft_im, io.fft_im, x.SN * p->n_fft_modes);
    return 0;
}

template <class Args>                                          // the outputs of pde_stage_outputs, back to the caller
int pde_fetch_outputs(OneShot &job, const Args &a, const pde_params *p, const PdeExtents &x, const PdeIo &io, bool tracer_series) {
    DOWN(io.m_series, m_series, x.SN * 8); DOWN(io.var_series, var_series, x.SN * 8);
    if (tracer_series) { DOWN(io.v_eff_series, v_eff, x.SN * 8); DOWN(io.D_eff_series, D_eff, x.SN * 8); }
    DOWN(io.snapshots, snapshots, x.S * x.n_snap * p->L * 8); DOWN(io.m_snapshots, m_snapshots, x.S * x.n_snap * p->L * 8);
    DOWN(io.fft_re, fft_re, x.SN * p->n_fft_modes * 8); DOWN(io.fft_im, fft_im, x.SN * p->n_fft_modes * 8);
    return 0;
}

// The checkpoint at the launch's last row, from where the shape keeps its final state on the device (fields, working tracers).
template <class Args>
int pde_fetch_checkpoint(OneShot &job, const Args &a, const pde_params *p, const PdeExtents &x, const PdeIo &io,
                         const double *rp, const double *rm) {
    pde_checkpoint *to = io.to;
    if (!to) return 0;
    if (int rc = job.download(to->rho_p, rp, x.SL * 8, "checkpoint rho_p")) return rc;
    if (int rc = job.download(to->rho_m, rm, x.SL * 8, "checkpoint rho_m")) return rc;
    if (p->n_tracers > 0) {
        const size_t ntr = (size_t)p->n_tracers, win = (size_t)p->window;
        if (int rc = job.download(to->tracer_x, a.trx, x.ST * 8, "checkpoint tracer_x")) return rc;
        if (int rc = job.download(to->tracer_s, a.trs, x.ST, "checkpoint tracer_s")) return rc;
        if (int rc = job.download(to->hist, a.hist, x.S * win * ntr * 8, "checkpoint hist")) return rc;
        for (size_t s = 0; s < x.S; ++s)                          // the slots no row has filled yet are written as 0
            for (size_t slot = (size_t)x.sp.n_end + 1; slot < win; ++slot) std::fill_n(to->hist + (s * win + slot) * ntr, ntr, 0.0);
    }
    to->step = x.sp.n_end;
    return 0;
}

// -------------------------------------------------------------------------------------------------------------- device

__device__ inline double cw_rate(double beta, double sigma, double m) {      // ref :64-66
    const double r = exp(-beta * sigma * m);
    return r < 1e-8 ? 1e-8 : (r > 1e8 ? 1e8 : r);
}

// Philox4x32-10 (Random123), as in the particle stepper
__device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0; c1 = l1; c2 = n2; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the tracer's uniform and normal number of step n, tracer i, system sys: counter (n, i, sys, 0x7AC3), key = seed
__device__ inline void tracer_noise(uint64_t seed, int n, int i, int sys, double &u, double &g) {
    uint32_t x[4];
    philox4x32_10((uint32_t)n, (uint32_t)i, (uint32_t)sys, 0x7AC3u, (uint32_t)seed, (uint32_t)(seed >> 32), x);
    u = ((double)(x[0] >> 5) * 67108864.0 + (double)(x[1] >> 6)) * 0x1.0p-53;
    const double u1 = ((double)x[2] + 0.5) * 0x1.0p-32, u2 = ((double)x[3] + 0.5) * 0x1.0p-32;
    g = sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925 * u2);
}

// sum over the workgroup; every thread gets the result.  `red` = NT doubles of LDS scratch.
__device__ inline double block_sum(double v, double *red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();                                          // scratch may still be read from the previous call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) s += red[w];
    return s;
}

// Scan of 2 x NT affine maps x -> A x + B (two fields at once) in LDS, Hillis-Steele.  Logical order: thread t is element t
// (forward) or NT-1-t (backward).  Returns the buffer that holds the INCLUSIVE compositions by logical index: [j - 1] is the
// composition of all maps before logical element j, [NT - 1] that of all NT maps.  `buf` = 2 * NT double4.
__device__ inline const double4 *scan_affine2_all(double A0, double B0, double A1, double B1, double4 *buf, bool backward) {
    const int j = backward ? NT - 1 - (int)threadIdx.x : (int)threadIdx.x;
    double4 *cur = buf, *nxt = buf + NT;
    __syncthreads();
    cur[j] = make_double4(A0, B0, A1, B1);
    __syncthreads();
    for (int off = 1; off < NT; off <<= 1) {
        double4 me = cur[j];
        if (j >= off) {                                       // me after prev:  x -> me.A (prev.A x + prev.B) + me.B
            const double4 pv = cur[j - off];
            me = make_double4(me.x * pv.x, me.x * pv.y + me.y, me.z * pv.z, me.z * pv.w + me.w);
        }
        nxt[j] = me;
        __syncthreads();
        double4 *sw = cur; cur = nxt; nxt = sw;
    }
    return cur;
}

// Exclusive form for a sweep that starts from 0: the value entering this thread's chunk.
__device__ inline void scan_affine2(double A0, double B0, double A1, double B1, double4 *buf, bool backward, double &in0, double &in1) {
    const int j = backward ? NT - 1 - (int)threadIdx.x : (int)threadIdx.x;
    const double4 *cur = scan_affine2_all(A0, B0, A1, B1, buf, backward);
    if (j == 0) { in0 = 0.0; in1 = 0.0; }
    else { const double4 pv = cur[j - 1]; in0 = pv.y; in1 = pv.w; }
}

}  // namespace pde_common
