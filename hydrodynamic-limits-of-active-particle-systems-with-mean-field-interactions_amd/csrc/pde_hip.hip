// pde_hip.hip -- MI355X (gfx950) implementation of the C ABIs in include/pde.h and include/pde_sweep.h, and of their resumable
// forms pder_solve / pdekr_solve in include/pde_resume.h (the same kernel; a resumed launch runs its RESUMED instantiation, whose loop
// starts at a given absolute step).
//
// Replaces the time loop of the reference's IMEXPDE (IMEX_PDE_solver_class.py:236-290): one PERSISTENT workgroup
// per system keeps rho_plus, rho_minus, the diffused fields and the magnetisation in LDS and runs all nsteps
// without leaving the kernel (a step is ~10 phases separated by workgroup barriers; nothing but the requested
// series is written to HBM).  Systems of a batch differ only in beta (pde_solve_batch; the reference's sweep parameter), or in
// beta and in the width of the Gaussian kernel (pdek_solve: the same kernel and host driver, mode, reach and taps per system).
//
//   implicit diffusion  (I - gamma dt Lap / dx^2) x = rho          ref :68-82, :192-193
//       constant matrix -> Thomas factorisation once on the host; the two triangular sweeps are first-order linear
//       recurrences y_i = a_i y_{i-1} + b_i, evaluated as a workgroup-wide scan of affine maps (chunk per thread,
//       Hillis-Steele over the 256 chunk maps in LDS); periodic corners by Sherman-Morrison
//   magnetisation       local ratio | circular Gaussian convolution | global mean      ref :156-168
//       the reference multiplies rfft's; here the periodic kernel (same normalised taps, cut where they fall below
//       1e-17 of the centre tap) is applied directly with a sliding 4-site register window; pdek_solve with convolution = 1
//       multiplies complex transforms held in LDS instead (pde_sweep_fft.hpp)
//   reaction/advection/clip/renormalise                                                   ref :195-233
//   observables per step: mean m, var(total), lowest rfft modes (direct DFT), snapshots   ref :243-255
//   tracers: Euler-Maruyama flip + drift + noise, windowed v_eff / D_eff                  ref :257-287
//
// Arithmetic: binary64.  Not bit-identical to the reference (different linear solver, summation orders and libm).  Two yardsticks:
// oracle/pde_numpy.py, which IS bit-identical to the reference (tests/test_gpu_pde*.py: 1e-11 of a field's scale at the drivers'
// parameters), and the scheme in extended precision (tests/pde_reference.py; tests/test_gpu_pde_random.py: max(1e-11, twice the
// oracle's own deviation) over random parameters).  On near-vacuum states the second is the better one: the oracle's rfft
// round-off is divided by den + 1e-12 on empty sites, the direct sum here has relative errors only.

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pde.h"
#include "pde_sweep.h"
#include "pde_common.hpp"                 // factorisation, taps, rate, Philox, workgroup sum and scan: shared with pde_wide_hip.hip
#include "dev_mem.hpp"                    // buffer owner, event pair, the driver of the one-shot entry points
#include "pde_sweep_fft.hpp"              // the transform in LDS of the kernel-width sweep (include/pde_sweep.h)

namespace {

using namespace pde_common;
std::string g_err, g_err_k, g_err_r, g_err_kr;

// The three forms of the kernel.  BATCH is pde_solve_batch: one kernel mode and one table of taps for the launch.  The two sweep
// forms (pdek_solve) read mode, reach and taps per system; SWEEP_SPECTRAL evaluates mode 1 by the transform of pde_sweep_fft.hpp.
enum Form { BATCH, SWEEP_DIRECT, SWEEP_SPECTRAL };
static_assert(pdek::THREADS == NT, "pde_sweep_fft.hpp strides its passes by the workgroup of pde_kernel");

struct PdeArgs {
    pde_params p;
    int n_snap, ktaps, chunk;           // chunk = sites per thread in the scans; ktaps: of the launch (sweep: the largest), sizes the LDS layout
    double dx, sm_coef, sm_denom;       // Sherman-Morrison: x = y - z * (y_0 + sm_coef y_{L-1}) / sm_denom
    const double *beta, *rho_p0, *rho_m0, *tracer_x0;
    const int8_t *tracer_s0;
    const double *rand_u, *rand_n;
    const double *fw, *finv, *fu, *fz;  // factorisation: multipliers, 1/pivots, upper diagonal, S-M vector z   [L]
    const double *ktab;                 // [ktaps + 1] normalised kernel taps by distance
    const double *twc, *tws;            // [L] cos / sin(2 pi j / L)
    double *rho_p, *rho_m, *m_series, *var_series, *v_eff, *D_eff, *snapshots, *m_snapshots, *fft_re, *fft_im, *tracer_x;
    int8_t *tracer_s;
    double *work;                       // systems beyond LDS: [n_systems][work_stride] fields + kernel taps in global memory (else null)
    long long work_stride;
    double *hist;                       // [n_systems][window][n_tracers] ring of unwrapped tracer positions
    double *trx; int8_t *trs;           // [n_systems][n_tracers] working tracer state
    // the sweep forms only (null for BATCH): per system [n_systems]
    const int *sys_mode, *sys_ktaps, *sys_log2;   // kernel mode, reach, log2 of the transform (0: none)
    const long long *sys_ktab;                    // where the system's taps begin in ktab
    const double2 *ctw;                           // twiddles of m = PDEK_MIN_LOG2 .., one table after another
    PdeSpan span;                       // the absolute steps this launch runs and the rows it records (pde_common.hpp); read by the RESUMED kernels only
};

// x = A^{-1} d for both fields: d in (dp, dm), result overwrites them.
__device__ inline void diffuse2(const PdeArgs &a, double *dp, double *dm, double4 *scan, double *red) {
    const int L = a.p.L, t = threadIdx.x, c0 = t * a.chunk, c1 = min(L, c0 + a.chunk);
    // forward: y_i = d_i - w_i y_{i-1}
    double A = 1.0, Bp = 0.0, Bm = 0.0;
    for (int i = c0; i < c1; ++i) { const double w = a.fw[i]; Bp = dp[i] - w * Bp; Bm = dm[i] - w * Bm; A = -w * A; }
    double yp, ym;
    scan_affine2(A, Bp, A, Bm, scan, false, yp, ym);
    for (int i = c0; i < c1; ++i) { const double w = a.fw[i]; yp = dp[i] - w * yp; ym = dm[i] - w * ym; dp[i] = yp; dm[i] = ym; }
    // backward: x_i = inv_i y_i - (u_i inv_i) x_{i+1}
    A = 1.0; Bp = 0.0; Bm = 0.0;
    for (int i = c1 - 1; i >= c0; --i) { const double iv = a.finv[i], q = -a.fu[i] * iv; Bp = dp[i] * iv + q * Bp; Bm = dm[i] * iv + q * Bm; A = q * A; }
    double xp, xm;
    scan_affine2(A, Bp, A, Bm, scan, true, xp, xm);
    __syncthreads();
    for (int i = c1 - 1; i >= c0; --i) { const double iv = a.finv[i], q = -a.fu[i] * iv; xp = dp[i] * iv + q * xp; xm = dm[i] * iv + q * xm; dp[i] = xp; dm[i] = xm; }
    __syncthreads();
    if (a.p.periodic) {                                       // Sherman-Morrison correction for the two corner entries
        const double fp = (dp[0] + a.sm_coef * dp[L - 1]) / a.sm_denom, fm = (dm[0] + a.sm_coef * dm[L - 1]) / a.sm_denom;
        __syncthreads();
        for (int i = t; i < L; i += NT) { const double z = a.fz[i]; dp[i] -= z * fp; dm[i] -= z * fm; }
        __syncthreads();
    }
    (void)red;
}

// RESUMED: the launch starts from a checkpoint (a.span).  A fresh start keeps an instantiation of its own, in which the span is the
// constant 0 .. nsteps: with the span read at run time the BATCH form ran 2.8 % slower on the reference's beta sweep.
template <Form FORM, bool RESUMED>
__global__ __launch_bounds__(NT) void pde_kernel(const PdeArgs a) {
    extern __shared__ double lds[];
    const int L = a.p.L, t = threadIdx.x, sys = blockIdx.x, ntr = a.p.n_tracers;
    // the five fields and the kernel taps: in LDS when they fit (L <= ~3000), else in this system's slab of global memory
    // (one workgroup = one CU: its L1 / the L2 serve it, workgroup barriers order the accesses); the scan scratch stays in LDS
    double *fields = a.work ? a.work + (size_t)sys * (size_t)a.work_stride : lds;
    double *rp = fields, *rm = rp + L, *xp = rm + L, *xm = xp + L, *mf = xm + L, *ktab = mf + L;
    double *red = a.work ? lds : ktab + ((a.ktaps + 2) & ~1);
    double4 *scan = a.work ? reinterpret_cast<double4 *>(lds + ((NT + 3) & ~3))
                           : reinterpret_cast<double4 *>(lds + ((5 * L + ((a.ktaps + 2) & ~1) + NT + 3) & ~3));   // 32-byte aligned
    const double beta = a.beta[sys], dx = a.dx, dt = a.p.dt, lam = a.p.lam;
    for (int i = t; i < L; i += NT) { rp[i] = a.rho_p0[(size_t)sys * L + i]; rm[i] = a.rho_m0[(size_t)sys * L + i]; }
    const int mode = FORM == BATCH ? a.p.kernel_mode : a.sys_mode[sys], ktaps = FORM == BATCH ? a.ktaps : a.sys_ktaps[sys];
    const double *ktab_g = FORM == BATCH ? a.ktab : a.ktab + a.sys_ktab[sys];
    for (int i = t; i <= ktaps; i += NT) ktab[i] = ktab_g[i];
    double *trx = a.trx + (size_t)sys * ntr;
    int8_t *trs = a.trs + (size_t)sys * ntr;
    for (int i = t; i < ntr; i += NT) { trx[i] = a.tracer_x0[(size_t)sys * ntr + i]; trs[i] = a.tracer_s0[(size_t)sys * ntr + i]; }
    __syncthreads();
    pdek::Ctx fc{};
    if constexpr (FORM == SWEEP_SPECTRAL) {                     // behind the scans' scratch: buffer, twiddles, spectrum, sized by the launch's largest m
        fc.m = mode == 1 ? a.sys_log2[sys] : 0;
        fc.L = L; fc.kt = ktaps; fc.t = t; fc.rp = rp; fc.rm = rm; fc.mf = mf;
        fc.buf = reinterpret_cast<double2 *>(scan + 2 * NT);
        if (fc.m) {
            const int M = 1 << fc.m;
            fc.tw = fc.buf + M + (M >> 4); fc.spec = reinterpret_cast<double *>(fc.tw + (M >> 1));
            const double2 *tw_g = a.ctw + pdek::twiddle_offset(fc.m);
            for (int i = t; i < (M >> 1); i += NT) fc.tw[i] = tw_g[i];
            pdek::build_spectrum(fc, ktab);
        }
    }
    const double noise_amp = sqrt(2.0 * a.p.gamma * dt);
    const int nsteps = a.p.nsteps, n_begin = RESUMED ? a.span.n_begin : 0, n_end = RESUMED ? a.span.n_end : nsteps;
    const int row0 = RESUMED ? a.span.row0 : 0, n_rows = RESUMED ? a.span.n_rows : nsteps + 1, snap0 = RESUMED ? a.span.snap0 : 0;
#define PDE_ROW ((size_t)sys * n_rows + (n - row0))             /* this system's row of iteration n in the launch's series */
    for (int n = n_begin; n <= n_end; ++n) {
        // a resumed launch starts behind the row of its checkpoint's step: the magnetisation only, step() needs it
        const bool record = !RESUMED || n != n_begin;
        // ---- magnetisation of the current state (ref :156-168): used by the observables, the tracers and step()
        double m_global = 0.0;
        if (mode == 0) {
            for (int i = t; i < L; i += NT) mf[i] = (rp[i] - rm[i]) / (rp[i] + rm[i] + 1e-12);
        } else if (mode == 2) {
            double s = 0.0, w = 0.0;
            for (int i = t; i < L; i += NT) { s += rp[i] - rm[i]; w += rp[i] + rm[i]; }
            s = block_sum(s, red); w = block_sum(w, red);
            m_global = s / (w + 1e-12);
            for (int i = t; i < L; i += NT) mf[i] = m_global;
        } else if (FORM == SWEEP_SPECTRAL && fc.m) {           // circular convolution by the transform in LDS
            pdek::convolve(fc);
        } else if (FORM == SWEEP_SPECTRAL) {                   // a kernel of one tap (the plan gives it no transform): the direct sum's one term
            const double kv = ktab[0];
            for (int i = t; i < L; i += NT) mf[i] = (kv * (rp[i] - rm[i])) / (kv * (rp[i] + rm[i]) + 1e-12);
        } else {                                               // circular convolution, 4 consecutive sites per thread
            for (int base = 4 * t; base < L; base += 4 * NT) {
                double num[4] = {0, 0, 0, 0}, den[4] = {0, 0, 0, 0};
                // window holds s, tot at sites base + j + (0..3); slide j from -ktaps to +ktaps
                int idx = base - ktaps;
                idx %= L; if (idx < 0) idx += L;
                double sp[4], sm[4];
#pragma unroll
                for (int k = 0; k < 3; ++k) { sp[k + 1] = rp[idx]; sm[k + 1] = rm[idx]; idx = idx + 1 == L ? 0 : idx + 1; }
                for (int j = -ktaps; j <= ktaps; ++j) {
                    sp[0] = sp[1]; sp[1] = sp[2]; sp[2] = sp[3]; sm[0] = sm[1]; sm[1] = sm[2]; sm[2] = sm[3];
                    sp[3] = rp[idx]; sm[3] = rm[idx]; idx = idx + 1 == L ? 0 : idx + 1;
                    // site base + k sees source base + k + j  <=>  window slot k holds it when the window starts at base + j
                    const double kv = ktab[j < 0 ? -j : j];
#pragma unroll
                    for (int k = 0; k < 4; ++k) { num[k] += kv * (sp[k] - sm[k]); den[k] += kv * (sp[k] + sm[k]); }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) if (base + k < L) mf[base + k] = num[k] / (den[k] + 1e-12);
            }
        }
        __syncthreads();
        // ---- observables (ref :243-255)
        if (record) {
            double sm_ = 0.0, st = 0.0;
            for (int i = t; i < L; i += NT) { sm_ += mf[i]; st += rp[i] + rm[i]; }
            sm_ = block_sum(sm_, red); st = block_sum(st, red);
            const double mean_t = st / L;
            double sv = 0.0;
            for (int i = t; i < L; i += NT) { const double d = rp[i] + rm[i] - mean_t; sv += d * d; }
            sv = block_sum(sv, red);
            if (t == 0) {
                if (a.m_series) a.m_series[PDE_ROW] = mode == 2 ? m_global : sm_ / L;
                if (a.var_series) a.var_series[PDE_ROW] = sv / L;
            }
            if (a.fft_re)
                for (int k = t; k < a.p.n_fft_modes; k += NT) {   // rfft(total)[k] / L = sum total_i (cos - i sin)(2 pi k i / L) / L
                    double re = 0.0, im = 0.0;
                    int ph = 0;
                    for (int i = 0; i < L; ++i) {
                        const double v = rp[i] + rm[i];
                        re += v * a.twc[ph]; im -= v * a.tws[ph];
                        ph += k; if (ph >= L) ph -= L;
                    }
                    a.fft_re[PDE_ROW * a.p.n_fft_modes + k] = re / L;
                    a.fft_im[PDE_ROW * a.p.n_fft_modes + k] = im / L;
                }
            if (n % a.p.snapshot_interval == 0) {
                const size_t o = ((size_t)sys * a.n_snap + (n / a.p.snapshot_interval - snap0)) * L;
                for (int i = t; i < L; i += NT) {
                    if (a.snapshots) a.snapshots[o + i] = rp[i] + rm[i];
                    if (a.m_snapshots) a.m_snapshots[o + i] = rp[i] - rm[i];
                }
            }
        }
        // ---- tracers (ref :257-287)
        if (record && ntr > 0) {
            double sdr = 0.0;
            const bool windowed = n >= a.p.window;
            double *hist = a.hist + (size_t)sys * a.p.window * ntr;
            for (int i = t; i < ntr; i += NT) {
                double xu = trx[i];
                double xw = fmod(xu, a.p.xlim);                // numpy's % : floor modulo
                if (xw != 0.0 && xw < 0.0) xw += a.p.xlim;
                int idx = (int)(xw / dx) % L;
                const double m_loc = mf[idx];
                int s = trs[i];
                double u, g;
                if (a.rand_u) {
                    const size_t o = PDE_ROW * ntr + i;
                    u = a.rand_u[o]; g = a.rand_n[o];
                } else {
                    uint32_t x[4];
                    philox4x32_10((uint32_t)n, (uint32_t)i, (uint32_t)sys, 0x7AC3u, (uint32_t)a.p.seed, (uint32_t)(a.p.seed >> 32), x);
                    u = ((double)(x[0] >> 5) * 67108864.0 + (double)(x[1] >> 6)) * 0x1.0p-53;
                    const double u1 = ((double)x[2] + 0.5) * 0x1.0p-32, u2 = ((double)x[3] + 0.5) * 0x1.0p-32;
                    g = sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925 * u2);
                }
                const double rate = cw_rate(beta, (double)s, m_loc);
                if (u < rate * dt) s = -s;
                xu += lam * (double)s * dt + noise_amp * g;
                trx[i] = xu; trs[i] = (int8_t)s;
                hist[(size_t)(n % a.p.window) * ntr + i] = xu;
            }
            __syncthreads();
            if (windowed) {                                    // dr = x_n - x_{n - window + 1}  (ref: history[-window])
                const double *old = hist + (size_t)((n + 1) % a.p.window) * ntr;
                for (int i = t; i < ntr; i += NT) sdr += trx[i] - old[i];
                const double mean_dr = block_sum(sdr, red) / ntr;
                double sv = 0.0;
                for (int i = t; i < ntr; i += NT) { const double d = trx[i] - old[i] - mean_dr; sv += d * d; }
                sv = block_sum(sv, red) / ntr;
                if (t == 0) {
                    if (a.v_eff) a.v_eff[PDE_ROW] = mean_dr / (a.p.window * dt);
                    if (a.D_eff) a.D_eff[PDE_ROW] = sv / (2 * a.p.window * dt);
                }
            } else if (t == 0) {
                const double nan = __longlong_as_double(0x7ff8000000000000ll);
                if (a.v_eff) a.v_eff[PDE_ROW] = nan;
                if (a.D_eff) a.D_eff[PDE_ROW] = nan;
            }
        }
        if (n == n_end) break;
        // ---- step() (ref :190-233)
        for (int i = t; i < L; i += NT) { xp[i] = rp[i]; xm[i] = rm[i]; }
        __syncthreads();
        diffuse2(a, xp, xm, scan, red);
        double m0 = 0.0;
        for (int i = t; i < L; i += NT) m0 += xp[i] + xm[i];
        m0 = block_sum(m0, red);
        const int per = a.p.periodic;
        if (!a.p.anchored_minus) {
            for (int i = t; i < L; i += NT) {
                const double dpl = i > 0 ? (xp[i] - xp[i - 1]) / dx : (per ? (xp[0] - xp[L - 1]) / dx : 0.0);     // right-moving: backward difference
                const double dmr = i < L - 1 ? (xm[i + 1] - xm[i]) / dx : (per ? (xm[0] - xm[L - 1]) / dx : 0.0); // left-moving: forward difference
                const double Rp = cw_rate(beta, -1.0, mf[i]) * xm[i] - cw_rate(beta, 1.0, mf[i]) * xp[i];
                const double np_ = xp[i] + dt * (-lam * dpl + Rp), nm_ = xm[i] + dt * (lam * dmr + (-Rp));
                rp[i] = np_ < 0.0 ? 0.0 : np_; rm[i] = nm_ < 0.0 ? 0.0 : nm_;
            }
        } else {
            for (int i = t; i < L; i += NT) {                  // reaction first, into rp (star_p) / rm (star_m)
                const double Rp = cw_rate(beta, -1.0, mf[i]) * xm[i] - cw_rate(beta, 1.0, mf[i]) * xp[i];
                const double sp_ = xp[i] + dt * Rp, sm_ = xm[i] + dt * (-Rp);
                rp[i] = sp_ < 0.0 ? 0.0 : sp_; rm[i] = sm_ < 0.0 ? 0.0 : sm_;
            }
            __syncthreads();
            for (int i = t; i < L; i += NT) {                  // advection of star_p, result into xp
                const double dpl = i > 0 ? (rp[i] - rp[i - 1]) / dx : (per ? (rp[0] - rp[L - 1]) / dx : 0.0);
                const double v = rp[i] + dt * (-lam * dpl);
                xp[i] = v < 0.0 ? 0.0 : v;
            }
            __syncthreads();
            for (int i = t; i < L; i += NT) rp[i] = xp[i];
        }
        __syncthreads();
        double m1 = 0.0;
        for (int i = t; i < L; i += NT) m1 += rp[i] + rm[i];
        m1 = block_sum(m1, red);
        const double sc = m0 / m1;
        for (int i = t; i < L; i += NT) { rp[i] *= sc; rm[i] *= sc; }
        __syncthreads();
    }
#undef PDE_ROW
    for (int i = t; i < L; i += NT) {
        if (a.rho_p) a.rho_p[(size_t)sys * L + i] = rp[i];
        if (a.rho_m) a.rho_m[(size_t)sys * L + i] = rm[i];
    }
    for (int i = t; i < ntr; i += NT) {
        if (a.tracer_x) a.tracer_x[(size_t)sys * ntr + i] = trx[i];
        if (a.tracer_s) a.tracer_s[(size_t)sys * ntr + i] = trs[i];
    }
}


// ---- host: the plan of a sweep launch (pdek_plan; no device)
struct SweepPlan {
    std::vector<int> mode, ktaps, log2;
    std::vector<long long> ktab_off;
    std::vector<double> ktab;           // the systems' tables one after another (systems of one width share theirs)
    pdek_plan_info info{};
};

size_t base_lds_bytes(int L, int ktaps) {
    return (size_t)((5 * L + ((ktaps + 2) & ~1) + NT + 3) & ~3) * sizeof(double) + (size_t)2 * NT * sizeof(double4);
}

// 0, or PDE_ERR_ARG with the complaint in `why`
int make_sweep_plan(const pde_params *p, int32_t n_systems, const double *kernel_sigma, SweepPlan &pl, std::string &why) {
    if (!p || n_systems < 1) { why = "null argument or n_systems < 1"; return PDE_ERR_ARG; }
    if (p->L < 4 || p->L > PDE_MAX_L || !(p->xlim > 0.0)) { why = "L must be in [4, PDE_MAX_L], xlim > 0"; return PDE_ERR_ARG; }
    if (p->kernel_mode < 0 || p->kernel_mode > 2) { why = "kernel_mode must be 0, 1 or 2"; return PDE_ERR_ARG; }
    if (p->convolution != 0 && p->convolution != 1) { why = "convolution must be 0 (direct) or 1 (spectral)"; return PDE_ERR_ARG; }
    if (p->kernel_mode != 0 && !kernel_sigma) { why = "a Gaussian kernel needs kernel_sigma[n_systems]"; return PDE_ERR_ARG; }
    const int L = p->L;
    const double dx = p->xlim / L;
    pl.mode.assign(n_systems, 0); pl.ktaps.assign(n_systems, 0); pl.log2.assign(n_systems, 0); pl.ktab_off.assign(n_systems, 0);
    pl.ktab.assign(1, 1.0);                                    // modes 0 and 2 read nothing of it: one tap at offset 0
    int kmax = 0, mmax = 0;
    for (int s = 0; s < n_systems; ++s) {
        if (p->kernel_mode == 0) continue;
        const double sg = kernel_sigma[s];
        if (!std::isfinite(sg) || !(sg > 0.0)) { why = "kernel_sigma[" + std::to_string(s) + "] must be finite and > 0 for a Gaussian kernel"; return PDE_ERR_ARG; }
        if (sg > 100000) { pl.mode[s] = 2; continue; }          // ref :161
        pl.mode[s] = 1;
        int twin = -1;
        for (int r = 0; r < s && twin < 0; ++r) if (pl.mode[r] == 1 && kernel_sigma[r] == sg) twin = r;
        if (twin >= 0) { pl.ktaps[s] = pl.ktaps[twin]; pl.ktab_off[s] = pl.ktab_off[twin]; pl.log2[s] = pl.log2[twin]; continue; }
        pde_params q = *p;
        q.kernel_mode = 1; q.kernel_sigma = sg;
        std::vector<double> tab;
        pl.ktaps[s] = kernel_taps(&q, dx, tab);
        pl.ktab_off[s] = (long long)pl.ktab.size();
        pl.ktab.insert(pl.ktab.end(), tab.begin(), tab.end());
        if (p->convolution == 1 && pl.ktaps[s] > 0) pl.log2[s] = pdek::log2_for((long long)L + 2ll * pl.ktaps[s]);   // one tap: nothing to transform
        kmax = std::max(kmax, pl.ktaps[s]); mmax = std::max(mmax, pl.log2[s]);
    }
    const size_t base = base_lds_bytes(L, kmax);
    if (base > PDEK_LDS_LIMIT) { why = "not eligible: the five fields of L = " + std::to_string(L) + " sites do not fit LDS and would live in global memory; that is the wide shape's ground (pdew_solve, include/pde_wide.h)"; return PDE_ERR_ARG; }
    if (mmax > PDEK_MAX_LOG2) { why = "not eligible for the transform in LDS: L + 2 ktaps = " + std::to_string(L + 2 * kmax) + " needs 2^" + std::to_string(mmax) + " words, the largest is 2^" + std::to_string(PDEK_MAX_LOG2); return PDE_ERR_ARG; }
    const size_t lds = base + pdek::lds_bytes(mmax);
    if (lds > PDEK_LDS_LIMIT) { why = "not eligible for the transform in LDS: fields, taps and a transform of 2^" + std::to_string(mmax) + " words need " + std::to_string(lds) + " bytes of " + std::to_string(PDEK_LDS_LIMIT); return PDE_ERR_ARG; }
    pl.info.ktaps_max = kmax; pl.info.conv_log2_max = mmax; pl.info.lds_bytes = (int32_t)lds; pl.info.fields_in_lds = 1;
    return PDE_OK;
}

// ---- host: the driver of the entry points.  sweep == nullptr: pde_solve_batch / pder_solve, one table of taps from p->kernel_sigma.
// `span`: the steps and rows of the launch; io.from / io.to: the checkpoints of the resumable forms.
int solve_impl(const char *who, std::string &err, const SweepPlan *sweep, const pde_params *p, int32_t n_systems, const PdeIo &io, const PdeSpan &span) {
    OneShot job{who, err, false, PDE_ERR_NODEVICE, PDE_ERR_ARG, PDE_ERR_HIP};   // no zero-fill: the kernel writes every output in full
    if (int rc = job.select_device(p->device)) return rc;

    const int L = p->L;
    const PdeExtents x(p, n_systems, span);
    std::vector<double> plain;                                 // kernel taps (ref :84-93) of the one width; a sweep brings its systems' tables
    const int ktaps = sweep ? sweep->info.ktaps_max : kernel_taps(p, p->xlim / L, plain);
    PdeArgs a{};
    a.chunk = (L + NT - 1) / NT;
    if (int rc = pde_stage_inputs(job, a, p, x, io, ktaps, sweep ? sweep->ktab : plain)) return rc;
    if (sweep) {
        UP(sys_mode, sweep->mode.data(), x.S); UP(sys_ktaps, sweep->ktaps.data(), x.S);
        UP(sys_log2, sweep->log2.data(), x.S); UP(sys_ktab, sweep->ktab_off.data(), x.S);
        if (sweep->info.conv_log2_max) {
            std::vector<double2> ctw;
            pdek::build_twiddles(sweep->info.conv_log2_max, ctw);
            UP(ctw, ctw.data(), ctw.size());
        }
    }
    const bool tracer_series = true;                           // wherever the caller gave the pointer; without tracers nothing writes them: unspecified values
    if (int rc = pde_stage_outputs(job, a, p, x, io, tracer_series)) return rc;
    OUT(rho_p, io.rho_p ? io.rho_p : io.to ? io.to->rho_p : nullptr, x.SL); OUT(rho_m, io.rho_m ? io.rho_m : io.to ? io.to->rho_m : nullptr, x.SL);   // a checkpoint wants the fields too
    OUT(tracer_x, io.tracer_x, x.ST); OUT(tracer_s, io.tracer_s, x.ST);
    size_t lds = base_lds_bytes(L, ktaps);
    if (sweep) lds = (size_t)sweep->info.lds_bytes;             // the plan has refused what does not fit
    else if (lds > 160 * 1024) {                               // beyond LDS: the fields live in global memory, the scans' scratch in LDS
        a.work_stride = (long long)((5 * (size_t)L + ((ktaps + 2) & ~1) + 3) & ~(size_t)3);
        WORK(work, x.S * (size_t)a.work_stride);
        lds = (size_t)((NT + 3) & ~3) * sizeof(double) + (size_t)2 * NT * sizeof(double4);
    }
    void (*kernel)(const PdeArgs) = span.resume ? (!sweep ? pde_kernel<BATCH, true> : sweep->info.conv_log2_max ? pde_kernel<SWEEP_SPECTRAL, true> : pde_kernel<SWEEP_DIRECT, true>)
                                                : (!sweep ? pde_kernel<BATCH, false> : sweep->info.conv_log2_max ? pde_kernel<SWEEP_SPECTRAL, false> : pde_kernel<SWEEP_DIRECT, false>);
    if (int rc = job.raise_lds_limit(reinterpret_cast<const void *>(kernel), lds)) return rc;
    if (int rc = job.create_events()) return rc;
    job.ev.start();
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_systems), dim3(NT), lds, nullptr, a);
    job.ev.stop();
    if (int rc = job.finish(hipGetLastError(), "pde_kernel", io.kernel_ms)) return rc;
    DOWN(io.rho_p, rho_p, x.SL * 8); DOWN(io.rho_m, rho_m, x.SL * 8);
    if (int rc = pde_fetch_outputs(job, a, p, x, io, tracer_series)) return rc;
    DOWN(io.tracer_x, tracer_x, x.ST * 8); DOWN(io.tracer_s, tracer_s, x.ST);
    return pde_fetch_checkpoint(job, a, p, x, io, a.rho_p, a.rho_m);
}

// The checks and the launch behind pde_solve_batch and pder_solve, behind pdek_solve and pdekr_solve: one body each, worded
// by the entry's name.
int batch_entry(const char *who, std::string &err, const pde_params *p, int32_t n_systems, PdeIo io) {
    auto bad = [&](const char *m) { err = std::string(who) + ": " + m; return PDE_ERR_ARG; };
    PdeSpan span;
    if (const char *why = adopt_checkpoint(p, io, span)) return bad(why);
    if (const char *why = check_args(p, n_systems, io)) return bad(why);
    if (p->convolution != 0) return bad("convolution must be 0 here: the spectral convolution belongs to the wide shape (pdew_solve, include/pde_wide.h)");
    return solve_impl(who, err, nullptr, p, n_systems, io, span);
}

int sweep_entry(const char *who, std::string &err, const pde_params *p, int32_t n_systems, const double *kernel_sigma, PdeIo io) {
    auto bad = [&](const std::string &m) { err = std::string(who) + ": " + m; return PDE_ERR_ARG; };
    PdeSpan span;
    if (const char *why = adopt_checkpoint(p, io, span)) return bad(why);
    if (const char *why = check_args(p, n_systems, io)) return bad(why);
    SweepPlan pl;
    std::string why;
    if (make_sweep_plan(p, n_systems, kernel_sigma, pl, why)) return bad(why);
    return solve_impl(who, err, &pl, p, n_systems, io, span);
}

}  // namespace

extern "C" {

const char *pde_last_error(void) { return g_err.c_str(); }

int pde_solve_batch(const pde_params *p, int32_t n_systems, const double *beta, const double *rho_p0, const double *rho_m0,
                    const double *tracer_x0, const int8_t *tracer_s0, const double *rand_u, const double *rand_n,
                    double *rho_p, double *rho_m, double *m_series, double *var_series, double *v_eff_series,
                    double *D_eff_series, double *snapshots, double *m_snapshots, double *fft_re, double *fft_im,
                    double *tracer_x, int8_t *tracer_s, double *kernel_ms) {
    const PdeIo io{beta, rho_p0, rho_m0, tracer_x0, tracer_s0, rand_u, rand_n, rho_p, rho_m, m_series, var_series, v_eff_series,
                   D_eff_series, snapshots, m_snapshots, fft_re, fft_im, tracer_x, tracer_s, kernel_ms};
    return batch_entry("pde_solve_batch", g_err, p, n_systems, io);
}

const char *pdek_last_error(void) { return g_err_k.c_str(); }

int pdek_plan(const pde_params *p, int32_t n_systems, const double *kernel_sigma,
              pdek_plan_info *info, int32_t *kernel_mode, int32_t *ktaps, int32_t *conv_log2) {
    SweepPlan pl;
    std::string why;
    if (int rc = make_sweep_plan(p, n_systems, kernel_sigma, pl, why)) { g_err_k = "pdek_plan: " + why; return rc; }
    if (info) *info = pl.info;
    for (int s = 0; s < n_systems; ++s) {
        if (kernel_mode) kernel_mode[s] = pl.mode[s];
        if (ktaps) ktaps[s] = pl.ktaps[s];
        if (conv_log2) conv_log2[s] = pl.log2[s];
    }
    return PDE_OK;
}

int pdek_solve(const pde_params *p, int32_t n_systems, const double *beta, const double *kernel_sigma,
               const double *rho_p0, const double *rho_m0, const double *tracer_x0, const int8_t *tracer_s0,
               const double *rand_u, const double *rand_n,
               double *rho_p, double *rho_m, double *m_series, double *var_series, double *v_eff_series,
               double *D_eff_series, double *snapshots, double *m_snapshots, double *fft_re, double *fft_im,
               double *tracer_x, int8_t *tracer_s, double *kernel_ms) {
    const PdeIo io{beta, rho_p0, rho_m0, tracer_x0, tracer_s0, rand_u, rand_n, rho_p, rho_m, m_series, var_series, v_eff_series,
                   D_eff_series, snapshots, m_snapshots, fft_re, fft_im, tracer_x, tracer_s, kernel_ms};
    return sweep_entry("pdek_solve", g_err_k, p, n_systems, kernel_sigma, io);
}

const char *pder_last_error(void) { return g_err_r.c_str(); }
const char *pdekr_last_error(void) { return g_err_kr.c_str(); }

int pder_extents(const pde_params *p, int32_t from_step, int32_t *first_row, int32_t *n_rows, int32_t *n_snap, int32_t *first_snap) {
    auto bad = [&](const char *m) { g_err_r = std::string("pder_extents: ") + m; return PDE_ERR_ARG; };
    if (!p) return bad("null argument");
    PdeSpan sp;
    if (const char *why = pde_span(p, from_step, sp)) return bad(from_step < -1 ? "from_step must be >= -1" : why);
    if (first_row) *first_row = sp.row0;
    if (n_rows) *n_rows = sp.n_rows;
    if (n_snap) *n_snap = sp.n_snap;
    if (first_snap) *first_snap = sp.snap0;
    return PDE_OK;
}

int pder_solve(const pde_params *p, int32_t n_systems, const double *beta, const double *rho_p0, const double *rho_m0,
               const double *tracer_x0, const int8_t *tracer_s0, const double *rand_u, const double *rand_n,
               double *rho_p, double *rho_m, double *m_series, double *var_series, double *v_eff_series,
               double *D_eff_series, double *snapshots, double *m_snapshots, double *fft_re, double *fft_im,
               double *tracer_x, int8_t *tracer_s, double *kernel_ms, const pde_checkpoint *from, pde_checkpoint *to) {
    const PdeIo io{beta, rho_p0, rho_m0, tracer_x0, tracer_s0, rand_u, rand_n, rho_p, rho_m, m_series, var_series, v_eff_series,
                   D_eff_series, snapshots, m_snapshots, fft_re, fft_im, tracer_x, tracer_s, kernel_ms, from, to};
    return batch_entry("pder_solve", g_err_r, p, n_systems, io);
}

int pdekr_solve(const pde_params *p, int32_t n_systems, const double *beta, const double *kernel_sigma,
                const double *rho_p0, const double *rho_m0, const double *tracer_x0, const int8_t *tracer_s0,
                const double *rand_u, const double *rand_n,
                double *rho_p, double *rho_m, double *m_series, double *var_series, double *v_eff_series,
                double *D_eff_series, double *snapshots, double *m_snapshots, double *fft_re, double *fft_im,
                double *tracer_x, int8_t *tracer_s, double *kernel_ms, const pde_checkpoint *from, pde_checkpoint *to) {
    const PdeIo io{beta, rho_p0, rho_m0, tracer_x0, tracer_s0, rand_u, rand_n, rho_p, rho_m, m_series, var_series, v_eff_series,
                   D_eff_series, snapshots, m_snapshots, fft_re, fft_im, tracer_x, tracer_s, kernel_ms, from, to};
    return sweep_entry("pdekr_solve", g_err_kr, p, n_systems, kernel_sigma, io);
}

}  // extern "C"
