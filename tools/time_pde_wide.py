"""Times the hydrodynamic-limit PDE on one fine grid: the wide shape (pdew_solve, one system over many workgroups) and,
when asked, the one-workgroup kernel (pde_solve_batch) on the same problem.

    python tools/time_pde_wide.py [--L 131072] [--sigma 0.005] [--steps 200] [--workgroups auto|G[,G...]] [--old-steps 0]
                                  [--convolution direct,spectral] [--repeats 3] [--json out.json]

Case neumann_anchored_kernel (the config-5 comparison's PDE), no tracers, no Fourier modes, so the time is the field
update alone.  Times are the library's own (events around the launch chain), best of --repeats after one warm-up
run.  Per run it prints us per step, launches per step, the convolution's multiply-adds per second from the WHOLE step
time (a lower bound for the convolution kernel itself; the per-kernel split comes from a rocprofv3 --kernel-trace run
of this script) against the binary64 vector peak, and with --old-steps > 0 the ratio to the one-workgroup kernel.
--convolution names the ways to evaluate the kernel convolution; several are run ALTERNATELY within each repeat, so that they
see the same state of the machine; a row carries the best and the spread (worst - best) of its way.  A spectral row also carries
the transforms' algorithmic bytes and flops per step, computed from the plan: every launch reads and writes the blocks' 2^m
complex words once (the first reads the state, the last writes the magnetisation instead), the middle one reads the spectrum;
5 m 2^m flops per transform of 2^m words, two transforms, plus the twiddle and spectrum products."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"
PEAK_FMA = 256 * 4 * 16 * 2.4e9          # CUs x SIMDs x binary64 fused multiply-adds per clock x 2.4 GHz = 39.3e12 / s
PEAK_HBM = 8.0e12                        # bytes / s, the data sheet's HBM3E figure


def transform_cost(plan, L):
    """Algorithmic bytes and flops per step of the spectral convolution's launches, from the plan."""
    m, B = plan["conv_log2"], plan["conv_blocks"]
    M, launches = 1 << m, 5 if m > 14 else 3
    words = B * M
    inner = launches - 2                                     # launches that read and write the complex words
    byts = 16 * L + 16 * words                               # first: the window of rho_plus, rho_minus in, words out
    byts += inner * 32 * words + 8 * words                   # in between: words in and out; the middle one also the spectrum
    byts += 16 * words + 8 * L                               # last: words in, the magnetisation out
    flops = words * (2 * 5 * m + 12 * (launches - 1) + 2)    # butterflies both ways; a twiddle per strided launch (hi * lo, then the word: 6 + 6); spectrum
    return byts, flops


def make(pde, L, sigma, steps, workgroups, convolution=None):
    dt = 5e-4
    s = pde.IMEXPDE(L=L, xlim=1.0, T=(steps + 0.5) * dt, dt=dt, gamma=2.33e-4, lam=0.6, beta=2.0, bc="neumann",
                    active_model="anchored_minus", gaussian_kernel=True, kernel_sigma=sigma, snapshot_interval=max(steps, 1),
                    seed=99, record_fft=False, workgroups=workgroups, convolution=convolution)
    assert s.nsteps == steps
    return s


def run_alternately(solvers, repeats):
    """One warm-up and `repeats` timed solves of every solver, in turn within each repeat; per solver (best, worst) ms."""
    times = [[] for _ in solvers]
    for rep in range(repeats + 1):
        for i, s in enumerate(solvers):
            s.initialize(mode="poisson", rho0=1.0, noise=0.2, n_tracers=0)
            s.solve()
            if rep or repeats == 0:
                times[i].append(s.kernel_ms)
    return [(min(t), max(t)) for t in times]


def run(pde, L, sigma, steps, workgroups, repeats):
    s = make(pde, L, sigma, steps, workgroups)
    return run_alternately([s], repeats)[0][0], s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=131072)
    ap.add_argument("--sigma", type=float, default=0.005)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--workgroups", default="auto")
    ap.add_argument("--old-steps", type=int, default=0, help="also time the one-workgroup kernel over this many steps")
    ap.add_argument("--convolution", default="direct", help="direct, spectral or both (comma-separated): run alternately")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json")
    a = ap.parse_args()
    pde = importlib.import_module(PKG + ".pde")
    rows = []
    old_us = None
    if a.old_steps > 0:
        ms, _ = run(pde, a.L, a.sigma, a.old_steps, None, 0)
        old_us = ms * 1e3 / a.old_steps
    for wg in a.workgroups.split(","):
        wg = wg if wg == "auto" else int(wg)
        convs = a.convolution.split(",")
        solvers = [make(pde, a.L, a.sigma, a.steps, wg, c) for c in convs]
        direct_us = None
        for c, s, (ms, ms_worst) in zip(convs, solvers, run_alternately(solvers, a.repeats)):
            plan = s.plan()
            us = ms * 1e3 / a.steps
            fma = 2.0 * a.L * (2 * plan["ktaps"] + 1)            # num and den, every tap of every site (what the direct sum does)
            row = dict(L=a.L, kernel_sigma=a.sigma, steps=a.steps, workgroups=plan["workgroups"], slab_len=plan["slab_len"],
                       ktaps=plan["ktaps"], launches_per_step=plan["launches_per_step"], lds_bytes=plan["lds_bytes"],
                       convolution=plan["convolution"], us_per_step=us, us_per_step_spread=(ms_worst - ms) * 1e3 / a.steps,
                       one_workgroup_us_per_step=old_us, ratio_to_one_workgroup=None if old_us is None else old_us / us,
                       m_last=float(s.m_series[-1]))
            if plan["convolution"] == "direct":
                direct_us = us
                row.update(conv_fma_per_step=fma, conv_fma_per_s_lower_bound=fma / (us * 1e-6),
                           fraction_of_f64_vector_peak_lower_bound=fma / (us * 1e-6) / PEAK_FMA)
            else:
                byts, flops = transform_cost(plan, a.L)
                row.update(conv_log2=plan["conv_log2"], conv_blocks=plan["conv_blocks"], conv_block_sites=plan["conv_block_sites"],
                           transform_bytes_per_step=byts, transform_flops_per_step=flops,
                           transform_bytes_per_s_lower_bound=byts / (us * 1e-6),
                           fraction_of_hbm_peak_lower_bound=byts / (us * 1e-6) / PEAK_HBM,
                           ratio_to_direct=None if direct_us is None else direct_us / us)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(dict(case="neumann_anchored_kernel", peak_f64_fma_per_s=PEAK_FMA, peak_hbm_bytes_per_s=PEAK_HBM, rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
