"""Times the hydrodynamic-limit PDE on one fine grid: the wide shape (pdew_solve, one system over many workgroups) and,
when asked, the one-workgroup kernel (pde_solve_batch) on the same problem.

    python tools/time_pde_wide.py [--L 131072] [--sigma 0.005] [--steps 200] [--workgroups auto|G[,G...]] [--old-steps 0]
                                  [--repeats 3] [--json out.json]

Case neumann_anchored_kernel (the config-5 comparison's PDE), no tracers, no Fourier modes, so the time is the field
update alone.  Times are the library's own (events around the launch chain), best of --repeats after one warm-up
run.  Per run it prints us per step, launches per step, the convolution's multiply-adds per second from the WHOLE step
time (a lower bound for the convolution kernel itself; the per-kernel split comes from a rocprofv3 --kernel-trace run
of this script) against the binary64 vector peak, and with --old-steps > 0 the ratio to the one-workgroup kernel."""
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


def run(pde, L, sigma, steps, workgroups, repeats):
    dt = 5e-4
    s = pde.IMEXPDE(L=L, xlim=1.0, T=(steps + 0.5) * dt, dt=dt, gamma=2.33e-4, lam=0.6, beta=2.0, bc="neumann",
                    active_model="anchored_minus", gaussian_kernel=True, kernel_sigma=sigma, snapshot_interval=max(steps, 1),
                    seed=99, record_fft=False, workgroups=workgroups)
    assert s.nsteps == steps
    best, out = None, None
    for rep in range(repeats + 1):
        s.initialize(mode="poisson", rho0=1.0, noise=0.2, n_tracers=0)
        s.solve()
        if rep and (best is None or s.kernel_ms < best):
            best = s.kernel_ms
        out = s
    return best if best is not None else out.kernel_ms, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=131072)
    ap.add_argument("--sigma", type=float, default=0.005)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--workgroups", default="auto")
    ap.add_argument("--old-steps", type=int, default=0, help="also time the one-workgroup kernel over this many steps")
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
        ms, s = run(pde, a.L, a.sigma, a.steps, wg, a.repeats)
        plan = s.plan()
        us = ms * 1e3 / a.steps
        fma = 2.0 * a.L * (2 * plan["ktaps"] + 1)                # num and den, every tap of every site
        row = dict(L=a.L, kernel_sigma=a.sigma, steps=a.steps, workgroups=plan["workgroups"], slab_len=plan["slab_len"],
                   ktaps=plan["ktaps"], launches_per_step=plan["launches_per_step"], lds_bytes=plan["lds_bytes"],
                   us_per_step=us, conv_fma_per_step=fma, conv_fma_per_s_lower_bound=fma / (us * 1e-6),
                   fraction_of_f64_vector_peak_lower_bound=fma / (us * 1e-6) / PEAK_FMA,
                   one_workgroup_us_per_step=old_us, ratio_to_one_workgroup=None if old_us is None else old_us / us,
                   m_last=float(s.m_series[-1]))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(dict(case="neumann_anchored_kernel", peak_f64_fma_per_s=PEAK_FMA, rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
