"""Times the reference's kernel-width sweep (IMEX_PDE_solver_run_sweep_magn.py: L = 1000, kernel_sigma in {0.0005, 0.005, 0.05,
0.1, 1.0} x 5 seeded runs, gamma = 0.2, beta = 0.75, 1000 tracers) on the one-workgroup shape, three ways:

    sweep, direct      one launch of 25 systems (pdek_solve), the direct circular sum over each system's own taps
    sweep, spectral    one launch of 25 systems, the Gaussian-kernel magnetisation by the transform in LDS
    five launches      one solve_batch launch of 5 systems per width (pde_solve_batch): the way before include/pde_sweep.h

    python tools/time_pde_sweep.py [--steps 20000] [--repeats 3] [--runs 5] [--json OUT.json]

The three ways are run ALTERNATELY within each repeat after one warm-up round, so that they see the same state of the machine;
a row carries the best and the spread (worst - best) of its way.  Times are the library's own (events around the launch);
for the five launches their sum.  A last row times the fields alone where the kernel spans the ring (sigma = 0.1, four beta,
400 steps, no tracers): direct against spectral, the same way.  Every system starts from the driver's seeded initial condition (seed = 100 + 1000 k + r)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"
SIGMAS = [0.0005, 0.005, 0.05, 0.1, 1.0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tracers", type=int, default=1000)
    ap.add_argument("--json")
    a = ap.parse_args()
    pde = importlib.import_module(PKG + ".pde")
    dt = 5e-4
    ctor = dict(L=a.L, xlim=1.0, T=(a.steps + 0.5) * dt, dt=dt, gamma=0.2, lam=0.6, beta=0.75, bc="periodic",
                active_model="bidirectional", gaussian_kernel=True, snapshot_interval=max(a.steps, 1), record_fft=False)
    sig, rp, rm, tx, ts = [], [], [], [], []
    for k, sigma in enumerate(SIGMAS):
        for r in range(a.runs):
            s = pde.IMEXPDE(kernel_sigma=sigma, seed=100 + 1000 * k + r, **ctor)
            s.initialize(mode="homogeneous", rho0=1.0, noise=0.3, n_tracers=a.tracers)
            assert s.nsteps == a.steps
            sig.append(sigma); rp.append(s.rho_p); rm.append(s.rho_m); tx.append(s.tracers_unwrapped); ts.append(s.tracer_state)
    rp, rm, tx, ts = np.array(rp), np.array(rm), np.array(tx), np.array(ts)
    common = dict(L=a.L, xlim=1.0, dt=dt, nsteps=a.steps, gamma=0.2, lam=0.6, bc="periodic", active_model="bidirectional",
                  gaussian_kernel=True, snapshot_interval=max(a.steps, 1), seed=100, want_snapshots=False)
    tr = lambda rows: dict(tracer_x0=tx[rows], tracer_s0=ts[rows]) if a.tracers else {}
    every = slice(0, len(sig))

    def sweep(conv):
        r = pde.solve_sweep_raw(betas=0.75, kernel_sigmas=sig, convolution=conv, rho_p0=rp, rho_m0=rm, **tr(every), **common)
        return r["kernel_ms"], r["m_series"]

    def five_launches():
        ms, m = 0.0, []
        for k, sigma in enumerate(SIGMAS):
            rows = slice(k * a.runs, (k + 1) * a.runs)
            r = pde.solve_batch_raw(betas=[0.75] * a.runs, kernel_sigma=sigma, rho_p0=rp[rows], rho_m0=rm[rows], **tr(rows), **common)
            ms += r["kernel_ms"]; m.append(r["m_series"])
        return ms, np.concatenate(m)

    ways = [("sweep_direct", lambda: sweep("direct")), ("sweep_spectral", lambda: sweep("spectral")), ("five_solve_batch_launches", five_launches)]
    times, series = {n: [] for n, _ in ways}, {}
    for rep in range(a.repeats + 1):
        for name, fn in ways:
            ms, m = fn()
            series[name] = m
            if rep or a.repeats == 0:
                times[name].append(ms)
    plan = pde.sweep_plan(L=a.L, kernel_sigmas=SIGMAS, convolution="spectral", gaussian_kernel=True, n_tracers=a.tracers)
    rows = []
    for name, _ in ways:
        best, worst = min(times[name]), max(times[name])
        rows.append(dict(way=name, kernel_ms=best, kernel_ms_spread=worst - best, us_per_step=best * 1e3 / max(a.steps, 1),
                         ratio_to_sweep_direct=min(times["sweep_direct"]) / best,
                         max_abs_m_series_minus_sweep_direct=float(np.max(np.abs(series[name] - series["sweep_direct"])))))
        print(json.dumps(rows[-1]), flush=True)
    # the shape of the test that requires the transform to win: sigma = 0.1 (ring-wide), four beta, 400 steps, nothing else recorded
    ring = dict(common, nsteps=400, snapshot_interval=400)
    rt = {"direct": [], "spectral": []}
    for rep in range(a.repeats + 1):
        for conv in rt:
            ms = pde.solve_sweep_raw(betas=[0.5, 0.75, 1.5, 2.5], kernel_sigmas=0.1, convolution=conv, rho_p0=rp[:4], rho_m0=rm[:4], **ring)["kernel_ms"]
            if rep or a.repeats == 0:
                rt[conv].append(ms)
    ring_row = dict(L=a.L, kernel_sigma=0.1, systems=4, steps=400, tracers=0,
                    direct_us_per_step=min(rt["direct"]) * 1e3 / 400, direct_spread_us=(max(rt["direct"]) - min(rt["direct"])) * 1e3 / 400,
                    spectral_us_per_step=min(rt["spectral"]) * 1e3 / 400, spectral_spread_us=(max(rt["spectral"]) - min(rt["spectral"])) * 1e3 / 400,
                    ratio_direct_to_spectral=min(rt["direct"]) / min(rt["spectral"]))
    print(json.dumps(ring_row), flush=True)
    out = dict(ring_wide_fields_only=ring_row, shape=dict(L=a.L, kernel_sigmas=SIGMAS, runs=a.runs, systems=len(sig), steps=a.steps, tracers=a.tracers, gamma=0.2, beta=0.75,
                          dt=dt), repeats=a.repeats, ktaps=plan["ktaps"], conv_log2=plan["conv_log2"], lds_bytes_spectral=plan["lds_bytes"],
               rows=rows)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
