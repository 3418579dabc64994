"""Exact event loop with structure sums taken on the device (gils_run): what recording costs, and the public function against
the host route over full outputs.  The shape is the reference's own structure study (PARTICLE_solver_BIOLOGY_local_structure.py
:671-753): 33 systems (11 beta x 3 runs), L = 1000, N = 900, K = 1, T = 40, local_kernel_sigma = 0.005, all L modes, with
obs_dt = 1 as in the driver and again with obs_dt = 0.1; then a large-shape size: 8 systems, L = 4200, N = 2000, 64 modes.

    python tools/time_exact_structure.py [--repeats 3] [--only batch_dt1,batch_dt01,large] [--out profiles/exact_structure_bench.json]

(a) kernel_ms of gils_run against gil_run_batch / gilm_run with the same parameters and seed, neither downloading states;
(b) wall time of run_batched_exact_structure against run_batched_exact(record_fft=True, record_var=True) +
    observables.structure_observables, the only route without the sums.
Every figure is the median of `repeats` runs after one warm-up.  A section whose output file exists is kept, so the sections can
run as separate processes, each under a time limit of its own."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"
gil = importlib.import_module(PKG + ".gillespie")
obs = importlib.import_module(PKG + ".observables")
psys = importlib.import_module(PKG + ".particle_system")

SECTIONS = {
    "batch_dt1": dict(L=1000, N=900, n_systems=33, T=40.0, obs_dt=1.0, k_max=1000),
    "batch_dt01": dict(L=1000, N=900, n_systems=33, T=40.0, obs_dt=0.1, k_max=1000),
    "large": dict(L=4200, N=2000, n_systems=8, T=40.0, obs_dt=1.0, k_max=64),
}


def systems(sec):
    """The driver's constructor keywords (ref :694-714); beta over [0, 3] as there, a seeded initial condition per system."""
    kw = dict(L=sec["L"], xlim=1, rate_diffusion=0.05, rate_active=5, init="fixed", N=sec["N"], scale_rates=False, local_kernel_sigma=0.005,
              minus_anchor=True, periodic=False, site_capacity=1, k_on=0, k_off=0, k_exit=0, seed=1)
    betas = np.linspace(0.0, 3.0, 11)
    return [psys.ParticleSystem(beta=float(betas[i % 11]), rng=np.random.default_rng(100 + i), **kw) for i in range(sec["n_systems"])]


def median_of(fn, repeats):
    fn()                                                          # warm-up
    runs = [fn() for _ in range(repeats)]
    return dict(median=statistics.median(runs), runs=runs)


def section(name, repeats):
    sec = SECTIONS[name]
    sy = systems(sec)
    first, inits = sy[0], [ps.init_particles() for ps in sy]
    times = np.arange(0.0, sec["T"], sec["obs_dt"])
    kw = dict(L=first.L, K=first.K, periodic=first.periodic, sigma_grid=first._sigma_grid, rate_diffusion=first.rate_diffusion,
              rate_active=first.rate_active, betas=[float(ps.beta) for ps in sy], states=inits, times_obs=times, T=sec["T"], seed=1,
              want_states=False)
    plain_entry = gil.run_raw if gil.plan_structure(L=first.L, K=first.K, periodic=False, sigma_grid=first._sigma_grid, n_systems=len(sy),
                                                    n_cap=sec["N"], n_obs=len(times), k_max=sec["k_max"])["shape"] == 0 else gil.run_many_large_raw
    events = []

    def with_sums():
        r = gil.run_structure_raw(k_max=sec["k_max"], first_obs=0, **kw)
        events.append(int(r["n_events"].sum()))
        return r["kernel_ms"]

    res = dict(shape=dict(sec, n_obs=len(times)))
    res["kernel_ms_with_sums"] = median_of(with_sums, repeats)
    res["kernel_ms_plain"] = median_of(lambda: plain_entry(**kw)["kernel_ms"], repeats)
    res["events"] = events[-1]
    res["recording_share"] = res["kernel_ms_with_sums"]["median"] / res["kernel_ms_plain"]["median"] - 1.0

    def device_route():
        t0 = time.perf_counter()
        rows = gil.run_batched_exact_structure(systems(sec), T=sec["T"], obs_dt=sec["obs_dt"], start_fraction=0.5, k_max=sec["k_max"])
        assert len(rows) == sec["n_systems"]
        return time.perf_counter() - t0

    def host_route():
        t0 = time.perf_counter()
        outs = gil.run_batched_exact(systems(sec), T=sec["T"], obs_dt=sec["obs_dt"], record_fft=True, record_var=True)
        rows = [obs.structure_observables(out, start_fraction=0.5, k_max=sec["k_max"]) for out in outs]
        assert len(rows) == sec["n_systems"]
        return time.perf_counter() - t0

    res["wall_s_device_sums"] = median_of(device_route, repeats)
    res["wall_s_host_route"] = median_of(host_route, repeats)
    res["wall_ratio"] = res["wall_s_host_route"]["median"] / res["wall_s_device_sums"]["median"]
    print(f"{name}: kernel {res['kernel_ms_with_sums']['median']:.1f} ms with sums, {res['kernel_ms_plain']['median']:.1f} ms without "
          f"(+{res['recording_share']:.1%}), {res['events']} events; wall {res['wall_s_device_sums']['median']:.2f} s against "
          f"{res['wall_s_host_route']['median']:.2f} s over full outputs", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=",".join(SECTIONS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_structure_bench.json"))
    a = ap.parse_args()
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            res = json.load(fh)
    for name in a.only.split(","):
        res[name] = section(name, a.repeats)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
