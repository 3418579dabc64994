"""Exact event loop with ensemble density and field profiles summed on the device (gilp_run): what recording costs, and
ensemble.profile_sweep from device sums against the same sweep over full outputs.  The shape is the beta-sweep driver's
(PARTICLE_solver_BIOLOGY_EXCLUSION_sweep_beta.py): L = 1000, N = 500, K = 1, sigma = 0.005, walls, rate_active = 5,
rate_diffusion = 0.05, scale_rates = False, T = 20, 1024 systems in 32 groups (beta over [0, 3]), with obs_dt = 0.5 and 0.05, n_bins
50 and 1000, without and with the field; then one large-shape size: 8 systems of L = 4200, N = 2000 in 2 groups.

    python tools/time_exact_profiles.py [--repeats 3] [--only batch_dt05,batch_dt005,large,sweep_dt05,sweep_dt005]
                                        [--out profiles/exact_profiles_bench.json]

(a) kernel_ms of gilp_run (all state outputs NULL) against gil_run_batch / gilm_run on the same inputs, taken alternately:
    `repeats` pairs after one warm-up pair, the median of each side.  This is where the 64-bit integer global atomics of the
    group sums show: 32 workgroups add to one row of sums.
(b) wall time of ensemble.profile_sweep (32 betas x 8 runs, 50 bins) with on_device=True against on_device=False, and the
    bytes each route brings off the device.
A section whose result is in the output file is replaced, the others are kept, so the sections can run as separate processes,
each under a time limit of its own."""
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
psys = importlib.import_module(PKG + ".particle_system")
ens = importlib.import_module(PKG + ".ensemble")

DRIVER = dict(xlim=1, rate_diffusion=0.05, rate_active=5, scale_rates=False, local_kernel_sigma=0.005, minus_anchor=True, periodic=False,
              site_capacity=1, k_on=0, k_off=0, k_exit=0, seed=1)
SECTIONS = {
    "batch_dt05": dict(L=1000, N=500, n_systems=1024, n_groups=32, T=20.0, obs_dt=0.5, bins=(50, 1000)),
    "batch_dt005": dict(L=1000, N=500, n_systems=1024, n_groups=32, T=20.0, obs_dt=0.05, bins=(50, 1000)),
    "large": dict(L=4200, N=2000, n_systems=8, n_groups=2, T=20.0, obs_dt=0.5, bins=(50, 1000)),
    "sweep_dt05": dict(L=1000, N=500, n_betas=32, n_runs=8, T=20.0, obs_dt=0.5, n_bins=50),
    "sweep_dt005": dict(L=1000, N=500, n_betas=32, n_runs=8, T=20.0, obs_dt=0.05, n_bins=50),
}


def median_and_runs(runs):
    return dict(median=statistics.median(runs), runs=runs)


def kernel_section(name, repeats):
    sec = SECTIONS[name]
    betas = np.linspace(0.0, 3.0, sec["n_groups"])
    groups = np.arange(sec["n_systems"], dtype=np.int32) % sec["n_groups"]
    sy = [psys.ParticleSystem(L=sec["L"], init="fixed", N=sec["N"], beta=float(betas[g]), rng=np.random.default_rng(100 + i), **DRIVER)
          for i, g in enumerate(groups)]
    first = sy[0]
    times = np.arange(0.0, sec["T"], sec["obs_dt"])
    kw = dict(L=first.L, K=first.K, periodic=first.periodic, sigma_grid=first._sigma_grid, rate_diffusion=first.rate_diffusion,
              rate_active=first.rate_active, betas=[float(ps.beta) for ps in sy], states=[ps.init_particles() for ps in sy], times_obs=times,
              T=sec["T"], seed=1, want_states=False)
    res = dict(shape=dict(sec, n_obs=len(times)), variants={})
    for n_bins in sec["bins"]:
        for want_field in (False, True):
            plan = gil.plan_profiles(L=first.L, K=first.K, periodic=False, sigma_grid=first._sigma_grid, n_systems=len(sy), n_cap=sec["N"],
                                     n_obs=len(times), n_bins=n_bins, n_groups=sec["n_groups"], want_field=want_field, want_states=False)
            plain_entry = gil.run_raw if plan["shape"] == 0 else gil.run_many_large_raw
            prof, plain, events = [], [], 0
            for it in range(repeats + 1):                          # alternately; the first pair warms up
                r = gil.run_profiles_raw(n_bins=n_bins, want_field=want_field, group_of_system=groups, n_groups=sec["n_groups"], **kw)
                p = plain_entry(**kw)
                assert np.array_equal(r["n_events"], p["n_events"]) and np.array_equal(r["scalars"], p["scalars"])
                assert int(r["ensemble_sums"][:, :, :2].sum()) == int(p["scalars"][:, :, 0].sum())     # every live particle was counted
                events = int(r["n_events"].sum())
                if it:
                    prof.append(r["kernel_ms"])
                    plain.append(p["kernel_ms"])
            v = dict(kernel_shape=plan["shape"], threads=plan["threads"], lds_bytes=plan["lds_bytes"], kernel_ms_profiles=median_and_runs(prof),
                     kernel_ms_plain=median_and_runs(plain), events=events, nonzero_sums=int(np.count_nonzero(r["ensemble_sums"])),
                     bytes_off_device=int(r["ensemble_sums"].nbytes + r["members"].nbytes))
            v["recording_share"] = v["kernel_ms_profiles"]["median"] / v["kernel_ms_plain"]["median"] - 1.0
            res["variants"][f"bins{n_bins}_field{int(want_field)}"] = v
            print(f"{name} n_bins {n_bins} field {int(want_field)}: kernel {v['kernel_ms_profiles']['median']:.1f} ms with profiles, "
                  f"{v['kernel_ms_plain']['median']:.1f} ms without ({v['recording_share']:+.1%}), {events} events", flush=True)
    return res


def sweep_section(name, repeats):
    sec = SECTIONS[name]
    betas = [float(b) for b in np.linspace(0.0, 3.0, sec["n_betas"])]
    kw = dict(beta_values=betas, n_runs_per_beta=sec["n_runs"], ps_kwargs=dict(DRIVER, L=sec["L"]), init_kwargs=dict(init="fixed", N=sec["N"]),
              run_kwargs=dict(T=sec["T"], obs_dt=sec["obs_dt"]), n_bins=sec["n_bins"],
              rng_seeds=[[1000 * b + r for r in range(sec["n_runs"])] for b in range(sec["n_betas"])])
    wall = {True: [], False: []}
    for it in range(repeats + 1):
        for on_device in (True, False):
            t0 = time.perf_counter()
            out = ens.profile_sweep(on_device=on_device, **kw)
            assert len(out) == sec["n_betas"]
            if it:
                wall[on_device].append(time.perf_counter() - t0)
    S, M = sec["n_betas"] * sec["n_runs"], len(np.arange(0.0, sec["T"], sec["obs_dt"]))
    res = dict(shape=dict(sec, n_obs=M), wall_s_on_device=median_and_runs(wall[True]), wall_s_full_outputs=median_and_runs(wall[False]),
               bytes_off_device_on_device=sec["n_betas"] * M * (7 * sec["n_bins"] * 8 + 4), bytes_off_device_full_outputs=S * M * sec["N"] * 6)
    res["wall_ratio"] = res["wall_s_full_outputs"]["median"] / res["wall_s_on_device"]["median"]
    print(f"{name}: sweep of {S} runs {res['wall_s_on_device']['median']:.2f} s on the device against {res['wall_s_full_outputs']['median']:.2f} s "
          f"over full outputs; {res['bytes_off_device_on_device']} against {res['bytes_off_device_full_outputs']} bytes", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=",".join(SECTIONS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_profiles_bench.json"))
    a = ap.parse_args()
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            res = json.load(fh)
    for name in a.only.split(","):
        res[name] = (sweep_section if name.startswith("sweep") else kernel_section)(name, a.repeats)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
