"""Times the ensemble-profile sweeps over the interaction range and over the density under the exact dynamics, once as the host
loop (one gilp_run launch per sigma / per N, ensemble.profile_sweep) and once as ONE mixed launch with profiles
(include/gillespie_mixed_profile.h), and the same mixed launch without profiles (gilx_run / gilxm_run) for the cost of recording:
  sigma sweep        9 sigma x 11 beta x 5 runs, L = 1000, N = 750, T = 20, 250 bins, with the field
  density sweep      19 N x 11 beta x 4 runs, L = 1000, T = 10, 250 bins
  large sigma sweep  9 sigma x 4 beta x 2 runs, L = 8192, N = 6144, T = 1, 1024 bins, with the field (the large shape)
obs_dt = 0.1.  Every timing is the kernel time of HIP events around the launch, taken REPS times after one untimed round that
loads the code objects; the file holds the median and the extremes.  Writes profiles/exact_mixed_profiles_bench.json.

--yardstick-lib PATH: a libaps_hip.so built from the parent commit.  The entry points this feature leaves unchanged (gilp_run,
gilx_run, gilxm_run) are then timed with both libraries on the same seeded inputs, in child processes (APS_LIB names the
library a child loads) that alternate between the two builds, ROUNDS times each; the file holds per build the median and the
extremes over all rounds, and whether both builds returned the same bits.
APS_ONLY_SWEEPS=name[,name]: time a selection only and add it to what out.json holds (for sessions that must stay short).
Usage (GPU box): python tools/time_exact_mixed_profiles.py [--yardstick-lib PATH] [out.json]"""
import importlib
import json
import os
import subprocess
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"
capi = importlib.import_module(PKG + ".capi")
if os.environ.get("APS_LIB"):                      # the child of --yardstick-lib: another build of the library
    capi.LIB_PATH = os.environ["APS_LIB"]
gil = importlib.import_module(PKG + ".gillespie")
ParticleSystem = importlib.import_module(PKG + ".particle_system").ParticleSystem

REPS, ROUNDS = 5, 4
BETAS = np.linspace(0, 3, 11)
SIGMAS = [1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 3e-2, 0.1, 0.3, 0]
NUMBERS = [int(n) for n in np.linspace(50, 950, 19)]
COMMON = dict(xlim=1, scale_rates=False, periodic=False, site_capacity=1, k_on=0, k_off=0, k_exit=0, seed=2026, init="fixed")
SWEEPS = {
    "sigma_sweep": dict(T=20.0, runs=5, betas=BETAS, n_bins=250, want_field=True, labels=SIGMAS,
                        cases=[dict(COMMON, L=1000, N=750, rate_diffusion=0.002, rate_active=5, local_kernel_sigma=s) for s in SIGMAS]),
    "density_sweep": dict(T=10.0, runs=4, betas=BETAS, n_bins=250, want_field=False, labels=NUMBERS,
                          cases=[dict(COMMON, L=1000, N=n, rate_diffusion=0.005, rate_active=10, local_kernel_sigma=0.02) for n in NUMBERS]),
    "large_sigma_sweep": dict(T=1.0, runs=2, betas=BETAS[::3], n_bins=1024, want_field=True, labels=SIGMAS,
                              cases=[dict(COMMON, L=8192, N=6144, site_capacity=2, rate_diffusion=0.002, rate_active=5, local_kernel_sigma=s)
                                     for s in SIGMAS]),
}


def spread(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), reps=len(ms))


def build(sweep):
    """The systems of a sweep in the order of the host loop (case, beta, run), the ensemble group and the key group of each."""
    systems, group, key_group = [], [], []
    for ci, case in enumerate(sweep["cases"]):
        for bi, beta in enumerate(sweep["betas"]):
            for r in range(sweep["runs"]):
                systems.append(ParticleSystem(beta=beta, rng=np.random.default_rng(100000 * ci + 100 * bi + r), **case))
                group.append(ci * len(sweep["betas"]) + bi)
                key_group.append(ci)
    return systems, group, key_group


def same_rows(a, b):
    return all(set(x) == set(y) and all(np.array_equal(np.asarray(x[k], float), np.asarray(y[k], float), equal_nan=True) for k in x)
               for x, y in zip(a, b))


def time_sweep(name, sweep):
    run_kw = dict(T=sweep["T"], obs_dt=0.1)
    prof_kw = dict(n_bins=sweep["n_bins"], want_field=sweep["want_field"])
    B, per = len(sweep["betas"]), len(sweep["betas"]) * sweep["runs"]
    loop_ms, one_ms, bare_ms, loop_rows, rows, events = [], [], [], None, None, 0
    for rep in range(REPS + 1):                                    # round 0 loads the code objects and is not kept
        systems, group, key_group = build(sweep)
        got, ms = [], []
        for ci in range(len(sweep["cases"])):                      # the host loop: one gilp_run launch per case
            mine = systems[ci * per:(ci + 1) * per]
            got += gil.run_batched_exact_profiles(mine, groups=[g - ci * B for g in group[ci * per:(ci + 1) * per]], **prof_kw, **run_kw)
            ms.append(mine[0].kernel_ms)
        events = int(sum(ps.n_events for ps in systems))
        systems, group, key_group = build(sweep)                   # one mixed launch with profiles
        rows = gil.run_batched_exact_profiles_mixed(systems, groups=group, key_groups=key_group, allow_large=True, **prof_kw, **run_kw)
        with_ms = systems[0].kernel_ms
        assert events == int(sum(ps.n_events for ps in systems))
        systems, group, key_group = build(sweep)                   # the same mixed launch without profiles: sums only, no states
        gil.run_batched_exact_statistics_mixed(systems, groups=key_group, allow_large=True, **run_kw)
        assert events == int(sum(ps.n_events for ps in systems))
        if rep:
            loop_ms.append(ms)
            one_ms.append(with_ms)
            bare_ms.append(systems[0].kernel_ms)
        loop_rows = got
    n0 = [case["N"] for case in sweep["cases"]]
    sig, _, owner = gil.mixed_variants([ps._sigma_grid for ps in systems])
    first = systems[0]
    plan = gil.plan_mixed_profiles(L=first.L, K=first.K, periodic=False, sigma_grids=sig, n_systems=len(systems), n_cap=max(n0),
                                   n_obs=len(np.arange(0.0, sweep["T"], 0.1)), variant_of_system=owner, n_groups=len(sweep["cases"]) * B,
                                   want_states=False, **prof_kw)
    totals = [float(sum(ms)) for ms in loop_ms]
    out = dict(cases=len(sweep["cases"]), systems=len(systems), L=first.L, T=sweep["T"], events=events, n0_min=min(n0), n0_max=max(n0), **prof_kw,
               host_loop=dict(spread(totals), kernel_ms_per_launch=[float(x) for x in np.median(np.array(loop_ms), axis=0)]),
               one_launch=spread(one_ms), one_launch_without_profiles=spread(bare_ms),
               kernel_ratio_loop_over_one=float(np.median(totals) / np.median(one_ms)),
               recording_cost=float(np.median(one_ms) / np.median(bare_ms)), same_rows=bool(same_rows(rows, loop_rows)), plan=plan)
    print(name, json.dumps({k: v for k, v in out.items() if k != "plan"}))
    return out


# ---- the unchanged entry points against the parent's build

def crc(r, keys):
    return f"{zlib.crc32(b''.join(np.ascontiguousarray(r[k]).tobytes() for k in keys)):08x}"


def unchanged_entry_points():
    """gilp_run, gilx_run and gilxm_run of the loaded library on fixed seeded inputs: REPS kernel times each after one untimed
    launch, and a CRC of what they returned.  Raw calls only, so that a parent's build can be asked the same."""
    rng = np.random.default_rng(12)

    def states(S, L, N):
        return [(rng.choice(L, size=N, replace=False), rng.choice([1, -1], size=N).astype(np.int8)) for _ in range(S)]

    base = dict(K=1, periodic=False, rate_diffusion=0.002, rate_active=5.0, times_obs=np.arange(0.0, 10.0, 0.1), T=10.0, want_states=False)
    S = 55
    small = dict(base, L=1000, betas=list(np.linspace(0, 3, S)), states=states(S, 1000, 750))
    owner = [s % 3 for s in range(S)]
    big = dict(base, L=8192, T=1.0, times_obs=np.arange(0.0, 1.0, 0.1), betas=list(np.linspace(0, 3, 8)), states=states(8, 8192, 6144))
    calls = {
        "gilp_run": (lambda: gil.run_profiles_raw(sigma_grid=10.0, seed=7, n_bins=250, want_field=True, group_of_system=[s % 11 for s in range(S)], **small),
                     ("ensemble_sums", "members", "n_events", "t_final")),
        "gilx_run": (lambda: gil.run_mixed_raw(sigma_grids=[10.0, 30.0, 0.0], variant_of_system=owner, seed=7, **small), ("scalars", "n_events", "t_final")),
        "gilxm_run": (lambda: gil.run_mixed_many_raw(sigma_grids=[10.0, 80.0], variant_of_system=[s % 2 for s in range(8)], seed=7, **big),
                      ("scalars", "n_events", "t_final")),
    }
    out = {}
    for name, (call, keys) in calls.items():
        r = call()
        out[name] = dict(kernel_ms=[call()["kernel_ms"] for _ in range(REPS)], crc=crc(r, keys), events=int(r["n_events"].sum()))
    return out


def against_yardstick(lib):
    """Child processes alternate between this build and the yardstick build."""
    rounds = {"this_build": [], "parent_build": []}
    for _ in range(ROUNDS):
        for which, env in (("parent_build", dict(os.environ, APS_LIB=lib)), ("this_build", {k: v for k, v in os.environ.items() if k != "APS_LIB"})):
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, check=True, capture_output=True, text=True)
            rounds[which].append(json.loads(res.stdout.strip().splitlines()[-1]))
    out = {}
    for name in rounds["this_build"][0]:
        crcs = {r[name]["crc"] for which in rounds for r in rounds[which]}
        out[name] = dict({which: spread([ms for r in rounds[which] for ms in r[name]["kernel_ms"]]) for which in rounds},
                         same_bits=len(crcs) == 1, events=rounds["this_build"][0][name]["events"])
        out[name]["median_ratio_this_over_parent"] = out[name]["this_build"]["median_ms"] / out[name]["parent_build"]["median_ms"]
    print("unchanged_entry_points", json.dumps(out))
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--child" in args:
        print(json.dumps(unchanged_entry_points()))
        sys.exit(0)
    yardstick = None
    if "--yardstick-lib" in args:
        i = args.index("--yardstick-lib")
        yardstick = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    path = args[0] if args else os.path.join(ROOT, "profiles", "exact_mixed_profiles_bench.json")
    result = dict(obs_dt=0.1, reps=REPS)
    only = os.environ.get("APS_ONLY_SWEEPS")                     # a comma-separated selection, for a call that must stay short
    for name, sweep in SWEEPS.items():
        if only is None or name in only.split(","):
            result[name] = time_sweep(name, sweep)
    if yardstick:
        result["unchanged_entry_points"] = dict(against_yardstick(yardstick), rounds=ROUNDS, reps_per_round=REPS)
    if os.path.exists(path) and only is not None:                  # a selection adds to what an earlier call wrote
        with open(path) as fh:
            result = dict(json.load(fh), **result)
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
    print("written", path)
