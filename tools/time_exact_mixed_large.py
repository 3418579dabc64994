"""Times the two sweeps of the reference's drivers that vary the interaction range or the particle number at a LARGE shape
(L = 8192: the large-system kernel, one 1024-thread workgroup per system), under the exact dynamics with device sums, once as
the host loop (one gilm_run launch per sigma / per N) and once as ONE mixed launch (include/gillespie_mixed_many.h):
  sigma sweep   PARTICLE_solver_BIOLOGY_EXCLUSION_sweep_beta_2.py:1277-1284   9 sigma x 11 beta x 5 runs, N = 6144
  double sweep  PARTICLE_solver_BIOLOGY_EXCLUSION_double_sweep.py:851-861     19 N x 11 beta x 4 runs, N = 50 ... 950 scaled by L / 1000
both with obs_dt = 0.1, a fixed particle number per run and T = 1, which keeps the whole tool under two minutes.  Writes
profiles/exact_mixed_large_bench.json: kernel time (HIP events) and wall time of both ways, whether both ways gave the same
rows, and the plan of the mixed launch.  The host loop is what the library did before the mixed launch existed: the baseline.
Usage (GPU box): python tools/time_exact_mixed_large.py [out.json]"""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"
gil = importlib.import_module(PKG + ".gillespie")
ParticleSystem = importlib.import_module(PKG + ".particle_system").ParticleSystem

L, T = 8192, 1.0
BETAS = np.linspace(0, 3, 11)
COMMON = dict(L=L, xlim=1, scale_rates=False, periodic=False, site_capacity=1, k_on=0, k_off=0, k_exit=0, seed=2026, init="fixed")
SIGMAS = [1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 3e-2, 0.1, 0.3, 0]
NUMBERS = [int(n * L / 1000) for n in np.linspace(50, 950, 19)]
SWEEPS = {
    "sigma_sweep": dict(runs=5, cases=[dict(COMMON, rate_diffusion=0.002, rate_active=5, local_kernel_sigma=s, N=6144) for s in SIGMAS]),
    "double_sweep": dict(runs=4, cases=[dict(COMMON, rate_diffusion=0.005, rate_active=10, local_kernel_sigma=0.02, N=n) for n in NUMBERS]),
}


def build(sweep):
    """The systems of a sweep in the order of the host loop (case, beta, run), and the case of each."""
    systems, group = [], []
    for ci, kw in enumerate(sweep["cases"]):
        for bi, beta in enumerate(BETAS):
            for r in range(sweep["runs"]):
                systems.append(ParticleSystem(beta=beta, rng=np.random.default_rng(100000 * ci + 100 * bi + r), **kw))
                group.append(ci)
    return systems, group


def same_rows(a, b):
    return all(set(x) == set(y) and all(np.array_equal(np.asarray(x[k], float), np.asarray(y[k], float), equal_nan=True) for k in x)
               for x, y in zip(a, b))


def time_sweep(name, sweep):
    run_kw = dict(T=T, obs_dt=0.1)
    per = len(BETAS) * sweep["runs"]
    # the host loop: one launch per case
    systems, group = build(sweep)
    t0 = time.perf_counter()
    loop_rows, loop_ms = [], []
    for ci in range(len(sweep["cases"])):
        mine = systems[ci * per:(ci + 1) * per]
        loop_rows += gil.run_batched_exact_statistics(mine, **run_kw)
        loop_ms.append(mine[0].kernel_ms)
    loop_wall = time.perf_counter() - t0
    events = int(sum(ps.n_events for ps in systems))
    # one mixed launch
    systems, group = build(sweep)
    t0 = time.perf_counter()
    rows = gil.run_batched_exact_statistics_mixed(systems, groups=group, allow_large=True, **run_kw)
    one_wall = time.perf_counter() - t0
    one_ms = systems[0].kernel_ms
    n0 = [kw["N"] for kw in sweep["cases"]]
    sig, _, owner = gil.mixed_variants([ps._sigma_grid for ps in systems])
    plan = gil.plan_mixed_many(L=L, K=1, periodic=False, sigma_grids=sig, n_systems=len(systems), n_cap=max(n0), n_obs=len(np.arange(0.0, T, 0.1)),
                               variant_of_system=owner, want_states=False)
    out = dict(cases=len(sweep["cases"]), systems=len(systems), systems_per_loop_launch=per, T=T, events=events, n0_min=min(n0), n0_max=max(n0),
               host_loop=dict(kernel_ms=float(sum(loop_ms)), kernel_ms_per_launch=[float(x) for x in loop_ms], wall_s=loop_wall),
               one_launch=dict(kernel_ms=float(one_ms), wall_s=one_wall, events=int(sum(ps.n_events for ps in systems))),
               kernel_ratio=float(one_ms / sum(loop_ms)), wall_ratio=one_wall / loop_wall, same_rows=bool(same_rows(rows, loop_rows)), plan=plan)
    print(name, json.dumps({k: v for k, v in out.items() if k != "plan"}), flush=True)
    return out


def load_kernels():
    """Both kernels loaded before the sweeps are timed."""
    tiny = [(np.array([3, 9]), np.array([1, -1], np.int8))]
    kw = dict(L=L, K=1, periodic=False, rate_diffusion=0.5, rate_active=4.0, betas=[1.0], states=tiny, times_obs=[0.0, 0.05], T=0.1, want_states=False)
    gil.run_many_large_raw(sigma_grid=20.0, seed=1, **kw)
    gil.run_mixed_many_raw(sigma_grids=[20.0], variant_of_system=[0], seed=1, **kw)


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "exact_mixed_large_bench.json")
    result = dict(L=L, obs_dt=0.1, betas=len(BETAS))
    load_kernels()
    for name, sweep in SWEEPS.items():
        result[name] = time_sweep(name, sweep)
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
    print("written", path)
