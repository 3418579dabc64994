"""Times the two sweeps of the reference's drivers that vary the interaction range or the particle number, under the exact
dynamics with device sums, once as the host loop (one launch per sigma / per N) and once as ONE mixed launch
(include/gillespie_mixed.h):
  sigma sweep   PARTICLE_solver_BIOLOGY_EXCLUSION_sweep_beta_2.py:1277-1284   9 sigma x 11 beta x 5 runs, T = 20
  double sweep  PARTICLE_solver_BIOLOGY_EXCLUSION_double_sweep.py:851-861     19 N x 11 beta x 4 runs, T = 10, Poisson initial state
both at L = 1000, obs_dt = 0.1.  Writes profiles/exact_mixed_bench.json: kernel time (HIP events) and wall time of both ways,
whether both ways gave the same rows, the plan of the mixed launch, and the event rate of an N = 50 system launched alone
against the same system in a mixed launch that has the 950 slots of the N = 50 ... 950 batch.
Usage (GPU box): python tools/time_exact_mixed.py [out.json]"""
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

L = 1000
BETAS = np.linspace(0, 3, 11)


def exp_profile(total, decay):
    """x -> expected particles per site for an exponential profile holding `total` particles on [0, 1)."""
    x = (np.arange(L) + 0.5) / L
    w = np.exp(-x / decay)
    w *= total / w.sum()
    return lambda xx: float(w[min(L - 1, int(xx * L))])


def poisson(n, decay):
    return dict(init="poisson", rho0_plus=exp_profile(0.75 * n, decay), rho0_minus=exp_profile(0.25 * n, decay))


COMMON = dict(L=L, xlim=1, scale_rates=False, periodic=False, site_capacity=1, k_on=0, k_off=0, k_exit=0, seed=2026)
SIGMAS = [1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 3e-2, 0.1, 0.3, 0]
NUMBERS = [int(n) for n in np.linspace(50, 950, 19)]
SWEEPS = {
    "sigma_sweep": dict(T=20.0, runs=5, cases=[(dict(COMMON, rate_diffusion=0.002, rate_active=5, local_kernel_sigma=s), poisson(500, 0.35))
                                              for s in SIGMAS], labels=SIGMAS),
    "double_sweep": dict(T=10.0, runs=4, cases=[(dict(COMMON, rate_diffusion=0.005, rate_active=10, local_kernel_sigma=0.02), poisson(n, 0.2))
                                               for n in NUMBERS], labels=NUMBERS),
}


def build(sweep):
    """The systems of a sweep in the order of the host loop (case, beta, run), and the case of each."""
    systems, group = [], []
    for ci, (ps_kwargs, init_kwargs) in enumerate(sweep["cases"]):
        for bi, beta in enumerate(BETAS):
            for r in range(sweep["runs"]):
                systems.append(ParticleSystem(beta=beta, rng=np.random.default_rng(100000 * ci + 100 * bi + r), **ps_kwargs, **init_kwargs))
                group.append(ci)
    return systems, group


def same_rows(a, b):
    return all(set(x) == set(y) and all(np.array_equal(np.asarray(x[k], float), np.asarray(y[k], float), equal_nan=True) for k in x)
               for x, y in zip(a, b))


def time_sweep(name, sweep):
    run_kw = dict(T=sweep["T"], obs_dt=0.1)
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
    rows = gil.run_batched_exact_statistics_mixed(systems, groups=group, **run_kw)
    one_wall = time.perf_counter() - t0
    one_ms = systems[0].kernel_ms
    n0 = [len(ps.init_particles()[0]) for ps in build(sweep)[0]]       # the particle numbers (fresh systems: same seeds, same states)
    sig, _, owner = gil.mixed_variants([ps._sigma_grid for ps in systems])
    plan = gil.plan_mixed(L=L, K=1, periodic=False, sigma_grids=sig, n_systems=len(systems), n_cap=max(n0), n_obs=len(np.arange(0.0, sweep["T"], 0.1)),
                          variant_of_system=owner, want_states=False)
    out = dict(cases=len(sweep["cases"]), systems=len(systems), T=sweep["T"], events=events, n0_min=min(n0), n0_max=max(n0),
               host_loop=dict(kernel_ms=float(sum(loop_ms)), kernel_ms_per_launch=[float(x) for x in loop_ms], wall_s=loop_wall),
               one_launch=dict(kernel_ms=float(one_ms), wall_s=one_wall, events=int(sum(ps.n_events for ps in systems))),
               kernel_ratio=float(one_ms / sum(loop_ms)), wall_ratio=one_wall / loop_wall, same_rows=bool(same_rows(rows, loop_rows)), plan=plan)
    print(name, json.dumps({k: v for k, v in out.items() if k != "plan"}))
    return out


def small_system_rate():
    """An N = 50 system alone (gil_run_batch, 50 slots) and in a mixed launch with the 950 slots of the N = 50 ... 950 batch."""
    rng = np.random.default_rng(3)
    state = (rng.choice(L, size=50, replace=False), rng.choice([1, -1], size=50).astype(np.int8))
    kw = dict(L=L, K=1, periodic=False, rate_diffusion=0.005, rate_active=10, betas=[1.5], states=[state], times_obs=np.arange(0.0, 10.0, 0.1),
              T=10.0, want_states=False)
    res = {}
    for rep in range(2):                                           # the second round is the one kept: kernels loaded
        alone = gil.run_raw(sigma_grid=20.0, seed=11, **kw)
        wide = gil.run_mixed_raw(sigma_grids=[20.0], variant_of_system=[0], seeds=[11], streams=[0], n_cap=950, **kw)
        assert np.array_equal(alone["scalars"], wide["scalars"]) and int(alone["n_events"][0]) == int(wide["n_events"][0])
        res = dict(events=int(alone["n_events"][0]), alone_kernel_ms=alone["kernel_ms"], in_batch_kernel_ms=wide["kernel_ms"],
                   alone_events_per_ms=int(alone["n_events"][0]) / alone["kernel_ms"],
                   in_batch_events_per_ms=int(wide["n_events"][0]) / wide["kernel_ms"])
    print("small_system", json.dumps(res))
    return res


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "exact_mixed_bench.json")
    result = dict(L=L, obs_dt=0.1, betas=len(BETAS))
    result["small_system"] = small_system_rate()                  # also loads both kernels before the sweeps are timed
    for name, sweep in SWEEPS.items():
        result[name] = time_sweep(name, sweep)
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
    print("written", path)
