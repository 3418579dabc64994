"""Times what cutting a run of the exact event loop into segments costs (include/gillespie_resume.h): a launch that starts from a
checkpoint rebuilds occupancy, the field and the rates, and every launch uploads and downloads the state.  Two shapes, each as
one launch (of the entry point without a checkpoint, and of the resumable one), then the same run in 4 segments and in 20:
  sweep    the reference sweep shape (L = 1000, N = 500, T = 20, 11 beta x 32 runs), device sums, obs_dt = 0.1
  large    one system of the large-system kernel (L = 20000, N = 10000, T = 0.2, obs_dt = 0.01), states recorded
Writes profiles/exact_resume_bench.json: kernel time (HIP events, summed over the launches) and wall time of the three ways, and
whether the three gave the same numbers.  No threshold is set on any of them.
Usage (GPU box): python tools/time_exact_resume.py [out.json]"""
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

BETAS = np.linspace(0, 3, 11)
SEGMENTS = (1, 4, 20)


def sweep_systems():
    kw = dict(L=1000, xlim=1, N=500, init="fixed", scale_rates=False, periodic=False, site_capacity=1, rate_diffusion=0.002, rate_active=5,
              local_kernel_sigma=0.01, k_on=0, k_off=0, k_exit=0, seed=2026)
    return [ParticleSystem(beta=b, rng=np.random.default_rng(100 * bi + r), **kw) for bi, b in enumerate(BETAS) for r in range(32)]


def large_systems():
    return [ParticleSystem(L=20000, xlim=1, N=10000, init="fixed", scale_rates=False, periodic=False, site_capacity=1, rate_diffusion=0.3,
                           rate_active=4.0, beta=1.0, local_kernel_sigma=0.002, k_on=0, k_off=0, k_exit=0, seed=5, rng=np.random.default_rng(2))]


def same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is b
    return bool(np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True))


def time_shape(name, build, run, T, obs_dt):
    n_obs = len(np.arange(0.0, T, obs_dt))
    out, first = dict(T=T, obs_dt=obs_dt, observations=n_obs), None
    for rep in range(2):                                       # the second round is the one kept: kernels loaded
        systems = build()                                      # the entry point that knows no checkpoint
        t0 = time.perf_counter()
        plain = run(systems, T=T, obs_dt=obs_dt)
        out["plain_launch"] = dict(kernel_ms=float(systems[0].kernel_ms), wall_s=time.perf_counter() - t0)
        for n_seg in SEGMENTS:
            systems = build()
            per = -(-n_obs // n_seg)
            t0 = time.perf_counter()
            res = run(systems, T=T, obs_dt=obs_dt, obs_per_launch=per)
            wall = time.perf_counter() - t0
            if n_seg == 1:
                first = res
                out["plain_launch"]["same_as_one_launch"] = same(plain, res)
            out[f"segments_{n_seg}"] = dict(obs_per_launch=per, launches=-(-n_obs // per), kernel_ms=float(systems[0].kernel_ms), wall_s=wall,
                                            events=int(sum(ps.n_events for ps in systems)), same_as_one_launch=same(res, first))
    one = out["segments_1"]
    for n_seg in SEGMENTS[1:]:
        seg = out[f"segments_{n_seg}"]
        seg.update(kernel_ratio=seg["kernel_ms"] / one["kernel_ms"], wall_ratio=seg["wall_s"] / one["wall_s"])
    print(name, json.dumps(out))
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "exact_resume_bench.json")
    result = dict(betas=len(BETAS), runs_per_beta=32)
    result["sweep"] = time_shape("sweep", sweep_systems, gil.run_batched_exact_statistics, 20.0, 0.1)
    result["large"] = time_shape("large", large_systems, lambda s, **kw: gil.run_batched_exact(s, want_m_local=False, **kw), 0.2, 0.01)
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
    print("written", path)
