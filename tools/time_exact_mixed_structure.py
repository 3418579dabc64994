"""Times the pattern study over the interaction range under the exact dynamics (include/gillespie_mixed_structure.h), at the
reference's structure shape (PARTICLE_solver_BIOLOGY_local_structure.py:671-753: L = 1000, N = 900, K = 1, all L modes, T = 40)
over nine widths x 11 beta x 5 runs, with obs_dt = 1 and obs_dt = 0.1, three ways:
  window     ONE mixed launch, the window sums reduced on the device, no rows       (run_batched_exact_structure_mixed, reduce="device")
  rows       the same launch with the full rows, reduced on the host                (reduce="rows")
  host_loop  nine gils_run launches, one per width, each followed by the host reduction (run_batched_exact_structure)
Writes profiles/exact_mixed_structure_bench.json: per way the kernel time (HIP events around the launches) and the wall time
(perf_counter around the public function, systems built outside), the bytes copied back (counted for the mixed launch, by arithmetic for the host loop; `bytes_back_how` says which), and whether the ways agree.  Every
figure is the median of `repeats` runs; both kernels are loaded by a small launch before the clock counts.  A section whose
entry exists in the output file is kept, so the sections can run as separate processes, each under a time limit of its own.

    python tools/time_exact_mixed_structure.py [--repeats 1] [--only dt1,dt01] [--out profiles/exact_mixed_structure_bench.json]"""
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

L, N, T, RUNS, START = 1000, 900, 40.0, 5, 0.5
BETAS = np.linspace(0.0, 3.0, 11)
SIGMAS = [1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 3e-2, 0.1, 0.3, 0]      # the widths of the reference's sigma sweep (..._sweep_beta_2.py:1277-1284)
SECTIONS = {"dt1": 1.0, "dt01": 0.1}
KW = dict(L=L, xlim=1, rate_diffusion=0.05, rate_active=5, init="fixed", N=N, scale_rates=False, minus_anchor=True, periodic=False,
          site_capacity=1, k_on=0, k_off=0, k_exit=0, seed=1)    # the driver's constructor keywords (ref :694-714)


def build():
    """The systems in the order of the host loop (width, beta, run) and the width of each."""
    systems, group = [], []
    for si, sigma in enumerate(SIGMAS):
        for bi, beta in enumerate(BETAS):
            for r in range(RUNS):
                systems.append(psys.ParticleSystem(beta=float(beta), local_kernel_sigma=sigma, rng=np.random.default_rng(100 * bi + r), **KW))
                group.append(si)
    return systems, group


def rows_bytes(n_systems, n_obs):
    """What run_batched_exact_structure's launch copies back, by arithmetic (the function keeps its raw arrays to itself): the
    output arrays of run_structure_raw without states -- scalars, counts, times, exit log, rows."""
    return n_systems * (n_obs * gil.NSCALARS * 8 + 4 + 8 + 8 + N * 24 + 4 + n_obs * (4 + 2 * L) * 8)


def close(a, b):
    keys = ("var_mean", "var_std", "low_k_power", "m_local_var", "lowk_variance")
    return bool(all(np.allclose([x[k] for k in keys], [y[k] for k in keys], rtol=1e-9, atol=1e-12) and
                    np.allclose(x["fft_mean"], y["fft_mean"], rtol=1e-9) and np.allclose(x["fft_std"], y["fft_std"], rtol=1e-8, atol=1e-9)
                    for x, y in zip(a, b)))


def section(obs_dt, repeats):
    per, n_obs = len(BETAS) * RUNS, len(np.arange(0.0, T, obs_dt))
    kept = {}

    def mixed(reduce):
        systems, group = build()
        t0 = time.perf_counter()
        rows = gil.run_batched_exact_structure_mixed(systems, T=T, obs_dt=obs_dt, start_fraction=START, groups=group, reduce=reduce)
        wall = time.perf_counter() - t0
        kept[reduce] = rows
        return dict(kernel_ms=systems[0].kernel_ms, wall_s=wall, bytes_back=systems[0].bytes_back, bytes_back_how="counted: nbytes of the arrays the call copied back", events=int(sum(ps.n_events for ps in systems)))

    def host_loop():
        systems, _ = build()
        t0 = time.perf_counter()
        rows, ms = [], []
        for si in range(len(SIGMAS)):
            mine = systems[si * per:(si + 1) * per]
            rows += gil.run_batched_exact_structure(mine, T=T, obs_dt=obs_dt, start_fraction=START)
            ms.append(mine[0].kernel_ms)
        wall = time.perf_counter() - t0
        kept["host_loop"] = rows
        return dict(kernel_ms=float(sum(ms)), kernel_ms_per_launch=[float(x) for x in ms], wall_s=wall,
                    bytes_back=len(SIGMAS) * rows_bytes(per, n_obs), bytes_back_how="arithmetic: sizes of gils_run's output arrays", events=int(sum(ps.n_events for ps in systems)))

    def median_of(fn):
        runs = [fn() for _ in range(repeats)]
        out = dict(runs[-1])
        for key in ("kernel_ms", "wall_s"):
            out[key] = statistics.median(r[key] for r in runs)
            out[key + "_runs"] = [r[key] for r in runs]
        return out

    res = dict(shape=dict(L=L, N=N, T=T, obs_dt=obs_dt, n_obs=n_obs, widths=len(SIGMAS), betas=len(BETAS), runs=RUNS, systems=len(SIGMAS) * per,
                          k_max=L, start_fraction=START))
    res["window"] = median_of(lambda: mixed("device"))
    res["rows"] = median_of(lambda: mixed("rows"))
    res["host_loop"] = median_of(host_loop)
    res["window_agrees_with_rows"] = close(kept["device"], kept["rows"])
    res["window_agrees_with_host_loop"] = close(kept["device"], kept["host_loop"])
    res["kernel_ratio_window_to_host_loop"] = res["window"]["kernel_ms"] / res["host_loop"]["kernel_ms"]
    res["wall_ratio_window_to_host_loop"] = res["window"]["wall_s"] / res["host_loop"]["wall_s"]
    res["wall_ratio_window_to_rows"] = res["window"]["wall_s"] / res["rows"]["wall_s"]
    print(f"obs_dt {obs_dt}: window {res['window']['kernel_ms']:.0f} ms kernel, {res['window']['wall_s']:.2f} s wall, {res['window']['bytes_back']} bytes; "
          f"rows {res['rows']['kernel_ms']:.0f} ms, {res['rows']['wall_s']:.2f} s, {res['rows']['bytes_back']} bytes; "
          f"host loop {res['host_loop']['kernel_ms']:.0f} ms, {res['host_loop']['wall_s']:.2f} s, {res['host_loop']['bytes_back']} bytes", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--only", default=",".join(SECTIONS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_mixed_structure_bench.json"))
    a = ap.parse_args()
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            res = json.load(fh)
    tiny = [(np.array([3, 9]), np.array([1, -1], np.int8))]        # both kernels loaded before the clock counts
    common = dict(L=L, K=1, periodic=False, rate_diffusion=0.05, rate_active=5.0, betas=[1.0], states=tiny, times_obs=np.arange(0.0, 1.0, 0.5),
                  T=1.0, want_states=False, k_max=L)
    gil.run_structure_raw(sigma_grid=5.0, **common)
    gil.run_mixed_structure_raw(sigma_grids=[5.0], variant_of_system=[0], **common)
    for name in a.only.split(","):
        res[name] = section(SECTIONS[name], a.repeats)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
