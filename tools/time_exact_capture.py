"""Exact event loop with anchor-capture and cluster statistics taken on the device (gilc_run): what recording costs, and
ensemble.capture_study from device counts against the same study over full outputs.  The shape is the reference driver's own
(PARTICLE_solver_BIOLOGY_EXCLUSION.py) with its commented-out anchors switched on: L = 1000, N = 750, K = 3, sigma = 0.002,
walls, rate_active = 5, rate_diffusion = 0, scale_rates = False, anchors at 0.25 / 0.60 / 0.80 with radius 0.003, k_on = 20,
k_off = 5, k_exit = 30, T = 20, 256 systems, with obs_dt = 0.5 and obs_dt = 0.05; then one large-shape size: 8 systems of
L = 4200, N = 2000.

    python tools/time_exact_capture.py [--repeats 3] [--only batch_dt05,batch_dt005,large] [--yardstick-lib PATH]
                                       [--out profiles/exact_capture_bench.json]

(a) kernel_ms of gilc_run (want_states=False) against gil_run_batch / gilm_run on the same inputs, taken alternately: `repeats`
    pairs after one warm-up pair; best and spread (max - min) of each side.  `--yardstick-lib`: a libaps_hip.so built from the
    parent commit; its gil_run_batch / gilm_run is then timed as well, in a child process of its own (APS_LIB), so that the
    yardstick is not the code under test.
(b) wall time of ensemble.capture_study with on_device=True against on_device=False (batch sections; 32 runs).
A section whose output file exists is kept, so the sections can run as separate processes, each under a time limit of its own."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"
gil = importlib.import_module(PKG + ".gillespie")
obs = importlib.import_module(PKG + ".observables")
psys = importlib.import_module(PKG + ".particle_system")
ens = importlib.import_module(PKG + ".ensemble")

DRIVER = dict(xlim=1, rate_diffusion=0, rate_active=5, beta=1.0, scale_rates=False, local_kernel_sigma=0.002, minus_anchor=True, periodic=False,
              site_capacity=3, anchor_positions=[0.25, 0.60, 0.80], anchor_radius=0.003, k_on=20, k_off=5, k_exit=30, seed=1)
SECTIONS = {
    "batch_dt05": dict(L=1000, N=750, n_systems=256, T=20.0, obs_dt=0.5, study_runs=32),
    "batch_dt005": dict(L=1000, N=750, n_systems=256, T=20.0, obs_dt=0.05, study_runs=32),
    "large": dict(L=4200, N=2000, n_systems=8, T=20.0, obs_dt=0.5, study_runs=0),
}
C_BINS, H_BINS = 16, 40


def inputs(sec, plan=True):
    sy = [psys.ParticleSystem(L=sec["L"], init="fixed", N=sec["N"], rng=np.random.default_rng(100 + i), **DRIVER) for i in range(sec["n_systems"])]
    first = sy[0]
    times = np.arange(0.0, sec["T"], sec["obs_dt"])
    kw = dict(L=first.L, K=first.K, periodic=first.periodic, sigma_grid=first._sigma_grid, rate_diffusion=first.rate_diffusion,
              rate_active=first.rate_active, betas=[float(ps.beta) for ps in sy], states=[ps.init_particles() for ps in sy], times_obs=times,
              T=sec["T"], seed=1, minus_anchor=first.minus_anchor, immobilize=first.immobilize_when_anchored,
              suppress_flip=first.suppress_flip_when_bound, crowding=first.crowding_suppresses_rates, k_on=first.k_on, k_off=first.k_off,
              k_exit=first.k_exit, anchor_mask=first.is_anchor_site, want_states=False)
    plan = plan and gil.plan_capture(L=first.L, K=first.K, periodic=False, sigma_grid=first._sigma_grid, n_systems=len(sy), n_cap=sec["N"],
                            n_obs=len(times), n_groups=3, c_bins=C_BINS, h_bins=H_BINS, want_states=False)
    return first, kw, plan


def best_and_spread(runs):
    return dict(best=min(runs), spread=max(runs) - min(runs), runs=runs)


def plain_only(name, repeats, shape):
    """The child of --yardstick-lib: gil_run_batch / gilm_run of the library APS_LIB names (which need not know gilc_plan: the
    parent passes the shape), one warm-up and `repeats` runs."""
    _, kw, _ = inputs(SECTIONS[name], plan=False)
    entry = gil.run_raw if shape == 0 else gil.run_many_large_raw
    entry(**kw)
    print(json.dumps([entry(**kw)["kernel_ms"] for _ in range(repeats)]))


def section(name, repeats, yardstick_lib):
    sec = SECTIONS[name]
    first, kw, plan = inputs(sec)
    plain_entry = gil.run_raw if plan["shape"] == 0 else gil.run_many_large_raw
    groups = obs.anchor_groups(first)
    cap, plain, events, exits = [], [], 0, 0
    for it in range(repeats + 1):                                  # alternately; the first pair warms up
        r = gil.run_capture_raw(group_of_site=groups, c_bins=C_BINS, h_bins=H_BINS, **kw)
        p = plain_entry(**kw)
        assert np.array_equal(r["n_events"], p["n_events"]) and np.array_equal(r["scalars"], p["scalars"])
        events, exits = int(r["n_events"].sum()), int(r["n_exits"].sum())
        if it:
            cap.append(r["kernel_ms"])
            plain.append(p["kernel_ms"])
    res = dict(shape=dict(sec, n_obs=len(kw["times_obs"]), kernel_shape=plan["shape"], threads=plan["threads"], lds_bytes=plan["lds_bytes"]),
               kernel_ms_capture=best_and_spread(cap), kernel_ms_plain=best_and_spread(plain), events=events, exits=exits,
               binds=int(r["capture"][:, -1, 2].sum()), lifetimes_counted=int(r["life_hist"].sum()))
    res["recording_share"] = res["kernel_ms_capture"]["best"] / res["kernel_ms_plain"]["best"] - 1.0
    line = (f"{name}: kernel {res['kernel_ms_capture']['best']:.1f} ms with capture, {res['kernel_ms_plain']['best']:.1f} ms without "
            f"(+{res['recording_share']:.1%}), {events} events, {exits} exits")
    if yardstick_lib:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", name, "--plain-shape", str(plan["shape"]), "--repeats", str(repeats)],
                               env=dict(os.environ, APS_LIB=os.path.abspath(yardstick_lib)), capture_output=True, text=True, timeout=600, check=True)
        res["kernel_ms_plain_parent_build"] = best_and_spread(json.loads(child.stdout.strip().splitlines()[-1]))
        res["recording_share_against_parent_build"] = res["kernel_ms_capture"]["best"] / res["kernel_ms_plain_parent_build"]["best"] - 1.0
        line += f"; parent build {res['kernel_ms_plain_parent_build']['best']:.1f} ms (+{res['recording_share_against_parent_build']:.1%})"
    if sec["study_runs"]:
        study = dict(ps_kwargs=dict(DRIVER, L=sec["L"]), init_kwargs=dict(init="fixed", N=sec["N"]), n_runs=sec["study_runs"],
                     run_kwargs=dict(T=sec["T"], obs_dt=sec["obs_dt"]), rng_seeds=list(range(500, 500 + sec["study_runs"])), c_bins=C_BINS)
        wall = {True: [], False: []}
        for it in range(repeats + 1):
            for on_device in (True, False):
                t0 = time.perf_counter()
                out = ens.capture_study(on_device=on_device, **study)
                assert out["n_runs"] == sec["study_runs"]
                if it:
                    wall[on_device].append(time.perf_counter() - t0)
        res["wall_s_study_on_device"], res["wall_s_study_full_outputs"] = best_and_spread(wall[True]), best_and_spread(wall[False])
        res["wall_ratio"] = res["wall_s_study_full_outputs"]["best"] / res["wall_s_study_on_device"]["best"]
        line += f"; study of {sec['study_runs']} runs {res['wall_s_study_on_device']['best']:.2f} s against {res['wall_s_study_full_outputs']['best']:.2f} s over full outputs"
    print(line, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=",".join(SECTIONS))
    ap.add_argument("--yardstick-lib", default=None)
    ap.add_argument("--plain-only", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--plain-shape", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_capture_bench.json"))
    a = ap.parse_args()
    if a.plain_only:
        return plain_only(a.plain_only, a.repeats, a.plain_shape)
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            res = json.load(fh)
    for name in a.only.split(","):
        res[name] = section(name, a.repeats, a.yardstick_lib)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
