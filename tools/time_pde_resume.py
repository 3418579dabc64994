"""Times the PDE solver run in segments (include/pde_resume.h) against the single launch, and the three unchanged entry points
against an older build of the library.

    python tools/time_pde_resume.py [--steps 4000] [--wide-steps 200] [--repeats 5] [--parent-lib OLD/libaps_hip.so] [--json OUT.json]

Two shapes:
    sweep    the reference's beta sweep (IMEX_PDE_solver_run_sweep.py): 11 beta x 3 seeded runs, L = 1000, 1000 tracers, dt = 5e-4,
             one workgroup per system (pde_solve_batch / pder_solve; the same systems through pdek_solve / pdekr_solve)
    wide     one system of L = 131 072 sites on the wide shape, kernel_sigma = 0.005 (a reach of 5798 sites), no tracers: the case
             of profiles/pde_wide_bench.json (pdew_solve / pdewr_solve)
Per shape the same call runs as one launch and with steps_per_launch = steps / 4 and steps / 20.  A cut costs one more evaluation
of the magnetisation and the state's way to the host and back: `kernel_ms` (the library's events around each launch, summed over
the segments) shows the first, `wall_ms` (a host clock around the whole Python call, which ends in the downloads) both.

With --parent-lib the three entry points that did not change (pde_solve_batch, pdek_solve, pdew_solve) are timed through that
build and through this one, alternately, on the same shapes.  Every way is run once to warm up and then `repeats` times in turn
with the others; a row carries the median and the spread (worst - best) of its way, the comparison the parent's own spread and
whether the difference of the medians exceeds three times it."""
import argparse
import ctypes as C
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
BETAS = np.linspace(0.0, 5.0, 11)


def load_parent(pde, path):
    """An older build of the library with the three one-shot solves declared as pde._lib() declares them."""
    lib = C.CDLL(os.path.abspath(path))
    for name, e in pde.SOLVES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = C.c_int, [pde._PAR, pde._I32] + e.own + [pde._PTR] * len(pde.COMMON) + [pde._MS]
        getattr(lib, e.last_error).restype = C.c_char_p
    return lib


def sweep_systems(pde, steps, dt=5e-4, runs=3):
    model, start = None, dict(rho_p0=[], rho_m0=[], tracer_x0=[], tracer_s0=[])
    betas = []
    for beta in BETAS:
        for run in range(runs):
            s = pde.IMEXPDE(L=1000, T=(steps + 0.5) * dt, dt=dt, beta=beta, seed=run, record_fft=False, snapshot_interval=max(steps, 1))
            s.initialize(n_tracers=1000)
            assert s.nsteps == steps
            model = model or s._model()
            betas.append(float(beta))
            for k, v in s._start().items():
                start[k].append(v)
    return model, betas, {k: np.array(v) for k, v in start.items()}


def wide_system(pde, steps, dt=5e-4):
    s = pde.IMEXPDE(L=131072, xlim=1.0, T=(steps + 0.5) * dt, dt=dt, gamma=2.33e-4, lam=0.6, beta=2.0, bc="neumann", active_model="anchored_minus",
                    gaussian_kernel=True, kernel_sigma=0.005, snapshot_interval=max(steps, 1), seed=99, record_fft=False)
    s.initialize(mode="poisson", rho0=1.0, noise=0.2, n_tracers=0)
    assert s.nsteps == steps
    return s._model(), [2.0], dict(rho_p0=s.rho_p[None], rho_m0=s.rho_m[None])


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r["kernel_ms"], (time.perf_counter() - t0) * 1e3, r


def alternately(ways, repeats):
    """{name: fn} -> {name: dict(kernel_ms, wall_ms: median; *_spread: worst - best; result: of the last run)}."""
    got = {name: ([], [], []) for name in ways}
    for rep in range(repeats + 1):
        for name, fn in ways.items():
            k, w, r = timed(fn)
            got[name][2][:] = [r]
            if rep:
                got[name][0].append(k)
                got[name][1].append(w)
    return {name: dict(kernel_ms=statistics.median(k), kernel_ms_spread=max(k) - min(k), wall_ms=statistics.median(w), wall_ms_spread=max(w) - min(w),
                       result=r[0]) for name, (k, w, r) in got.items()}


def same(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k], equal_nan=True) for k in ("rho_p", "rho_m", "m_series", "var_series", "v_eff_series", "D_eff_series"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--wide-steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib")
    ap.add_argument("--json")
    a = ap.parse_args()
    pde = importlib.import_module(PKG + ".pde")
    lib = pde._lib()
    parent = load_parent(pde, a.parent_lib) if a.parent_lib else None
    out = dict(repeats=a.repeats, statistic="median of the repeats after one warm-up, the ways run in turn; spread = worst - best", shapes={})
    shapes = [("sweep", a.steps, sweep_systems(pde, a.steps), "pde_solve_batch", {}),
              ("wide", a.wide_steps, wide_system(pde, a.wide_steps), "pdew_solve", dict(workgroups="auto"))]
    for shape, steps, (model, betas, start), entry, ext in shapes:
        common = dict(model, betas=betas, seed=0, want_snapshots=False, **start, **ext)
        ways = {"one_launch": lambda: pde.solve_batch_raw(**common)}
        for parts in (4, 20):
            ways[f"{parts}_segments"] = lambda n=-(-steps // parts): pde.solve_batch_raw(**common, steps_per_launch=n)
        t = alternately(ways, a.repeats)
        one, base = t["one_launch"], t["one_launch"]["result"]
        rows = []
        for name, v in t.items():
            r = v.pop("result")
            cuts = len(r.get("kernel_ms_segments", [0])) - 1
            rows.append(dict(way=name, launches=cuts + 1, same_bits_as_one_launch=same(r, base), **v,
                             kernel_ms_over_one_launch=v["kernel_ms"] / one["kernel_ms"], wall_ms_over_one_launch=v["wall_ms"] / one["wall_ms"],
                             kernel_us_per_cut=(v["kernel_ms"] - one["kernel_ms"]) * 1e3 / max(cuts, 1),
                             wall_ms_per_cut=(v["wall_ms"] - one["wall_ms"]) / max(cuts, 1)))
            print(shape, json.dumps(rows[-1]), flush=True)
        entry_rows = []
        if parent is not None:
            entries = [(entry, 0 if ext else None, model)]
            if shape == "sweep":
                entries.append(("pdek_solve", np.full(len(betas), 0.02), dict(model, kernel_sigma=0.0)))
            for name, own, mdl in entries:
                args = dict(betas=betas, rho_p0=start["rho_p0"], rho_m0=start["rho_m0"], tracer_x0=start.get("tracer_x0"), tracer_s0=start.get("tracer_s0"),
                            rand_u=None, rand_n=None, n_fft_modes=0, seed=0, want_snapshots=False, convolution=0)
                t = alternately({"parent": lambda: pde._launch(parent, name, own, mdl, **args), "this": lambda: pde._launch(lib, name, own, mdl, **args)}, a.repeats)
                old, new = t["parent"], t["this"]
                entry_rows.append(dict(entry=name, parent_kernel_ms=old["kernel_ms"], parent_kernel_ms_spread=old["kernel_ms_spread"], kernel_ms=new["kernel_ms"],
                                       kernel_ms_spread=new["kernel_ms_spread"], ratio_to_parent=new["kernel_ms"] / old["kernel_ms"],
                                       slower_beyond_three_parent_spreads=bool(new["kernel_ms"] - old["kernel_ms"] > 3.0 * old["kernel_ms_spread"]),
                                       same_bits_as_parent=same(new["result"], old["result"])))
                print(shape, json.dumps(entry_rows[-1]), flush=True)
        out["shapes"][shape] = dict(systems=len(betas), L=model["L"], steps=steps, n_tracers=0 if "tracer_x0" not in start else int(start["tracer_x0"].shape[1]),
                                    entry=entry, segments=rows, unchanged_entry_points=entry_rows)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
