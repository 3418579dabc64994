"""Exact event loop, many large systems per launch (gilm_run): events per second and kernel time of batches of 1, 32, 256
and 512 systems of L = 10 000, N = 5 000 (beyond one workgroup's LDS), 1e5 events per system; median of three after a warm-up.

    python tools/time_exact_many.py [--events N] [--systems 1,32,256,512] [--out profiles/gillespie_many_bench.json]
    python tools/time_exact_many.py --single-loop [--loop-systems 32] [--out FILE]

--single-loop uses run_large_raw only (one launch per system, what run_batched_exact did before gilm_run): it runs on a
checkout that has no gilm_run, which makes that checkout the yardstick.  --baseline FILE copies the numbers of such a run
into the output, next to the batch's."""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gil = importlib.import_module("hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd.gillespie")

L, N = 10_000, 5_000
KW = dict(L=L, K=1, periodic=False, sigma_grid=0.005 * L, rate_diffusion=0.02, rate_active=5.0, times_obs=np.array([0.0, 1e9]), T=1e9,
          want_states=False)


def states(n):
    rng = np.random.default_rng(0)
    return [(np.sort(rng.choice(L, size=N, replace=False)).astype(np.int32), rng.choice(np.array([1, -1], np.int8), size=N)) for _ in range(n)]


def summary(ms, events):
    med = statistics.median(ms)
    return dict(kernel_ms=med, kernel_ms_runs=ms, spread=(max(ms) - min(ms)) / med, events=int(events), events_per_s=events / med * 1e3,
                us_per_event_per_system=None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=100_000)
    ap.add_argument("--systems", default="1,32,256,512")
    ap.add_argument("--single-loop", action="store_true")
    ap.add_argument("--loop-systems", type=int, default=32)
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gillespie_many_bench.json"))
    a = ap.parse_args()
    res = dict(shape=dict(L=L, N=N, sigma_grid=KW["sigma_grid"], events_per_system=a.events, beta=0.7), seed=1)
    if a.single_loop:
        sts = states(a.loop_systems)

        def one(s):
            r = gil.run_large_raw(beta=0.7, state=sts[s], seed=1 + s, max_events=a.events, **KW)
            assert r["n_events"] == a.events
            return r["kernel_ms"]
        one(0)                                                    # warm-up
        single = [one(0) for _ in range(3)]
        res["single_system"] = summary(single, a.events)
        res["single_system"]["us_per_event_per_system"] = res["single_system"]["kernel_ms"] * 1e3 / a.events
        loops = [sum(one(s) for s in range(a.loop_systems)) for _ in range(3)]
        res["looped"] = dict(systems=a.loop_systems, **summary(loops, a.events * a.loop_systems))
        print(f"single system: {res['single_system']['kernel_ms']:.1f} ms = {res['single_system']['us_per_event_per_system']:.2f} us per event "
              f"(spread {res['single_system']['spread']:.1%}); {a.loop_systems} systems one after another: {res['looped']['kernel_ms']:.1f} ms")
    else:
        res["batches"] = []
        for S in (int(v) for v in a.systems.split(",")):
            sts = states(S)

            def batch():
                r = gil.run_many_large_raw(betas=[0.7] * S, states=sts, seed=1, max_events=a.events, **KW)
                assert np.all(r["n_events"] == a.events)
                return r["kernel_ms"]
            batch()                                               # warm-up
            row = dict(systems=S, **summary([batch() for _ in range(3)], a.events * S))
            row["us_per_event_per_system"] = row["kernel_ms"] * 1e3 / a.events
            res["batches"].append(row)
            print(f"{S} systems: {row['kernel_ms']:.1f} ms, {row['events_per_s']:.3g} events/s, {row['us_per_event_per_system']:.2f} us per event "
                  f"and system (spread {row['spread']:.1%})")
        if a.baseline:
            with open(a.baseline) as fh:
                res["baseline_parent_commit"] = json.load(fh)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
