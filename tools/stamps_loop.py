"""Diagnostic: build the library with -DAPS_LOOP_STAMPS into /tmp and print where a workgroup of the resident loop
(csrc/tile_loop.hpp) spends an iteration.  Usage (GPU box): python tools/stamps_loop.py [steps] [-DAPS_...]
-DAPS_LOOP_STAMP_MASK=0x298 keeps four stamps only (barrier E .. S, sweep .. B, proposals .. D, exclusion .. E): a stamped
eight-wave kernel without scratch.  With APS_LIB (a build made beforehand) give the same -D so that the rows are named right.
Bit 12 of the mask (0x1298: the four stamps and the trace) adds the trace of the records' wait -- per wave and iteration whether the
look asked ahead found everything, the polls that followed, one poll's round trip and the cycles from barrier E to the end of the
wait -- and this tool prints the hit rate, the polls per wait and how far the arrival offset moves from one iteration to the next."""
import ctypes as C, importlib, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"
extra = sys.argv[1:]
steps = 201
if extra and not extra[0].startswith("-"):
    steps, extra = int(extra[0]) | 1, extra[1:]
lib = f"/tmp/libaps_stamps_loop_{'_'.join(x.strip('-D') for x in extra)}.so"
if os.environ.get("APS_LIB"):                      # a stamps build made beforehand (tools/build_variant.sh ... -DAPS_LOOP_STAMPS -DAPS_DEV_RS=7)
    lib = os.environ["APS_LIB"]
else:
  subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-DAPS_LOOP_STAMPS",
                "-DAPS_DEV_RS=" + os.environ.get("APS_TS_R", "5"), *extra, "-I", os.path.join(ROOT, "include"), "-o", lib,
                os.path.join(ROOT, PKG, "csrc", "aps_hip.hip")], check=True)
capi = importlib.import_module(PKG + ".capi")
capi.LIB_PATH = lib
import bench
w = dict(bench.WORK)
h = bench.make_handle(capi, w, method="tiles")
h.set_state(*bench.initial_state(w))
h.step(201)
t0 = time.perf_counter(); h.step(steps); dt = time.perf_counter() - t0
print("loop_info", h.loop_info(), f"{dt / steps * 1e6:.2f} us per step (wall, stamps build)")
TRACE_TILES, TRACE_STRIDE, TRACE_ITERS = 64, 8, 256          # tile_loop.hpp: TL_TRACE_*
buf = np.zeros(8 * 4096 + TRACE_TILES * 8 * TRACE_ITERS, dtype=np.uint64)
fn = h.lib.aps_debug_stamps
fn.restype = C.c_int
fn(h._h, buf.ctypes.data_as(C.c_void_p), C.c_int64(len(buf)))
NW = h.loop_waves() or 4                                     # waves per tile of the kernel that ran (APS_LOOP_WAVES=4|8 forces the choice)
trace, buf = buf[8 * 4096:], buf[:8 * 4096]
allw = buf.reshape(-1, NW, 16).astype(float) / steps         # [tile][wave][16]
idxt = np.flatnonzero(allw[:, 0, 6] > 0)
allw = allw[idxt]
PHASES = ((2, "barrier F + random numbers"), (0, "wait for the records"), (8, "intake (pooling)"), (9, "barrier S"), (10, "sweep"), (11, "ds_add into the field"),
          (7, "barrier B"), (3, "proposals (D)"), (4, "exclusion (E)"), (5, "hand over + ask ahead"))       # in the order of an iteration
mask = 0xFFF
for x in extra:
    if x.startswith("-DAPS_LOOP_STAMP_MASK="):
        mask = int(x.split("=", 1)[1], 0)
# a stamp that the build leaves out gives its time to the next one kept (around the end of the iteration too)
kept = [i for i, (k, _) in enumerate(PHASES) if (mask >> k) & 1]
NAMES = []
for n, i in enumerate(kept):
    j, parts = kept[n - 1], []
    while j != i:
        j = (j + 1) % len(PHASES)
        parts.append(PHASES[j][1])
    NAMES.append((PHASES[i][0], " + ".join(parts) if mask != 0xFFF else PHASES[i][1]))
NAMES.append((6, "total"))
print("workgroups", len(allw), f"of {NW} waves; cycles per iteration (s_memtime), per wave: mean over tiles [wave 0 .. {NW - 1}]")
for k, name in NAMES:
    label = f"  {name:28s} " if mask == 0xFFF else f"  {name}\n  {'':28s} "
    print(label + "  ".join(f"{allw[:, wv, k].mean():9.1f}" for wv in range(NW)) + f"   | max over waves, mean over tiles {allw[:, :, k].max(axis=1).mean():9.1f}")
if mask == 0xFFF:                                            # (per-tile waits and intake .. sweep need the stamps 0 and 8 .. 11 of their own)
    st = np.zeros((len(allw), 8))
    st[:, :8] = allw[:, 0, :8]
    idx = idxt
    for k, name in ((1, "intake, barrier S, sweep (wave 0)"),):
        print(f"  {name:24s} mean {st[:, k].mean():9.1f}   median {np.median(st[:, k]):9.1f}   min {st[:, k].min():9.1f}   max {st[:, k].max():9.1f}")
    worst = np.argsort(-st[:, 1])[:8]
    print("  longest intake .. sweep: tiles", idx[worst], st[worst, 1].round(0), " their waits", st[worst, 0].round(0))
    best = np.argsort(st[:, 0])[:8]
    print("  shortest waits: tiles", idx[best], st[best, 0].round(0), "their intake+sweep", st[best, 1].round(0))
if (mask >> 12) & 1:                                         # the trace of the wait: [slot][wave][iteration], iteration 0 has no wait
    n_it = min(steps, TRACE_ITERS)
    tr = trace[:TRACE_TILES * NW * TRACE_ITERS].reshape(TRACE_TILES, NW, TRACE_ITERS)[:, :, 3:n_it]   # (the first iterations: the grid is still starting)
    tr = tr[(tr != 0).all(axis=(1, 2))]
    hit, polls = (tr & np.uint64(1)).astype(bool), ((tr >> np.uint64(1)) & np.uint64(0x7FFF)).astype(np.int64)
    rt, off = ((tr >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64), (tr >> np.uint64(32)).astype(np.int64)
    pct = lambda v, q: np.percentile(v, q)
    print(f"trace of the wait: {tr.shape[0]} tiles (every {TRACE_STRIDE}th) x {NW} waves x {tr.shape[2]} iterations")
    print(f"  look asked ahead found everything: {hit.mean() * 100:6.2f} % of the waits   by wave: " + "  ".join(f"{hit[:, wv].mean() * 100:5.1f}" for wv in range(NW)))
    hist = np.bincount(np.minimum(polls.ravel(), 8), minlength=9) / polls.size * 100
    print("  polls after it until the wait ended (%):  " + "  ".join(f"{k if k < 8 else '8+'}: {hist[k]:5.2f}" for k in range(9)))
    print(f"  mean {polls.mean():.3f}; of a workgroup's slowest wave (what barrier S sees): mean {polls.max(axis=1).mean():.3f}, two or more in {(polls.max(axis=1) >= 2).mean() * 100:.2f} % of the iterations")
    r1 = rt[polls >= 1]
    if r1.size:
        print(f"  round trip of the first poll (cycles): median {np.median(r1):.0f}   10 % {pct(r1, 10):.0f}   90 % {pct(r1, 90):.0f}   -> a poll period of about {np.median(r1) + 1024:.0f} with 16 sleeps")
    print(f"  barrier E -> end of the wait (cycles): mean {off.mean():.0f}   median {np.median(off):.0f}   10 % {pct(off, 10):.0f}   90 % {pct(off, 90):.0f}")
    wg = off.max(axis=1)                                     # [tile][iteration]: the wave that ends last
    sd, rng = wg.std(axis=1), np.percentile(wg, 95, axis=1) - np.percentile(wg, 5, axis=1)
    print(f"  spread over the iterations of a tile (slowest wave): standard deviation median {np.median(sd):.0f}, largest {sd.max():.0f};  5 % .. 95 % range median {np.median(rng):.0f}, largest {rng.max():.0f}")
    d1 = np.abs(np.diff(wg, axis=1))
    print(f"  change from one iteration to the next: median {np.median(d1):.0f}   90 % {pct(d1, 90):.0f}   99 % {pct(d1, 99):.0f}   (what a lead carried from the last iteration is off by)")
    print("  by polls, barrier E -> end of the wait (mean cycles): " + "  ".join(f"{k}: {off[polls == k].mean():.0f}" for k in range(5) if (polls == k).any()))
h.close()
