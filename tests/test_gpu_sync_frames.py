"""GPU suite (-m gpu): the fixed-dt stepper against the CPU oracle at EVERY frame height of every step kernel, bit for bit.

tile_step, tile_loop (four and eight waves) and field_update are templates over the frame height RS, one compilation each, and
the library's geometry gives every small lattice RS = 1 (field_update: R = 2): the rest of the suite meets the other
instantiations at K = 1, binary64, or at benchmark size.  Here every case of tests/sync_cases.py -- {walls, torus} x {K = 1,
K > 1} x {binary64, 32-bit field}: seeded random draws and named edges, sized per RS from own(rs) = 64 rs - 4 -- runs at
RS = 1 .. 8 (APS_TS_R, APS_FU_R) through every path that admits it:

    per_step   tile_step<BC, true, RS, K1, F32>, one launch per step (set_resident_loop(False))
    loop4      tile_loop with four waves (APS_LOOP_MIN=3, APS_LOOP_WAVES=4); WHERE the loop is eligible is written out in
               sync_cases.loop4_verdict from the rules of loop_prepare and tl_kernel_f, and what the handle reports must equal it:
               a loop that silently falls back does not pass as tested
    loop8      tile_loop with eight waves (K = 1, binary64, RS 5 .. 8)
    lattice    field_update<BC, true, rs> (method="lattice", binary64, RS >= 2)
    ensembles  ensemble 1 of two (test_second_ensemble_at_every_frame)
    windowed   tile_step<BC, false, RS, K1, F32>, tables beyond LDS with APS_NTT=0 (test_windowed_table_at_every_frame)
    site ranges  two and three handles on one device (test_site_ranges_at_forced_frames)

Bars, no tolerance anywhere: after every call pos, sigma, bound, alive equal the oracle's and check_lattice holds ({W, S,
occupancy} on all sites and the per-particle sums read from them); at the end the exit rows and time() = (steps dt, steps);
per_step, loop4 and loop8 of one (case, rs) agree on get_state() and get_lattice().  The oracle runs once per (case, rs) and is
shared by the paths (sync_cases.oracle_run).  Replaces the loop of ParticleSystem.run (PARTICLE_solver_CLASS.py:511-516)."""
import collections
import contextlib
import importlib
import os
import time

import numpy as np
import pytest

import sync_cases as X
from test_gpu_parity import _merged_state, check_lattice, make_handle

pytestmark = pytest.mark.gpu
PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"


@pytest.fixture(scope="module")
def capi():
    mod = importlib.import_module(PKG + ".capi")
    assert mod.device_count() >= 1, "no GPU visible"
    return mod


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def paths_of(case, rs):
    p = ["per_step", "loop4"]                                # (loop4 where it is not eligible: the fallback is held to the oracle too)
    if X.loop8_admits(case, rs):
        p.append("loop8")
    if X.lattice_admits(case, rs):
        p.append("lattice")
    return p


# what runs where, from the rules alone: (path, class, rs) -> items.  "loop4" counts the items the loop really takes.
PLANNED = collections.Counter()
for _c in X.all_cases():
    for _rs in X.RS_ALL:
        for _p in paths_of(_c, _rs):
            if _p != "loop4" or X.loop4_verdict(_c, _rs)[0]:
                PLANNED[(_p, _c["cls"], _rs)] += 1
MINIMUM = dict(per_step=5, loop4=2, loop8=5, lattice=5)


def loop4_has_kernel(cls, rs):
    """tl_kernel_f: no binary64 kernel of 8 rows, nor of 7 rows with more than one cell per site."""
    return not (cls[2] == "f64" and (rs == 8 or (rs == 7 and cls[1] == "kn")))


def same_state(h, snap, tag, ensemble=0):
    p, sg, bd, al = h.get_state(ensemble)
    assert np.array_equal(al, snap.alive), tag
    assert np.array_equal(p, snap.pos), tag
    assert np.array_equal(sg, snap.spin), tag
    assert np.array_equal(bd, snap.bound), tag


def same_exits(h, r, tag, ensemble=0):
    ex, ex0 = h.exits(ensemble), r["exits"]
    assert len(ex) == len(ex0), tag
    if len(ex0):
        assert np.array_equal(ex, ex0[np.lexsort((ex0[:, 2], ex0[:, 0]))]), tag


def open_handle(capi, inst, rs, method, betas=None, **kw):
    """A handle of `inst` at frame height rs (the geometry knobs are read when the handle is made)."""
    with env(APS_TS_R=rs, APS_FU_R=max(rs, 2)):
        h = make_handle(capi, inst["par"], inst["N"], dt=inst["dt"], seed=inst["seed"], method=method, fp32=inst["fp32"],
                        **(dict(beta=betas) if betas else {}), **kw)
    if inst["flip_table"] is not None:
        h.set_flip_table(inst["flip_table"])
    return h


def run_path(capi, path, case, rs, r):
    inst, tag = r["inst"], (case["tag"], rs, path)
    eligible, reason = X.loop4_verdict(case, rs)
    h = open_handle(capi, inst, rs, "lattice" if path == "lattice" else "tiles")
    try:
        h.set_state(inst["pos"], inst["spin"], bound=inst["bound"], alive=inst["alive"])
        if path != "lattice":
            info = h.tiles_info()
            assert info["frame_sites"] == 64 * rs and info["table_in_lds"] and not h.ntt_info()["on"], (tag, info)
            assert (info["owned_sites"], info["n_tiles"]) == (r["tile_sites"], r["n_tiles"]), (tag, info)
        if path == "per_step":
            h.set_resident_loop(False)
        total, looked, in_loop = 0, False, 0
        for n, snap in zip(r["calls"], r["snaps"]):
            with env(APS_LOOP_MIN=3, APS_LOOP_WAVES=8 if path == "loop8" else 4):
                h.step(n)
            total += n
            looked = looked or n >= 3
            in_loop += h.loop_info()[0]
            if path == "per_step":
                assert h.loop_info()[0] == 0, tag
            elif path in ("loop4", "loop8"):
                taken, state, why = h.loop_info()
                if path == "loop8" or eligible:
                    assert state == 1 and taken == (n if n >= 3 else 0), (tag, n, taken, state, why)
                    assert h.loop_waves() == (8 if path == "loop8" else 4), (tag, h.loop_waves())
                elif looked:
                    assert (taken, state) == (0, 0) and reason in why, (tag, n, taken, state, why, reason)
            same_state(h, snap, (tag, total))
            check_lattice(h, snap)
        t, k = h.time()
        assert k == total and t == total * inst["dt"], (tag, t, k)
        same_exits(h, r, tag)
        return h.get_state(), h.get_lattice(), in_loop
    finally:
        h.close()


@pytest.mark.parametrize("rs", X.RS_ALL)
@pytest.mark.parametrize("case", X.all_cases(), ids=lambda c: c["tag"])
def test_every_path_at_every_frame(capi, case, rs):
    before = X.ORACLE_SECONDS[0]
    r = X.oracle_run(case, rs)
    oracle_s = X.ORACLE_SECONDS[0] - before
    t0 = time.perf_counter()
    ends, ran = {}, []
    for path in paths_of(case, rs):
        ends[path] = run_path(capi, path, case, rs, r)
        # what the handle itself counted: a loop path that took no step inside the loop is listed as refused
        ran.append(path if path in ("per_step", "lattice") or ends[path][2] > 0 else path + "_refused")
        assert (ends[path][2] > 0) == (path == "loop8" or (path == "loop4" and X.loop4_verdict(case, rs)[0])), (case["tag"], rs, path, ends[path][2])
    for path in ("loop4", "loop8"):
        if path in ends:
            for x, y in zip(ends[path][0] + ends[path][1], ends["per_step"][0] + ends["per_step"][1]):
                assert np.array_equal(x, y), (case["tag"], rs, path, "against one launch per step")
    print(f"paths {case['tag']} {'/'.join(case['cls'])} rs={rs} L={r['inst']['L']} N={r['inst']['N']}: {' '.join(ran)}"
          f"  (device paths {time.perf_counter() - t0:.2f} s, oracle {oracle_s:.2f} s, oracle so far {X.ORACLE_SECONDS[0]:.1f} s)")
    # no path drops out unnoticed: what the rules plan for this class and frame height
    cls = case["cls"]
    assert PLANNED[("per_step", cls, rs)] >= MINIMUM["per_step"]
    assert (PLANNED[("loop4", cls, rs)] >= MINIMUM["loop4"]) == loop4_has_kernel(cls, rs) and (loop4_has_kernel(cls, rs) or PLANNED[("loop4", cls, rs)] == 0)
    if cls[1:] == ("k1", "f64") and rs >= 5:
        assert PLANNED[("loop8", cls, rs)] >= MINIMUM["loop8"]
    if cls[2] == "f64" and rs >= 2:
        assert PLANNED[("lattice", cls, rs)] >= MINIMUM["lattice"]
    if X.loop4_verdict(case, rs)[0]:                           # steps counted by the handle: every call of three steps or more, whole
        assert ends["loop4"][2] == sum(n for n in r["calls"] if n >= 3), (case["tag"], rs, ends["loop4"][2])


@pytest.mark.parametrize("rs", X.RS_ALL)
@pytest.mark.parametrize("case", X.ensemble_cases(), ids=lambda c: c["tag"])
def test_second_ensemble_at_every_frame(capi, case, rs):
    """E = 2 with two beta and two states in one handle (grid y = 2): ensemble 1 equals SyncOracle(..., ensemble=1), ensemble 0
    the run of the single handle; through the resident loop where it is eligible, one launch per step for the short calls."""
    runs = [X.oracle_run(case, rs, ensemble=e) for e in (0, 1)]
    insts = [r["inst"] for r in runs]
    eligible, reason = X.loop4_verdict(case, rs)
    h = open_handle(capi, insts[0], rs, "tiles", betas=[i["par"].beta for i in insts])
    try:
        for e, i in enumerate(insts):
            h.set_state(i["pos"], i["spin"], bound=i["bound"], alive=i["alive"], ensemble=e)
        assert h.tiles_info()["frame_sites"] == 64 * rs
        total = 0
        for k, n in enumerate(X.CALLS):
            with env(APS_LOOP_MIN=3, APS_LOOP_WAVES=4):
                h.step(n)
            total += n
            taken, state, why = h.loop_info()
            if eligible:
                assert state == 1 and taken == (n if n >= 3 else 0), (case["tag"], rs, n, taken, state, why)
            else:
                assert (taken, state) == (0, 0) and reason in why, (case["tag"], rs, why)
            for e in (1, 0):
                same_state(h, runs[e]["snaps"][k], (case["tag"], rs, total, e), ensemble=e)
                check_lattice(h, runs[e]["snaps"][k], ensemble=e)
        for e in (1, 0):
            same_exits(h, runs[e], (case["tag"], rs, e), ensemble=e)
        print(f"paths {case['tag']} rs={rs}: ensembles ({'loop4' if eligible else 'per_step'})")
    finally:
        h.close()


@pytest.mark.parametrize("rs", X.RS_ALL)
@pytest.mark.parametrize("case", X.window_cases(), ids=lambda c: c["tag"])
def test_windowed_table_at_every_frame(capi, case, rs):
    """tile_step<BC, false, RS, K1, F32>: a table beyond LDS swept through double-buffered windows (interior tiles between walls)
    or gathered from global memory (next to the walls, and every tile of a ring).  APS_NTT=0 when the handle is made: between
    walls the exact convolution would take such a table by default."""
    r = X.oracle_run(case, 1)                                # (one lattice for every RS)
    inst = r["inst"]
    with env(APS_NTT=0):
        h = open_handle(capi, inst, rs, "tiles")
    try:
        info = h.tiles_info()
        assert info["frame_sites"] == 64 * rs and info["table_in_lds"] == 0 and h.ntt_info()["on"] == 0, (info, h.ntt_info())
        tab, q = h.table()
        assert q == r["q"] and np.array_equal(tab, r["table"])
        h.set_state(inst["pos"], inst["spin"], bound=inst["bound"], alive=inst["alive"])
        total = 0
        for n, snap in zip(r["calls"], r["snaps"]):
            h.step(n)
            total += n
            taken, state, why = h.loop_info()
            assert taken == 0 and state in (-2, 0), (taken, state, why)     # (-2: calls shorter than the loop's minimum never ask)
            same_state(h, snap, (case["tag"], rs, total))
            check_lattice(h, snap)
        assert h.time() == (total * inst["dt"], total)
        assert not np.array_equal(h.get_state()[0], inst["pos"])
        print(f"paths {case['tag']} rs={rs}: windowed")
    finally:
        h.close()


@pytest.mark.parametrize("interval", [1, 0], ids=["every_step", "library_interval"])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("rs", X.SITE_RANGE_RS)
@pytest.mark.parametrize("case", X.site_range_cases(), ids=lambda c: c["tag"])
def test_site_ranges_at_forced_frames(capi, case, rs, world, interval):
    """Site-range shards (K = 2, exits) at frames of 2, 5 and 8 rows, `world` handles on one device driven as in
    tests/test_gpu_parity.py::test_site_sharded_tiles_equal_single_handle: propose, the halo copied from the neighbour
    handles when it is due, commit.  The merged state equals the oracle after every block of 20 steps, every particle is owned
    by exactly one rank, and the ranks' exit rows add up to the oracle's."""
    r = X.oracle_run(case, rs)
    inst, N, periodic = r["inst"], r["inst"]["N"], r["inst"]["periodic"]
    ranks = [open_handle(capi, inst, rs, "tiles", rank=q, world=world, halo_interval=interval) for q in range(world)]
    try:
        k = ranks[0].halo_info()[0]
        assert k == interval if interval else k >= 1
        bounds = [h.owned_sites() for h in ranks]
        assert bounds[0][0] == 0 and bounds[-1][1] == inst["L"] and all(a[1] == b[0] for a, b in zip(bounds[:-1], bounds[1:]))
        for h in ranks:
            assert h.tiles_info()["frame_sites"] == 64 * rs and h.tiles_info()["n_tiles"] == r["n_tiles"]
            h.set_state(inst["pos"], inst["spin"], bound=inst["bound"], alive=inst["alive"])
        total = 0
        for n, snap in zip(r["calls"], r["snaps"]):
            for _ in range(n):
                for h in ranks:
                    h.propose()
                due = ranks[0].halo_info()[2]
                assert all(h.halo_info()[2] == due for h in ranks)
                for q, h in enumerate(ranks):
                    nb = {(q - 1) % world, (q + 1) % world} if periodic else {p for p in (q - 1, q + 1) if 0 <= p < world}
                    for p in sorted(nb) if due else []:
                        h.halo_from(ranks[p])
                for h in ranks:
                    h.commit()
            total += n
            p, s, b, a, seen = _merged_state(ranks, N)
            assert np.array_equal(seen, np.ones(N, int)), (case["tag"], rs, world, total)
            assert np.array_equal(a, snap.alive) and np.array_equal(p, snap.pos), (case["tag"], rs, world, total)
            assert np.array_equal(s, snap.spin) and np.array_equal(b, snap.bound), (case["tag"], rs, world, total)
        ex, ex0 = np.concatenate([h.exits() for h in ranks]), r["exits"]
        assert len(ex0) > 10 and len(ex) == len(ex0)
        assert np.array_equal(ex[np.lexsort((ex[:, 2], ex[:, 0]))], ex0[np.lexsort((ex0[:, 2], ex0[:, 0]))])
        print(f"paths {case['tag']} rs={rs}: site ranges world={world} interval={k}")
    finally:
        for h in ranks:
            h.close()
