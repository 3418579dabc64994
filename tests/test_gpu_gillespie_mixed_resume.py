"""GPU suite (-m gpu): MIXED batches of the exact event loop run in segments (include/gillespie_mixed_resume.h).  A chain of
launches of gilxr_run / gilxmr_run / gilxsr_run must be, BIT FOR BIT, the one launch of the entry point that knows no checkpoint
(gilx_run / gilxm_run / gilxs_run), which is the reference in every test: positions, spins, flags, the twelve scalar sums, the
head rows, every entry of window / n_window / n_empty, event counts, the concatenated exit logs (np.array_equal) and the final
times (==).

Preconditions on the one-launch run: every observation recorded and at least two events per observation on average, per
system.  Two cases cannot meet them by their construction and state their own instead: the SLOW shape (its point is that
observations share an event: at least 10 do) and a system that empties (it stops recording when its total rate is zero)."""
import importlib
import zlib

import numpy as np
import pytest

from oracle.gillespie_numpy import GillespieOracle

pytestmark = pytest.mark.gpu
PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"
FIB_CUTS = [1, 2, 4, 7, 12, 20, 33, 54]                        # the cuts of tests/test_gpu_gillespie_resume.py, on a 60-observation grid
COMMON = ("pos", "sigma", "flags", "scalars", "n_recorded", "n_events", "n_exits")


@pytest.fixture(scope="module")
def gil():
    assert importlib.import_module(PKG + ".capi").device_count() >= 1
    return importlib.import_module(PKG + ".gillespie")


def mixed_keywords(gil, base, systems, seeds, streams, ref_obs=-1, order=None, states=None, anchor_mask=None, n_cap=None):
    """(keywords of the raw mixed entry points without times / T, initial states) of the systems (local_kernel_sigma, N, beta) on
    the oracle case `base`: system s starts from the oracle's initial condition under rng seed 17 + s and is counted with a
    blocking table of its own; every scalar sum is switched on."""
    kw = dict(xlim=1.0, scale_rates=False, k_on=0.0, k_off=0.0, k_exit=0.0)
    kw.update(base)
    inits, grids, tables, P = [], [], [], None
    for s, (sigma, N, beta) in enumerate(systems):
        orc = GillespieOracle(init="fixed", N=N, rng=np.random.default_rng(17 + s), local_kernel_sigma=sigma, beta=beta, **kw)
        inits.append(orc.init_particles())
        P = orc.par
        grids.append(P.sigma_grid if P.sigma_kernel > 0 else 0.0)
        tables.append((np.random.default_rng(zlib.crc32(b"table") + s).random((P.K + 1, P.K + 1)) > 0.4).astype(np.uint8))
    sig, tabs, owner = gil.mixed_variants(grids, tables)
    L = kw["L"]
    out = dict(L=L, K=P.K, periodic=P.periodic, sigma_grids=sig, variant_of_system=owner, block_tables=tabs, rate_diffusion=P.rate_diffusion,
               rate_active=P.rate_active, betas=[b for _, _, b in systems], minus_anchor=P.minus_anchor, immobilize=P.immobilize_when_anchored,
               suppress_flip=P.suppress_flip_when_bound, crowding=P.crowding_suppresses_rates, k_on=P.k_on, k_off=P.k_off, k_exit=P.k_exit,
               anchor_mask=P.is_anchor_site if anchor_mask is None else anchor_mask, seeds=seeds, streams=streams, order=order,
               x_wall=(3 * L) // 4, ref_obs=ref_obs, front_lo=np.maximum(np.arange(L) - 15, 0).astype(np.int32))
    if n_cap is not None:
        out["n_cap"] = n_cap
    return out, (inits if states is None else states)


def in_segments(gil, kw, states, times, T, cuts, large=False, checkpoint=None, first=0, structure=False, **more):
    """The observations first .. len(times) - 1 as a chain of launches cut before the observations `cuts`: (merged raw outputs,
    the raw outputs of every launch).  structure: through gilxsr_run; head and rows are concatenated, the window sums are the
    last checkpoint's."""
    kw = dict(kw)
    ref_abs = kw.pop("ref_obs", -1)
    edges = [first] + [c for c in cuts if first < c < len(times)] + [len(times)]
    parts = []
    for a, b in zip(edges[:-1], edges[1:]):
        ref = ref_abs - a if a <= ref_abs < b else -1
        if structure:
            r = gil.run_mixed_structure_resumable_raw(states=states, times_obs=times[a:b], T=T, obs_first=a, checkpoint=checkpoint, ref_obs=ref, **kw, **more)
        else:
            r = gil.run_mixed_resumable_raw(states=states, times_obs=times[a:b], T=T, obs_first=a, checkpoint=checkpoint, large=large, ref_obs=ref,
                                            **kw, **more)
        checkpoint = r["checkpoint"]
        parts.append(r)
    seg = gil._merge_segments(parts, first)
    if structure:
        seg.update(head=np.concatenate([r["head"] for r in parts], axis=1), window=checkpoint["window"], n_window=checkpoint["n_window"],
                   n_empty=checkpoint["n_empty"],
                   structure=None if parts[0]["structure"] is None else np.concatenate([r["structure"] for r in parts], axis=1))
    return seg, parts


def assert_equal_runs(one, seg, tag="", more=()):
    """`seg` (merged segments) against `one` (one launch): equal in every output."""
    for k in COMMON + tuple(more):
        assert np.array_equal(one[k], seg[k]), (tag, k)
    for s in range(len(one["n_exits"])):
        n = int(one["n_exits"][s])
        assert np.array_equal(one["exits"][s, :n], seg["exits"][s, :n]), (tag, "exits", s)
    assert all(a == b for a, b in zip(one["t_final"], seg["t_final"])), (tag, one["t_final"], seg["t_final"])


def require_busy(one, M, systems=None):
    """The preconditions on the one-launch run: every observation recorded, two events per observation on average."""
    pick = slice(None) if systems is None else systems
    print("n_recorded", one["n_recorded"], "n_events", one["n_events"], "of", M, "observations")
    assert np.all(one["n_recorded"][pick] == M) and np.all(one["n_events"][pick] >= 2 * M), (one["n_recorded"], one["n_events"])


# ---- 1. one wavefront: six systems, three table lengths, four slot counts, dead slots, exits, keys, a launch order

ANCHORED = dict(site_capacity=2, rate_diffusion=0.6, rate_active=4.0, anchor_positions=[0.3, 0.7], anchor_radius=0.08, k_on=3.0, k_off=1.0, k_exit=0.3)
SIX = [(0.0, 100, 0.9), (0.02, 100, 1.0), (0.2, 37, 1.1), (0.02, 37, 1.2), (0.0, 64, 1.3), (0.2, 5, 1.4)]   # (local_kernel_sigma, N, beta)
SIX_SEEDS, SIX_STREAMS = [1234, 1234, 77, 2 ** 63 + 5, 991, 992], [0, 1, 2, 2, 7, 3]   # 0, 1: one key, two streams; 2, 3: one stream, two keys
SIX_ORDER = [3, 0, 5, 1, 4, 2]
T_SIX = 15.0                                                   # long enough for the five-particle system's 120 events


@pytest.mark.parametrize("geometry", [dict(L=160), dict(L=150, periodic=True, site_capacity=1)], ids=["walls_K2", "ring_K1"])
def test_one_wavefront(gil, geometry):
    T, times = T_SIX, np.arange(60) * (T_SIX / 60)
    kw, states = mixed_keywords(gil, dict(ANCHORED, **geometry), SIX, SIX_SEEDS, SIX_STREAMS, ref_obs=5, order=SIX_ORDER)
    assert [len(p) for p, _ in states] == [100, 100, 37, 37, 64, 5] and len(kw["sigma_grids"]) >= 3
    one = gil.run_mixed_raw(states=states, times_obs=times, T=T, **kw)
    require_busy(one, 60)
    assert np.any(one["scalars"][:, 6:, 9] > 0)                # the displacement sums are on (origin: observation 5)
    seg, parts = in_segments(gil, kw, states, times, T, FIB_CUTS)
    assert len(parts) == len(FIB_CUTS) + 1
    assert_equal_runs(one, seg, geometry)
    assert np.array_equal(seg["checkpoint"]["n_slots"], [100, 100, 37, 37, 64, 5])
    if geometry["L"] == 160:                                   # exits and bound flags cross cuts (K = 1: an occupied site binds nobody)
        assert sum(int(np.sum(r["n_exits"])) > 0 for r in parts) >= 2 and np.any((one["flags"] & 1) != 0)
        assert np.any((one["flags"][0, -1] & 2) == 0)          # dead slots in the last state of a system that fills n_cap
    for r in parts:                                            # the end state beyond a system's slots is empty
        for s, n in enumerate([100, 100, 37, 37, 64, 5]):
            assert not r["checkpoint"]["pos"][s, n:].any() and not r["checkpoint"]["flags"][s, n:].any() and np.all(r["checkpoint"]["ref"][s, n:] == -1)


# ---- 2. four waves

def test_four_waves(gil):
    base = dict(L=700, site_capacity=2, rate_diffusion=0.5, rate_active=4.0)
    T, times = 1.2, np.arange(60) * 0.02                        # T = 0.3 of the uniform case gives the 70-particle system under 120 events
    kw, states = mixed_keywords(gil, base, [(0.02, 1100, 1.1), (0.005, 70, 1.2)], [1234, 1234], [0, 1], ref_obs=5)
    assert [len(p) for p, _ in states] == [1100, 70]           # n_cap beyond one wavefront's slots: the four-wave instantiations
    one = gil.run_mixed_raw(states=states, times_obs=times, T=T, **kw)
    require_busy(one, 60)
    seg, parts = in_segments(gil, kw, states, times, T, FIB_CUTS)
    assert_equal_runs(one, seg, "four waves")


# ---- 3. pending observations and the T break

SLOW = dict(L=60, site_capacity=1, rate_diffusion=1.0, rate_active=2.0)
SLOW_SYSTEMS = [(0.05, 8, 1.0), (0.0, 8, 1.1)]


def test_pending_observations_and_the_T_break(gil):
    T, times = 2.0, np.arange(0.0, 2.0, 0.02)
    kw, states = mixed_keywords(gil, SLOW, SLOW_SYSTEMS, [99, 99], [0, 1], ref_obs=3)
    one = gil.run_mixed_raw(states=states, times_obs=times, T=T, **kw)
    ev = one["scalars"][0, :int(one["n_recorded"][0]), 11]
    assert int(np.sum(ev[1:] == ev[:-1])) >= 10, ev            # observations that share their event with the one before
    seg, parts = in_segments(gil, kw, states, times, T, list(range(1, len(times))))
    assert len(parts) == len(times)
    assert_equal_runs(one, seg, "cut after every observation")
    # a run to T = 0.6, continued to T = 2.0 (each system from its own next observation), is the run to T = 2.0
    short_times = np.arange(0.0, 0.6, 0.02)
    assert np.array_equal(short_times, times[:len(short_times)])
    head = gil.run_mixed_resumable_raw(states=states, times_obs=short_times, T=0.6, **kw)
    ck = head["checkpoint"]
    assert np.array_equal(ck["next_obs"], head["n_recorded"]) and np.all(ck["t"] > 0.0)
    lo = int(ck["next_obs"].min())
    tail, _ = in_segments(gil, kw, None, times, T, [], checkpoint=ck, first=lo)
    for s in range(2):
        n, f = int(head["n_recorded"][s]), int(tail["first_row"][s])
        assert f == n - lo and tail["n_recorded"][s] == one["n_recorded"][s] - lo
        for k in ("pos", "sigma", "flags", "scalars"):
            assert np.array_equal(head[k][s, :n], one[k][s, :n]), k
            assert np.array_equal(tail[k][s, f:], one[k][s, n:]), k
            assert not np.any(tail[k][s, :f])                  # rows the first run had recorded stay untouched
    assert np.array_equal(tail["n_events"], one["n_events"]) and all(a == b for a, b in zip(tail["t_final"], one["t_final"]))


# ---- 4. a system that empties

EMPTYING = dict(L=40, site_capacity=2, rate_diffusion=1.0, rate_active=2.0, anchor_positions=[0.5], anchor_radius=0.6, k_on=50.0, k_off=0.0, k_exit=20.0)


@pytest.mark.parametrize("structure", [False, True], ids=["plain", "structure"])
def test_a_system_that_empties(gil, structure):
    T, times = 5.0, np.arange(0.0, 5.0, 0.1)
    kw, states = mixed_keywords(gil, EMPTYING, [(0.05, 3, 1.0), (0.0, 2, 1.0)], [5, 6], [0, 0])
    more = dict(k_max=8, first_obs=0, want_rows=False) if structure else {}
    one = (gil.run_mixed_structure_raw if structure else gil.run_mixed_raw)(states=states, times_obs=times, T=T, **kw, **more)
    n = int(one["n_recorded"][0])
    assert np.isinf(one["t_final"][0]) and one["n_exits"][0] == 3 and 1 <= n < 25 and one["n_events"][0] < 40
    from_inf = 0
    for cuts in ([25], [n], [1, n + 1, 30]):                   # after, at, before and after the observation where t becomes +inf
        seg, parts = in_segments(gil, kw, states, times, T, cuts, structure=structure, **more)
        assert_equal_runs(one, seg, cuts, more=("head", "window", "n_window", "n_empty") if structure else ())
        before, last = parts[-2]["checkpoint"], parts[-1]
        assert np.isinf(before["t"][0]) or cuts == [n]
        if not np.isinf(before["t"][0]):
            continue
        # system 0 is launched from t = inf: it records nothing and its checkpoint is passed on, slot count and window sums included
        assert last["n_recorded"][0] == last["first_row"][0] and last["n_events"][0] == one["n_events"][0] and last["n_exits"][0] == 0
        assert not np.any(last["pos"][0]) and not np.any(last["scalars"][0])
        for k in before:
            assert np.array_equal(before[k][0], last["checkpoint"][k][0]), k
        assert np.array_equal(last["checkpoint"]["n_slots"], [3, 2]) and last["checkpoint"]["next_obs"][0] == n
        from_inf += 1
    assert from_inf >= 1


# ---- 5. the large shape

LARGE = dict(walls=dict(base=dict(L=4200), systems=[(0.002, 90, 1.1), (0.05, 70, 2.0), (0.0, 40, 1.5)]),
             walls_anchors_exit=dict(base=dict(L=4200, anchor_positions=[0.3, 0.7], anchor_radius=0.02, k_on=2.0, k_off=0.5, k_exit=0.3),
                                     systems=[(0.002, 90, 1.1), (0.05, 70, 2.0), (0.0, 40, 1.5)]),
             wide=dict(base=dict(L=10050), systems=[(0.26, 40, 1.2), (0.002, 40, 0.8)]))   # one table in global memory, one in LDS


@pytest.mark.parametrize("name", list(LARGE))
def test_large_shape(gil, name):
    case = LARGE[name]
    T, times = 0.3, np.arange(15) * 0.02
    S = len(case["systems"])
    kw, states = mixed_keywords(gil, dict(dict(site_capacity=2, rate_diffusion=0.5, rate_active=4.0), **case["base"]), case["systems"],
                                [31 + 5 * s for s in range(S)], [0] * S, ref_obs=2, order=list(range(S))[::-1])
    one = gil.run_mixed_many_raw(states=states, times_obs=times, T=T, **kw)
    require_busy(one, 15)
    if name == "wide":
        plan = gil.plan_mixed_many(L=10050, K=2, periodic=False, sigma_grids=kw["sigma_grids"], n_systems=S, n_cap=40, n_obs=15)
        assert plan["n_global"] == 1 and plan["max_tlen_lds"] > 0
    seg, parts = in_segments(gil, kw, states, times, T, FIB_CUTS, large=True)
    assert len(parts) == 6
    assert_equal_runs(one, seg, name)
    assert np.array_equal(seg["checkpoint"]["n_slots"], [n for _, n, _ in case["systems"]])


# ---- 6. the structure sums

def structure_case(gil):
    """L = 64, N in {20, 33}, three ranges; anchors on the ten leftmost sites.  System 3 starts with its 20 particles bound there
    (they can only leave, at a total rate of k_exit per particle alive): it empties inside the window -- under its key and stream
    the 19th exit falls between the observations 37 and 38 and the last one between 47 and 48, so the window takes 8 observations
    with a particle and the last exit's event records 10 empty ones.  60 observations up to 4.5 give the slowest other system its
    120 events; T lies beyond them, so that a system whose events have become rare (particles piled up at the wall) still
    records the last observation instead of passing T first."""
    L, T, T_grid = 64, 6.0, 4.5
    mask = np.zeros(L, np.uint8)
    mask[:10] = 1
    base = dict(L=L, site_capacity=2, rate_diffusion=0.6, rate_active=4.0, k_on=1.0, k_off=0.0, k_exit=0.75)
    systems = [(0.0, 20, 0.9), (0.05, 33, 1.0), (0.2, 33, 1.1), (0.05, 20, 1.2), (0.2, 20, 1.3)]
    kw, states = mixed_keywords(gil, base, systems, [42] * 5, list(range(5)), anchor_mask=mask)
    states = [(30 + (np.arange(len(p)) % 34), s) for p, s in states]        # away from the anchors, at most one per site
    states[3] = (np.repeat(np.arange(10), 2), -np.ones(20, np.int8), np.ones(20, np.uint8))
    return kw, states, np.arange(60) * (T_grid / 60), T


@pytest.mark.parametrize("want_rows", [True, False], ids=["rows", "no_rows"])
def test_structure_sums(gil, want_rows):
    kw, states, times, T = structure_case(gil)
    more = dict(k_max=64, first_obs=30, want_rows=want_rows, want_states=False)
    one = gil.run_mixed_structure_raw(states=states, times_obs=times, T=T, **kw, **more)
    print("n_window", one["n_window"], "n_empty", one["n_empty"])
    require_busy(one, 60, systems=[0, 1, 2, 4])
    assert one["n_empty"][3] > 0 and one["n_window"][3] > 0, (one["n_window"], one["n_empty"])   # it empties inside the window
    assert 33 < one["n_window"][3] + 30 < 54 and one["n_recorded"][3] < 54                       # between the cuts at 33 and at 54
    assert (one["structure"] is None) == (not want_rows)
    keys = ("head", "window", "n_window", "n_empty") + (("structure",) if want_rows else ())
    for cuts in (FIB_CUTS, [30], list(range(1, 60))) if want_rows else (FIB_CUTS,):
        seg, parts = in_segments(gil, dict(kw), states, times, T, cuts, structure=True, **more)
        for k in COMMON[3:] + keys:
            assert np.array_equal(one[k], seg[k]), (cuts, k)
        assert all(a == b for a, b in zip(one["t_final"], seg["t_final"]))
        if cuts is FIB_CUTS:                                   # a cut before the window, and one inside it with the counts under way
            left_at = {r["obs_first"] + r["head"].shape[1]: r["checkpoint"] for r in parts}      # the checkpoint left at a cut
            assert not left_at[20]["n_window"].any() and not left_at[20]["n_empty"].any() and not left_at[20]["window"].any()
            assert np.all(left_at[33]["n_window"] + left_at[33]["n_empty"] == 33 - 30) and left_at[33]["window"][:, :, 0].any()


# ---- 7. the Python results

def build_systems(psys, sigmas=(0.02, 0.0, 0.05), L=200, N=(90, 60, 40), **over):
    kw = dict(L=L, xlim=1.0, rate_diffusion=0.4, rate_active=4.0, init="fixed", scale_rates=False, site_capacity=2, k_on=0.0, k_off=0.0, k_exit=0.0,
              seed=77, mode="gillespie_gpu")
    kw.update(over)
    return [psys.ParticleSystem(beta=0.5 + 0.5 * s, N=n, local_kernel_sigma=sg, rng=np.random.default_rng(40 + s), **kw)
            for s, (sg, n) in enumerate(zip(sigmas, N))]


@pytest.fixture(scope="module")
def psys(gil):
    return importlib.import_module(PKG + ".particle_system")


def assert_equal_outputs(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], list):
            assert len(a[k]) == len(b[k]) and all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a[k], b[k])), k
        else:
            assert (a[k] is None and b[k] is None) or np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def test_python_obs_per_launch_equals_the_single_launch(gil, psys):
    anchors = dict(k_on=3.0, k_off=1.0, k_exit=1.0, anchor_positions=[0.5], anchor_radius=0.1)
    kw = dict(T=2.0, obs_dt=0.1, record_fft=True, record_var=True)
    one_sys, seg_sys = build_systems(psys, **anchors), build_systems(psys, **anchors)
    one = gil.run_batched_exact_mixed(one_sys, **kw)
    seg, ck = gil.run_batched_exact_mixed(seg_sys, obs_per_launch=7, return_checkpoint=True, **kw)
    for a, b, pa, pb in zip(one, seg, one_sys, seg_sys):
        assert_equal_outputs(a, b)
        assert pa.n_events == pb.n_events > 100
    assert isinstance(ck, gil.MixedCheckpoint) and np.all(ck.next_obs == 20) and np.array_equal(ck.n_slots, [90, 60, 40]) and not ck.large
    one = gil.run_batched_exact_statistics_mixed(build_systems(psys), T=4.0, obs_dt=0.1)
    seg = gil.run_batched_exact_statistics_mixed(build_systems(psys), T=4.0, obs_dt=0.1, obs_per_launch=7)
    for a, b in zip(one, seg):
        assert_equal_outputs(a, b)
    skw = dict(T=3.0, obs_dt=0.05, k_max=30, reduce="device", return_series=True)
    one = gil.run_batched_exact_structure_mixed(build_systems(psys, L=100), **skw)
    seg = gil.run_batched_exact_structure_mixed(build_systems(psys, L=100), obs_per_launch=7, **skw)
    for a, b in zip(one, seg):
        assert_equal_outputs(a, b)


def test_python_sweeps_in_segments_equal_the_one_launch(gil):
    ens = importlib.import_module(PKG + ".ensemble")
    ps_kw = dict(L=100, xlim=1.0, rate_diffusion=0.4, rate_active=4.0, scale_rates=False, site_capacity=2, k_on=0.0, k_off=0.0, k_exit=0.0, seed=9)
    sweep = dict(ps_kwargs=ps_kw, init_kwargs=dict(init="fixed", N=50), run_kwargs=dict(T=3.0, obs_dt=0.1), rng_seeds=[[1, 2], [3, 4]])
    a = ens.sweep_over_sigmas([0.02, 0.0], [0.5, 2.0], 2, one_launch=True, on_device=True, dynamics="exact", **sweep)
    b = ens.sweep_over_sigmas([0.02, 0.0], [0.5, 2.0], 2, one_launch=True, on_device=True, dynamics="exact", obs_per_launch=10, **sweep)
    for sigma in a:
        for k in ("v_mean", "v_se", "D_mean", "D_se", "m_mean", "block_mean"):
            assert np.array_equal(a[sigma][k], b[sigma][k], equal_nan=True), (sigma, k)
    a = ens.sweep_sigmas_for_structures([0.02, 0.0], [0.5, 2.0], 2, one_launch=True, k_max=20, **sweep)
    b = ens.sweep_sigmas_for_structures([0.02, 0.0], [0.5, 2.0], 2, one_launch=True, k_max=20, obs_per_launch=10, **sweep)
    for sigma in a:
        for beta in a[sigma]:
            for k, v in a[sigma][beta].items():
                if k != "raw":
                    assert np.array_equal(np.asarray(v), np.asarray(b[sigma][beta][k]), equal_nan=True), (sigma, beta, k)


def test_python_save_load_resume_and_the_large_shape(gil, psys, tmp_path):
    _, ck = gil.run_batched_exact_mixed(build_systems(psys), T=2.0, obs_dt=0.1, obs_range=(0, 8), return_checkpoint=True)
    ck.save(tmp_path / "ck.npz")
    back = gil.MixedCheckpoint.load(tmp_path / "ck.npz")
    a, ca = gil.run_batched_exact_mixed(build_systems(psys), T=2.0, obs_dt=0.1, resume=ck, return_checkpoint=True)
    b, cb = gil.run_batched_exact_mixed(build_systems(psys), T=2.0, obs_dt=0.1, resume=back, return_checkpoint=True)
    for x, y in zip(a, b):
        assert_equal_outputs(x, y)
        assert len(x["times_obs"]) == 12 and x["pos_list"][-1] is not None
    for k in ca.arrays():
        assert np.array_equal(getattr(ca, k), getattr(cb, k)), k
    whole = gil.run_batched_exact_mixed(build_systems(psys), T=2.0, obs_dt=0.1)
    for s in range(3):
        assert all(np.array_equal(x, y) for x, y in zip(a[s]["pos_list"], whole[s]["pos_list"][8:]))
    # a large shape, two systems, three launches
    big = dict(sigmas=(0.002, 0.05), L=4200, N=(90, 70))
    one = gil.run_batched_exact_mixed(build_systems(psys, **big), T=0.3, obs_dt=0.02, allow_large=True, want_m_local=False)
    seg, ck = gil.run_batched_exact_mixed(build_systems(psys, **big), T=0.3, obs_dt=0.02, allow_large=True, want_m_local=False, obs_per_launch=5,
                                          return_checkpoint=True)
    assert ck.large and len(one[0]["times_obs"]) == 15
    for x, y in zip(one, seg):
        assert_equal_outputs(x, y)


# ---- 8. a switched beta, against the oracle

class TableRng:
    """tests/test_gpu_gillespie.py::TableRng: the oracle's generator fed from a table of uniforms, one row of four per event."""

    def __init__(self, table):
        self.table, self.row, self.col = table, -1, 0

    def exponential(self, scale):
        self.row += 1
        self.col = 2
        return scale * -np.log1p(-self.table[self.row, 0])

    def choice(self, n, p=None):
        cdf = np.cumsum(p)
        cdf /= cdf[-1]
        return int(np.searchsorted(cdf, self.table[self.row, 1], side="right"))

    def random(self):
        v = self.table[self.row, self.col]
        self.col += 1
        return v


def oracle_event_loop_switching_beta(orc, pos0, sigma0, table, T, times, n_events, switch_after, beta_new):
    """tests/test_gpu_gillespie_resume.py: the oracle's event loop with beta set to `beta_new` once observation `switch_after` is
    recorded."""
    orc.rng = TableRng(table)
    L, N = orc.par.L, len(pos0)
    pos, sigma, bound = pos0.copy(), sigma0.copy(), np.zeros(N, bool)
    cp, cm = np.bincount(pos[sigma == 1], minlength=L), np.bincount(pos[sigma == -1], minlength=L)
    snaps, exits, k, t, ev = [(pos.copy(), sigma.copy(), bound.copy())], ([], []), 1, 0.0, 0
    while t < T and k < len(times) and ev < n_events:
        field = orc.mean_field(cp, cm)
        pos, sigma, bound, tau = orc.fire_event(pos, sigma, bound, field, cp, cm, t, exits)
        ev += 1
        t += tau
        if t > T:
            break
        while k < len(times) and times[k] <= t:
            snaps.append((pos.copy(), sigma.copy(), bound.copy()))
            k += 1
        if k > switch_after:
            orc.par.beta = beta_new
    return snaps, exits, t, ev


def test_changed_beta_against_the_oracle(gil):
    """A mixed batch of two ranges; beta = 0.3 for the observations [0, 30), another per system after: the exact process with
    beta switched at the checkpoint's time, system by system against the oracle under the same uniforms."""
    base = dict(L=200, site_capacity=1, rate_diffusion=0.5, rate_active=4.0, xlim=1.0, scale_rates=False, k_on=0.0, k_off=0.0, k_exit=0.0)
    sigmas, N, new = (0.02, 0.05), 90, (2.5, 1.7)
    T, obs_dt, n_events = 3.0, 0.05, 12000
    times = np.arange(0.0, T, obs_dt)
    table = np.random.default_rng(zlib.crc32(b"changed_beta_mixed")).random((2, n_events, 4))
    orcs = [GillespieOracle(init="fixed", N=N, rng=np.random.default_rng(17 + s), local_kernel_sigma=sg, beta=0.3, **base) for s, sg in enumerate(sigmas)]
    states = [orc.init_particles() for orc in orcs]
    P = orcs[0].par
    raw = dict(L=base["L"], K=P.K, periodic=P.periodic, sigma_grids=[orc.par.sigma_grid for orc in orcs], variant_of_system=[0, 1],
               rate_diffusion=P.rate_diffusion, rate_active=P.rate_active, states=states, T=T, uniforms=table)
    head = gil.run_mixed_resumable_raw(betas=[0.3, 0.3], times_obs=times[:30], obs_first=0, **raw)
    tail = gil.run_mixed_resumable_raw(betas=list(new), times_obs=times[30:], obs_first=30, checkpoint=head["checkpoint"], **raw)
    r = gil._merge_segments([head, tail], 0)
    for s, orc in enumerate(orcs):
        snaps, exits, t, ev = oracle_event_loop_switching_beta(orc, *states[s], table[s], T, times, n_events, 29, new[s])
        assert int(r["n_events"][s]) == ev and int(r["n_recorded"][s]) == len(snaps) and ev > 400, (r["n_events"], ev)
        np.testing.assert_allclose(r["t_final"][s], t, rtol=1e-12)
        for kk, (p, sg, b) in enumerate(snaps):
            assert np.array_equal(r["pos"][s, kk, :N], p) and np.array_equal(r["sigma"][s, kk, :N], sg), (s, kk)
    same = gil.run_mixed_resumable_raw(betas=[0.3, 0.3], times_obs=times[30:], obs_first=30, checkpoint=head["checkpoint"], **raw)
    assert not np.array_equal(same["pos"], tail["pos"])        # the switch is not a no-op
