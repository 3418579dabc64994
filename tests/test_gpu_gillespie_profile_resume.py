"""GPU suite (-m gpu): the ensemble profiles of the exact event loop taken in SEGMENTS (include/gillespie_profile_resume.h).  A
chain of launches of gilpr_run / gilxpr_run must be, BIT FOR BIT, the one launch of the entry point that knows no checkpoint
(gilp_run / gilxp_run: run_profiles_raw / run_mixed_profiles_raw), which is the reference in every test: positions, spins,
flags, the twelve scalar sums, n_recorded, event counts, the concatenated exit logs, ensemble_sums, members and profile_obs
(np.array_equal) and the final times (==).  There are no tolerances.

Preconditions are stated on the one-launch run: every observation recorded and at least two events per observation on average,
per system.  The pending-observation case states its own (at least 10 observations share their event with the one before), and
so do the early stops (a system that empties, max_events)."""
import importlib
import zlib

import numpy as np
import pytest

from oracle.gillespie_numpy import GillespieOracle

pytestmark = pytest.mark.gpu
PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"
FIB_CUTS = [1, 2, 4, 7, 12, 20, 33, 54]                        # the cuts of tests/test_gpu_gillespie_resume.py, on a 60-observation grid
COMMON = ("pos", "sigma", "flags", "scalars", "n_recorded", "n_events", "n_exits")
PROFILE = ("ensemble_sums", "members", "profile_obs")


@pytest.fixture(scope="module")
def gil():
    assert importlib.import_module(PKG + ".capi").device_count() >= 1
    return importlib.import_module(PKG + ".gillespie")


def raw_keywords(case, n_systems, seed, ref_obs, ns=None):
    """tests/test_gpu_gillespie_resume.py::raw_keywords: (keywords of the raw entry points without times / T, initial states);
    system s starts from the oracle's initial condition under rng seed 17 + s (`ns`: its particle number), every scalar sum is on."""
    case = dict(case)
    tag, N = case.pop("tag"), case.pop("N")
    kw = dict(xlim=1.0, scale_rates=False, k_on=0.0, k_off=0.0, k_exit=0.0)
    kw.update(case)
    states, P = [], None
    for s in range(n_systems):
        orc = GillespieOracle(init="fixed", N=N if ns is None else ns[s], rng=np.random.default_rng(17 + s), **kw)
        states.append(orc.init_particles())
        P = orc.par
    L = kw["L"]
    table = (np.random.default_rng(zlib.crc32(tag.encode())).random((P.K + 1, P.K + 1)) > 0.4).astype(np.uint8)
    return dict(L=L, K=P.K, periodic=P.periodic, sigma_grid=P.sigma_grid if P.sigma_kernel > 0 else 0.0, rate_diffusion=P.rate_diffusion,
                rate_active=P.rate_active, betas=[P.beta + 0.1 * s for s in range(n_systems)], minus_anchor=P.minus_anchor,
                immobilize=P.immobilize_when_anchored, suppress_flip=P.suppress_flip_when_bound, crowding=P.crowding_suppresses_rates,
                k_on=P.k_on, k_off=P.k_off, k_exit=P.k_exit, anchor_mask=P.is_anchor_site, seed=seed, x_wall=(3 * L) // 4,
                ref_obs=ref_obs, front_lo=np.maximum(np.arange(L) - 15, 0).astype(np.int32), block_table=table), states


def mixed_keywords(gil, base, systems, seeds, streams, ref_obs=-1, order=None):
    """tests/test_gpu_gillespie_mixed_resume.py::mixed_keywords: the systems (local_kernel_sigma, N, beta) on the oracle case `base`."""
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
    return dict(L=L, K=P.K, periodic=P.periodic, sigma_grids=sig, variant_of_system=owner, block_tables=tabs, rate_diffusion=P.rate_diffusion,
                rate_active=P.rate_active, betas=[b for _, _, b in systems], minus_anchor=P.minus_anchor, immobilize=P.immobilize_when_anchored,
                suppress_flip=P.suppress_flip_when_bound, crowding=P.crowding_suppresses_rates, k_on=P.k_on, k_off=P.k_off, k_exit=P.k_exit,
                anchor_mask=P.is_anchor_site, seeds=seeds, streams=streams, order=order, x_wall=(3 * L) // 4, ref_obs=ref_obs,
                front_lo=np.maximum(np.arange(L) - 15, 0).astype(np.int32)), inits


def in_segments(gil, kw, states, times, T, cuts, mixed=False, checkpoint=None, first=0, **more):
    """The observations first .. len(times) - 1 as a chain of profile launches cut before the observations `cuts`: (merged raw
    outputs, the raw outputs of every launch).  `first_obs` in `more` is absolute and handed to every launch as it is."""
    kw = dict(kw)
    ref_abs = kw.pop("ref_obs", -1)
    run = gil.run_mixed_profiles_resumable_raw if mixed else gil.run_profiles_resumable_raw
    edges = [first] + [c for c in cuts if first < c < len(times)] + [len(times)]
    parts = []
    for a, b in zip(edges[:-1], edges[1:]):
        r = run(states=states, times_obs=times[a:b], T=T, obs_first=a, checkpoint=checkpoint, ref_obs=ref_abs - a if a <= ref_abs < b else -1,
                **kw, **more)
        for k in PROFILE:                                      # a segment's arrays have the slice's rows
            assert r[k].shape[1] == b - a, (k, r[k].shape, a, b)
        checkpoint = r["checkpoint"]
        parts.append(r)
    return gil._merge_segments(parts, first), parts


def assert_equal_runs(one, seg, tag=""):
    """`seg` (merged segments) against `one` (one launch): equal in every output, the three profile arrays included."""
    for k in COMMON + PROFILE:
        assert one[k].shape == seg[k].shape and np.array_equal(one[k], seg[k]), (tag, k)
    for s in range(len(one["n_exits"])):
        n = int(one["n_exits"][s])
        assert np.array_equal(one["exits"][s, :n], seg["exits"][s, :n]), (tag, "exits", s)
    assert all(a == b for a, b in zip(one["t_final"], seg["t_final"])), (tag, one["t_final"], seg["t_final"])
    assert (one["bin_width"], one["n_bins_used"]) == (seg["bin_width"], seg["n_bins_used"])


def require_busy(one, M):
    """The preconditions on the one-launch run: every observation recorded, two events per observation on average."""
    print("n_recorded", one["n_recorded"], "n_events", one["n_events"], "of", M, "observations")
    assert np.all(one["n_recorded"] == M) and np.all(one["n_events"] >= 2 * M), (one["n_recorded"], one["n_events"])


# ---- 1. one wavefront, unmixed

ANCHORS = dict(tag="anchors_exit", L=160, N=100, site_capacity=2, local_kernel_sigma=0.02, rate_diffusion=0.6, rate_active=4.0, beta=0.9,
               anchor_positions=[0.3, 0.7], anchor_radius=0.08, k_on=3.0, k_off=1.0, k_exit=2.0)
GLOBAL_MEAN = dict(tag="global_mean_exit", L=150, N=90, site_capacity=2, local_kernel_sigma=0.0, periodic=True, rate_diffusion=0.5, rate_active=3.0,
                   beta=1.2, anchor_positions=[0.3, 0.7], anchor_radius=0.08, k_on=3.0, k_off=1.0, k_exit=2.0)


@pytest.mark.parametrize("case,n_bins", [(ANCHORS, 16), (ANCHORS, 160), (GLOBAL_MEAN, 16)], ids=["anchors_16", "anchors_L", "global_mean_exits"])
def test_one_wavefront(gil, case, n_bins):
    T, times = 3.0, np.arange(0.0, 3.0, 0.05)
    kw, states = raw_keywords(case, n_systems=6, seed=1234, ref_obs=5)
    prof = dict(n_bins=n_bins, want_field=True, per_system=True, group_of_system=[0, 1, 0, 1, 0, 1])
    one = gil.run_profiles_raw(states=states, times_obs=times, T=T, **kw, **prof)
    assert len(times) == 60
    require_busy(one, 60)
    assert np.any(one["ensemble_sums"][:, :, 6] != 0) and np.any(one["ensemble_sums"][:, :, 2] != 0)    # the field and bound particles
    seg, parts = in_segments(gil, kw, states, times, T, FIB_CUTS, **prof)
    assert len(parts) == len(FIB_CUTS) + 1
    assert_equal_runs(one, seg, case["tag"])
    # particles leave across cuts: the live totals a resumed start rebuilds (and, in the global-mean mode, the field column) change
    alive = one["scalars"][0, :, 0]
    assert sum(int(r["n_exits"][0]) > 0 for r in parts) >= 2 and alive[-1] < alive[0], alive
    if case is GLOBAL_MEAN:
        assert kw["sigma_grid"] == 0.0 and len(set(one["ensemble_sums"][0, :, 6, 0].tolist())) > 10


# ---- 2. four waves

def test_four_waves(gil):
    case = dict(tag="four_waves", L=700, N=1100, site_capacity=2, local_kernel_sigma=0.02, rate_diffusion=0.5, rate_active=4.0, beta=1.1)
    T, times = 1.2, np.arange(60) * 0.02
    kw, states = raw_keywords(case, n_systems=2, seed=1234, ref_obs=5, ns=[1100, 70])
    assert [len(p) for p, _ in states] == [1100, 70]           # n_cap beyond one wavefront's slots: the four-wave instantiation
    prof = dict(n_bins=700, want_field=True, per_system=True)
    assert gil.plan_profiles(L=700, K=2, periodic=False, sigma_grid=kw["sigma_grid"], n_systems=2, n_cap=1100, n_obs=60, n_bins=700,
                             want_field=True)["threads"] == 256
    one = gil.run_profiles_raw(states=states, times_obs=times, T=T, **kw, **prof)
    require_busy(one, 60)
    seg, parts = in_segments(gil, kw, states, times, T, FIB_CUTS, **prof)
    assert_equal_runs(one, seg, "four waves")


# ---- 3. large shape

LARGE = dict(tag="large", L=4200, N=2000, site_capacity=2, local_kernel_sigma=0.002, rate_diffusion=0.3, rate_active=4.0, beta=0.8,
             anchor_positions=[0.4], anchor_radius=0.01, k_on=10.0, k_off=1.0, k_exit=5.0)
TIGHT = dict(tag="tight", L=4096, N=2048, site_capacity=2, local_kernel_sigma=0.15, rate_diffusion=0.3, rate_active=4.0, beta=0.8)


@pytest.mark.parametrize("case,ns,n_bins", [(LARGE, [2000, 1900], 1000), (TIGHT, [2048], 1024)], ids=["large", "batch_sized_sent_to_large"])
def test_large_shape(gil, case, ns, n_bins):
    T, times = 0.24, np.arange(12) * 0.02
    kw, states = raw_keywords(case, n_systems=len(ns), seed=31, ref_obs=2, ns=ns)
    prof = dict(n_bins=n_bins, want_field=True, per_system=True)
    shape = dict(L=kw["L"], K=kw["K"], periodic=kw["periodic"], sigma_grid=kw["sigma_grid"], n_systems=len(ns), n_cap=max(ns))
    assert [gil.plan_profiles(n_obs=m, n_bins=n_bins, want_field=True, **shape)["shape"] for m in (1, 5, 12)] == [1, 1, 1]
    if case is TIGHT:                                          # the profile slots alone send it there: the keys are the large shape's
        assert gil.plan_profiles(n_obs=12, n_bins=1, **shape)["shape"] == 0
    one = gil.run_profiles_raw(states=states, times_obs=times, T=T, **kw, **prof)
    require_busy(one, 12)
    seg, parts = in_segments(gil, kw, states, times, T, [1, 5, 6], **prof)
    assert len(parts) == 4
    assert_equal_runs(one, seg, case["tag"])
    # the large shape's key convention (system s: seed + s): the trajectory is gilm_run's, not gil_run_batch's
    plain = gil.run_many_large_raw(states=states, times_obs=times, T=T, **kw)
    assert np.array_equal(plain["pos"], seg["pos"]) and np.array_equal(plain["n_events"], seg["n_events"])


# ---- 4. mixed

ANCHORED = dict(site_capacity=2, rate_diffusion=0.6, rate_active=4.0, anchor_positions=[0.3, 0.7], anchor_radius=0.08, k_on=3.0, k_off=1.0, k_exit=0.3)
SIX = [(0.0, 100, 0.9), (0.02, 100, 1.0), (0.2, 37, 1.1), (0.02, 37, 1.2), (0.0, 64, 1.3), (0.2, 5, 1.4)]   # (local_kernel_sigma, N, beta)
SIX_SEEDS, SIX_STREAMS = [1234, 1234, 77, 2 ** 63 + 5, 991, 992], [0, 1, 2, 2, 7, 3]
SIX_ORDER = [3, 0, 5, 1, 4, 2]
T_SIX = 15.0


@pytest.mark.parametrize("geometry", [dict(L=160), dict(L=150, periodic=True, site_capacity=1)], ids=["walls_K2", "ring_K1"])
def test_mixed_one_wavefront(gil, geometry):
    T, times = T_SIX, np.arange(60) * (T_SIX / 60)
    kw, states = mixed_keywords(gil, dict(ANCHORED, **geometry), SIX, SIX_SEEDS, SIX_STREAMS, ref_obs=5, order=SIX_ORDER)
    assert [len(p) for p, _ in states] == [100, 100, 37, 37, 64, 5] and len(kw["sigma_grids"]) >= 3
    prof = dict(n_bins=16, want_field=True, per_system=True, group_of_system=[0, 1, 2, 1, 0, 2])
    one = gil.run_mixed_profiles_raw(states=states, times_obs=times, T=T, **kw, **prof)
    require_busy(one, 60)
    seg, parts = in_segments(gil, kw, states, times, T, FIB_CUTS, mixed=True, **prof)
    assert len(parts) == len(FIB_CUTS) + 1
    assert_equal_runs(one, seg, geometry)
    assert np.array_equal(seg["checkpoint"]["n_slots"], [100, 100, 37, 37, 64, 5])
    for r in parts:                                            # the end state beyond a system's slots is empty
        for s, n in enumerate([100, 100, 37, 37, 64, 5]):
            assert not r["checkpoint"]["pos"][s, n:].any() and not r["checkpoint"]["flags"][s, n:].any() and np.all(r["checkpoint"]["ref"][s, n:] == -1)


def test_mixed_large(gil):
    base = dict(L=4200, site_capacity=2, rate_diffusion=0.3, rate_active=4.0, anchor_positions=[0.4], anchor_radius=0.01, k_on=10.0, k_off=1.0,
                k_exit=5.0)
    T, times = 0.24, np.arange(12) * 0.02
    kw, states = mixed_keywords(gil, base, [(0.002, 2000, 0.8), (0.004, 1900, 0.9)], [31, 32], [0, 0], ref_obs=2)
    prof = dict(n_bins=1000, want_field=True, per_system=True, group_of_system=[0, 1])
    one = gil.run_mixed_profiles_raw(states=states, times_obs=times, T=T, **kw, **prof)
    require_busy(one, 12)
    seg, parts = in_segments(gil, kw, states, times, T, [1, 5, 6], mixed=True, **prof)
    assert len(parts) == 4
    assert_equal_runs(one, seg, "mixed large")


# ---- 5. pending observations and the T break

SLOW = dict(tag="slow", L=60, N=8, site_capacity=1, local_kernel_sigma=0.05, rate_diffusion=1.0, rate_active=2.0, beta=1.0)


def test_pending_observations_and_the_T_break(gil):
    T, times = 2.0, np.arange(0.0, 2.0, 0.02)
    kw, states = raw_keywords(SLOW, n_systems=2, seed=99, ref_obs=3)
    prof = dict(n_bins=12, want_field=True, per_system=True)
    one = gil.run_profiles_raw(states=states, times_obs=times, T=T, **kw, **prof)
    n = int(one["n_recorded"][0])
    ev = one["scalars"][0, :n, 11]
    shared = np.flatnonzero(ev[1:] == ev[:-1]) + 1
    assert len(shared) >= 10, ev                               # observations that share their event with the one before
    seg, parts = in_segments(gil, kw, states, times, T, list(range(1, len(times))), **prof)
    assert len(parts) == len(times)                            # every row but row 0 is recorded at a segment's start or behind one event
    assert_equal_runs(one, seg, "cut before every observation")
    for k in shared:                                           # the same state: the same rows, in the chain as in the one launch
        assert np.array_equal(seg["profile_obs"][0, k], seg["profile_obs"][0, k - 1]) and np.array_equal(seg["profile_obs"][0, k], one["profile_obs"][0, k])
    # a checkpoint with t > T and one with t = +inf record nothing
    ck = {k: v.copy() for k, v in parts[49]["checkpoint"].items()}
    assert np.all(ck["next_obs"] == 50)
    ck["t"][:] = [T + 0.5, np.inf]
    r = gil.run_profiles_resumable_raw(states=None, times_obs=times[50:], T=T, obs_first=50, checkpoint=ck, **dict(kw, ref_obs=-1), **prof)
    assert not r["members"].any() and not r["ensemble_sums"].any() and not r["profile_obs"].any() and not r["scalars"].any()
    assert np.array_equal(r["n_recorded"], r["first_row"]) and np.array_equal(r["checkpoint"]["next_obs"], [50, 50])
    assert np.array_equal(r["n_events"], ck["n_events"]) and r["checkpoint"]["t"][0] == T + 0.5 and np.isinf(r["checkpoint"]["t"][1])


# ---- 6. early stops and first_obs

def test_a_system_that_empties_and_max_events(gil):
    case = dict(tag="emptying", L=40, N=3, site_capacity=2, local_kernel_sigma=0.05, rate_diffusion=1.0, rate_active=2.0, beta=1.0,
                anchor_positions=[0.5], anchor_radius=0.6, k_on=50.0, k_off=0.0, k_exit=20.0)
    T, times = 5.0, np.arange(0.0, 5.0, 0.1)
    kw, states = raw_keywords(case, n_systems=1, seed=5, ref_obs=-1)
    prof = dict(n_bins=8, want_field=True, per_system=True)
    one = gil.run_profiles_raw(states=states, times_obs=times, T=T, **kw, **prof)
    n = int(one["n_recorded"][0])
    assert np.isinf(one["t_final"][0]) and one["n_exits"][0] == 3 and 1 <= n < 25 and one["n_events"][0] < 40
    assert np.array_equal(one["members"][0], (np.arange(50) < n).astype(np.int32))
    for cuts in ([25], [n], [1, n + 1, 30]):
        seg, parts = in_segments(gil, kw, states, times, T, cuts, **prof)
        assert_equal_runs(one, seg, cuts)                      # members falls exactly where the one launch's falls
    # max_events reached inside a segment: the systems behind the next cut are skipped and add nothing to members
    T, times = 3.0, np.arange(0.0, 3.0, 0.05)
    kw, states = raw_keywords(ANCHORS, n_systems=3, seed=1234, ref_obs=5)
    prof = dict(n_bins=16, want_field=True, per_system=True, group_of_system=[0, 1, 0], max_events=400)
    one = gil.run_profiles_raw(states=states, times_obs=times, T=T, **kw, **prof)
    stop = one["n_recorded"]
    assert np.all(one["n_events"] == 400) and np.all(stop > 4) and np.all(stop < 54), (stop, one["n_events"])
    assert all(one["members"][:, k].sum() == int(np.sum(stop > k)) for k in range(60))
    seg, parts = in_segments(gil, kw, states, times, T, FIB_CUTS, **prof)
    assert_equal_runs(one, seg, "max_events")
    assert not parts[-1]["members"].any() and np.all(parts[-1]["n_recorded"] == 0)


@pytest.mark.parametrize("first_obs", [9, 12, 60, 75], ids=["inside_a_slice", "at_a_cut", "the_grids_end", "beyond_the_grid"])
def test_first_obs(gil, first_obs):
    T, times = 3.0, np.arange(0.0, 3.0, 0.05)
    kw, states = raw_keywords(ANCHORS, n_systems=3, seed=1234, ref_obs=5)
    prof = dict(n_bins=16, want_field=True, per_system=True, group_of_system=[0, 1, 0])
    one = gil.run_profiles_raw(states=states, times_obs=times, T=T, first_obs=min(first_obs, 60), **kw, **prof)
    require_busy(one, 60)
    seg, parts = in_segments(gil, kw, states, times, T, FIB_CUTS, first_obs=first_obs, **prof)
    assert_equal_runs(one, seg, first_obs)
    for k in PROFILE:                                          # rows before first_obs are zero in all three arrays
        assert not seg[k][:, :first_obs].any() and (first_obs >= 60 or seg[k][:, first_obs:].any()), k


# ---- 7. the Python functions

@pytest.fixture(scope="module")
def ens(gil):
    return importlib.import_module(PKG + ".ensemble")


def _systems(betas, sigmas=None, seed=4242, **more):
    psys = importlib.import_module(PKG + ".particle_system")
    kw = dict(L=200, xlim=1.0, scale_rates=False, site_capacity=2, periodic=True, rate_diffusion=0.5, rate_active=3.0, local_kernel_sigma=0.02,
              init="fixed", N=100, seed=seed)
    kw.update(more)
    return [psys.ParticleSystem(beta=b, rng=np.random.default_rng(300 + i), **(kw if sigmas is None else dict(kw, local_kernel_sigma=sigmas[i])))
            for i, b in enumerate(betas)]


def _same_results(a, b, rows=slice(None), tag=""):
    """two lists of DeviceProfiles results: exact integer sums divided by the same counts, NaN where NaN"""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert set(x) == set(y)
        for key in x:
            u, v = np.asarray(x[key], dtype=float), np.asarray(y[key], dtype=float)
            if key == "profile_obs":
                u, v = u[:, rows], v
            elif u.ndim >= 1 and u.shape[0] == len(x["times_obs"]) and key not in ("bin_sites",):
                u = u[rows]
            np.testing.assert_array_equal(u, v, err_msg=f"{tag} {key}")


def test_python_chain_equals_the_one_launch(gil):
    betas, groups = [0.4, 0.4, 1.6, 1.6], [0, 0, 1, 1]
    kw = dict(T=3.0, obs_dt=0.1, n_bins=20, groups=groups, want_field=True, per_system=True, first_obs=4)
    one = gil.run_batched_exact_profiles(_systems(betas), **kw)
    assert all(o["members"][4:].tolist() == [2] * 26 for o in one)
    _same_results(gil.run_batched_exact_profiles(_systems(betas), obs_per_launch=7, **kw), one, tag="obs_per_launch")
    # the mixed function, and a large shape with allow_large
    sig = [0.02, 0.0, 0.3, 0.02]
    one_x = gil.run_batched_exact_profiles_mixed(_systems(betas, sig), **kw)
    _same_results(gil.run_batched_exact_profiles_mixed(_systems(betas, sig), obs_per_launch=7, **kw), one_x, tag="mixed")
    big = dict(L=4200, N=2000, periodic=False, rate_diffusion=0.3, rate_active=4.0)
    kb = dict(T=0.3, obs_dt=0.05, n_bins=100, groups=[0, 1], want_field=True, allow_large=True)
    one_b = gil.run_batched_exact_profiles_mixed(_systems([0.8, 0.9], [0.002, 0.005], **big), **kb)
    got, ck = gil.run_batched_exact_profiles_mixed(_systems([0.8, 0.9], [0.002, 0.005], **big), obs_per_launch=4, return_checkpoint=True, **kb)
    _same_results(got, one_b, tag="mixed large")
    assert ck.large and np.all(ck.next_obs == 6)


def test_python_save_load_resume_and_two_betas(gil, tmp_path):
    betas, groups = [0.4, 0.4, 1.6, 1.6], [0, 0, 1, 1]
    kw = dict(T=3.0, obs_dt=0.1, n_bins=20, groups=groups, want_field=True, per_system=True)
    one = gil.run_batched_exact_profiles(_systems(betas), **kw)
    head, ck = gil.run_batched_exact_profiles(_systems(betas), obs_range=(0, 12), return_checkpoint=True, **kw)
    _same_results(one, head, rows=slice(0, 12), tag="head")
    ck.save(tmp_path / "ck.npz")
    back = gil.ProfileCheckpoint.load(tmp_path / "ck.npz")
    assert type(back) is gil.ProfileCheckpoint and back.n_bins == 20 and back.groups.tolist() == groups
    tail = gil.run_batched_exact_profiles(_systems(betas), resume=back, obs_range=(12, 30), **kw)
    _same_results(one, tail, rows=slice(12, 30), tag="tail with the original beta")    # equals the uninterrupted run
    # the other continuation: beta switched at the cut.  It differs after the cut and equals the raw chain with beta switched
    other = gil.run_batched_exact_profiles(_systems([2.5] * 4), resume=back, obs_range=(12, 30), **kw)
    assert not np.array_equal(other[0]["plus_mean"], tail[0]["plus_mean"])
    first = _systems(betas)[0]
    raw = dict(L=first.L, K=first.K, periodic=first.periodic, sigma_grid=first._sigma_grid, rate_diffusion=first.rate_diffusion,
               rate_active=first.rate_active, minus_anchor=first.minus_anchor, immobilize=first.immobilize_when_anchored,
               suppress_flip=first.suppress_flip_when_bound, crowding=first.crowding_suppresses_rates, k_on=first.k_on, k_off=first.k_off,
               k_exit=first.k_exit, anchor_mask=first.is_anchor_site, flip_table=first.flip_table(), T=3.0, seed=4242, want_states=False,
               n_bins=20, want_field=True, per_system=True, group_of_system=groups)
    times = np.arange(0.0, 3.0, 0.1)
    a = gil.run_profiles_resumable_raw(states=[q.init_particles() for q in _systems(betas)], times_obs=times[:12], betas=betas, **raw)
    b = gil.run_profiles_resumable_raw(states=None, times_obs=times[12:], betas=[2.5] * 4, obs_first=12, checkpoint=a["checkpoint"], **raw)
    for g in range(2):
        mine = np.flatnonzero(np.array(groups) == g)
        assert np.array_equal(other[g]["profile_obs"], b["profile_obs"][mine]) and b["members"][g].tolist() == [2] * 18
        assert np.array_equal(other[g]["plus_mean"] * 2, b["ensemble_sums"][g][:, 0].astype(float))


# ---- 8. the sweep drivers

def _same_sweeps(one, two):
    assert list(one) == list(two)
    for o in one:
        assert list(one[o]) == list(two[o])
        _same_results([one[o][b] for b in one[o]], [two[o][b] for b in two[o]], tag=str(o))


def test_sweep_drivers_in_segments_equal_their_one_launch(ens, gil):
    ps = dict(L=200, xlim=1.0, scale_rates=False, site_capacity=2, periodic=True, rate_diffusion=0.5, rate_active=3.0)
    betas, seeds = [0.0, 1.8], [[100 * b + r for r in range(2)] for b in range(2)]
    kw = dict(beta_values=betas, n_runs_per_beta=2, run_kwargs=dict(T=5.0, obs_dt=0.5), n_bins=20, rng_seeds=seeds, want_field=True)
    args = dict(ps_kwargs=dict(ps, local_kernel_sigma=0.02), init_kwargs=dict(init="fixed", N=100), **kw)
    one = ens.profile_sweep(**args)
    seg, ck = ens.profile_sweep(obs_per_launch=3, return_checkpoint=True, **args)
    assert isinstance(ck, gil.ProfileCheckpoint)
    _same_results([one[b] for b in betas], [seg[b] for b in betas], tag="profile_sweep")
    args = dict(sigma_values=[0.02, 0.0, 0.6], ps_kwargs=ps, init_kwargs=dict(init="fixed", N=100), **kw)
    _same_sweeps(ens.profile_sweep_over_sigmas(one_launch=True, **args), ens.profile_sweep_over_sigmas(one_launch=True, obs_per_launch=3, **args))
    args = dict(n_part_values=[60, 100, 140], ps_kwargs=dict(ps, local_kernel_sigma=0.02), init_kwargs=dict(init="fixed"), **kw)
    _same_sweeps(ens.profile_sweep_over_densities(one_launch=True, **args), ens.profile_sweep_over_densities(one_launch=True, obs_per_launch=4, **args))
    with pytest.raises(ValueError, match="obs_per_launch needs one_launch=True"):
        ens.profile_sweep_over_densities(one_launch=False, obs_per_launch=4, **args)
    big = dict(L=4200, xlim=1.0, scale_rates=False, site_capacity=2, rate_diffusion=0.3, rate_active=4.0)
    args = dict(sigma_values=[0.002, 0.005], beta_values=[0.8], n_runs_per_beta=2, ps_kwargs=big, init_kwargs=dict(init="fixed", N=2000),
                run_kwargs=dict(T=0.3, obs_dt=0.05), n_bins=100, rng_seeds=[[7, 8]], want_field=True, one_launch=True, allow_large=True)
    got, ck = ens.profile_sweep_over_sigmas(obs_per_launch=4, return_checkpoint=True, **args)
    _same_sweeps(ens.profile_sweep_over_sigmas(**args), got)
    assert isinstance(ck, gil.MixedProfileCheckpoint) and ck.large
