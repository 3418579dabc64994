"""GPU suite (-m gpu): the exact event loop run in segments (include/gillespie_resume.h).  A run resumed from a checkpoint must
be the uninterrupted run BIT FOR BIT, wherever it is cut: positions, spins, flags, all twelve scalar sums (event count and
displacement sums included), event counts, the concatenated exit log (np.array_equal) and the final time (==).  The
uninterrupted run is the launch of the entry points that know no checkpoint (gil_run_batch, gilm_run); the segments go
through gilr_run / gilrm_run, the first of them from a fresh start."""
import importlib
import zlib

import numpy as np
import pytest

from oracle.gillespie_numpy import GillespieOracle

pytestmark = pytest.mark.gpu
PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"
FIB_CUTS = [1, 2, 4, 7, 12, 20, 33, 54]                        # segments of 1, 1, 2, 3, 5, 8, 13, 21, ... observations


@pytest.fixture(scope="module")
def gil():
    assert importlib.import_module(PKG + ".capi").device_count() >= 1
    return importlib.import_module(PKG + ".gillespie")


def raw_keywords(case, n_systems, seed, ref_obs):
    """(keywords of the raw entry points without times / T, initial states) of a case in the manner of test_gpu_gillespie.CASES;
    system s starts from the oracle's initial condition under rng seed 17 + s, every scalar sum is switched on."""
    case = dict(case)
    tag, N = case.pop("tag"), case.pop("N")
    kw = dict(xlim=1.0, scale_rates=False, k_on=0.0, k_off=0.0, k_exit=0.0)
    kw.update(case)
    states, P = [], None
    for s in range(n_systems):
        orc = GillespieOracle(init="fixed", N=N, rng=np.random.default_rng(17 + s), **kw)
        states.append(orc.init_particles())
        P = orc.par
    L = kw["L"]
    table = (np.random.default_rng(zlib.crc32(tag.encode())).random((P.K + 1, P.K + 1)) > 0.4).astype(np.uint8)
    return dict(L=L, K=P.K, periodic=P.periodic, sigma_grid=P.sigma_grid if P.sigma_kernel > 0 else 0.0, rate_diffusion=P.rate_diffusion,
                rate_active=P.rate_active, betas=[P.beta + 0.1 * s for s in range(n_systems)], minus_anchor=P.minus_anchor,
                immobilize=P.immobilize_when_anchored, suppress_flip=P.suppress_flip_when_bound, crowding=P.crowding_suppresses_rates,
                k_on=P.k_on, k_off=P.k_off, k_exit=P.k_exit, anchor_mask=P.is_anchor_site, seed=seed, x_wall=(3 * L) // 4,
                ref_obs=ref_obs, front_lo=np.maximum(np.arange(L) - 15, 0).astype(np.int32), block_table=table), states


def in_segments(gil, kw, states, times, T, cuts, large=False, checkpoint=None, first=0, **more):
    """The observations first .. len(times) - 1 as a chain of launches cut before the observations `cuts`: (merged raw outputs,
    the raw outputs of every launch)."""
    kw = dict(kw)
    ref_abs = kw.pop("ref_obs", -1)
    edges = [first] + [c for c in cuts if first < c < len(times)] + [len(times)]
    parts = []
    for a, b in zip(edges[:-1], edges[1:]):
        r = gil.run_resumable_raw(states=states, times_obs=times[a:b], T=T, obs_first=a, checkpoint=checkpoint, large=large,
                                  ref_obs=ref_abs - a if a <= ref_abs < b else -1, **kw, **more)
        checkpoint = r["checkpoint"]
        parts.append(r)
    return gil._merge_segments(parts, first), parts


def assert_equal_runs(one, seg, tag=""):
    """`seg` (merged segments) against `one` (one launch): equal in every output."""
    for k in ("pos", "sigma", "flags", "scalars", "n_recorded", "n_events", "n_exits"):
        assert np.array_equal(one[k], seg[k]), (tag, k)
    for s in range(len(one["n_exits"])):
        n = int(one["n_exits"][s])
        assert np.array_equal(one["exits"][s, :n], seg["exits"][s, :n]), (tag, "exits", s)
    assert all(a == b for a, b in zip(one["t_final"], seg["t_final"])), (tag, one["t_final"], seg["t_final"])


CASES = [
    dict(tag="reflect_k1", L=200, N=90, site_capacity=1, local_kernel_sigma=0.02, rate_diffusion=0.5, rate_active=4.0, beta=1.1),
    dict(tag="periodic_k2", L=150, N=160, site_capacity=2, local_kernel_sigma=0.03, periodic=True, rate_diffusion=0.8, rate_active=3.0, beta=0.6),
    dict(tag="global_field", L=100, N=60, site_capacity=1, local_kernel_sigma=0.0, rate_diffusion=1.0, rate_active=2.0, beta=1.5),
    dict(tag="anchors_exit", L=160, N=100, site_capacity=2, local_kernel_sigma=0.02, rate_diffusion=0.6, rate_active=4.0, beta=0.9,
         anchor_positions=[0.3, 0.7], anchor_radius=0.08, k_on=3.0, k_off=1.0, k_exit=2.0),
    dict(tag="four_waves", L=700, N=1100, site_capacity=2, local_kernel_sigma=0.02, rate_diffusion=0.5, rate_active=4.0, beta=1.1, T=0.3,
         obs_dt=0.005),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["tag"])
def test_cut_invariance_lds_kernel(gil, case):
    case = dict(case)
    T, obs_dt = case.pop("T", 3.0), case.pop("obs_dt", 0.05)
    times = np.arange(0.0, T, obs_dt)
    kw, states = raw_keywords(case, n_systems=2, seed=1234, ref_obs=5)
    one = gil.run_raw(states=states, times_obs=times, T=T, **kw)
    # precondition on the uninterrupted run: every observation reached, and at least two events per observation on average, so
    # that the cuts fall between events of a busy run and not into an idle stretch
    assert len(times) == 60 and np.all(one["n_recorded"] == 60) and np.all(one["n_events"] >= 2 * len(times))
    assert np.any(one["scalars"][:, 6:, 9] > 0)                # the displacement sums are on (origin: observation 5)
    seg, parts = in_segments(gil, kw, states, times, T, FIB_CUTS)
    assert len(parts) == len(FIB_CUTS) + 1
    assert_equal_runs(one, seg, case["tag"])
    if case["tag"] == "anchors_exit":                          # dead slots, bound flags and the exit log cross a cut
        alive = one["scalars"][0, :, 0]
        assert any(alive[c - 1] < len(states[0][0]) and alive[-1] < alive[c - 1] for c in FIB_CUTS), alive
        assert sum(int(r["n_exits"][0]) > 0 for r in parts) >= 2 and np.any((one["flags"][0] & 1) != 0)
    if case["tag"] == "four_waves":
        assert len(states[0][0]) > 1024                        # beyond one wavefront's slots: the four-wave instantiation


SLOW = dict(tag="slow", L=60, N=8, site_capacity=1, local_kernel_sigma=0.05, rate_diffusion=1.0, rate_active=2.0, beta=1.0)


def test_pending_observations_and_the_T_break(gil):
    T, times = 2.0, np.arange(0.0, 2.0, 0.02)
    kw, states = raw_keywords(SLOW, n_systems=2, seed=99, ref_obs=3)
    one = gil.run_raw(states=states, times_obs=times, T=T, **kw)
    ev = one["scalars"][0, :int(one["n_recorded"][0]), 11]
    assert int(np.sum(ev[1:] == ev[:-1])) >= 10, ev            # observations that share their event with the one before
    seg, parts = in_segments(gil, kw, states, times, T, list(range(1, len(times))))
    assert len(parts) == len(times)
    assert_equal_runs(one, seg, "cut after every observation")
    # a run to T = 0.6, continued to T = 2.0 (each system from its own next observation), is the run to T = 2.0
    short_times = np.arange(0.0, 0.6, 0.02)
    assert np.array_equal(short_times, times[:len(short_times)])
    head = gil.run_resumable_raw(states=states, times_obs=short_times, T=0.6, **kw)
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


def test_a_system_that_empties(gil):
    case = dict(tag="emptying", L=40, N=3, site_capacity=2, local_kernel_sigma=0.05, rate_diffusion=1.0, rate_active=2.0, beta=1.0,
                anchor_positions=[0.5], anchor_radius=0.6, k_on=50.0, k_off=0.0, k_exit=20.0)
    T, times = 5.0, np.arange(0.0, 5.0, 0.1)
    kw, states = raw_keywords(case, n_systems=1, seed=5, ref_obs=-1)
    one = gil.run_raw(states=states, times_obs=times, T=T, **kw)
    n = int(one["n_recorded"][0])
    assert np.isinf(one["t_final"][0]) and one["n_exits"][0] == 3 and 1 <= n < 25 and one["n_events"][0] < 40
    for cuts in ([25], [n], [1, n + 1, 30]):
        seg, parts = in_segments(gil, kw, states, times, T, cuts)
        assert_equal_runs(one, seg, cuts)
        assert np.isinf(parts[-2]["checkpoint"]["t"][0]) or cuts == [n]
        if not np.isinf(parts[-2]["checkpoint"]["t"][0]):
            continue
        last = parts[-1]                                       # launched from t = inf: it records nothing and changes nothing
        assert last["n_recorded"][0] == last["first_row"][0] and last["n_events"][0] == one["n_events"][0] and last["n_exits"][0] == 0
        assert not np.any(last["pos"]) and not np.any(last["scalars"]) and np.isinf(last["checkpoint"]["t"][0])
        assert last["checkpoint"]["next_obs"][0] == n


BIG_CASES = [
    dict(tag="big_reflect_k1", L=3000, N=1500, site_capacity=1, local_kernel_sigma=0.01, rate_diffusion=0.5, rate_active=4.0, beta=1.1),
    dict(tag="big_anchors_exit", L=2400, N=1700, site_capacity=2, local_kernel_sigma=0.01, rate_diffusion=0.6, rate_active=4.0, beta=0.9,
         anchor_positions=[0.3, 0.7], anchor_radius=0.05, k_on=3.0, k_off=1.0, k_exit=2.0),
]


@pytest.mark.parametrize("case", BIG_CASES, ids=lambda c: c["tag"])
def test_cut_invariance_large_kernel(gil, case):
    T, times = 0.3, np.arange(0.0, 0.3, 0.02)
    kw, states = raw_keywords(case, n_systems=2, seed=31, ref_obs=2)
    kw["n_cap"] = 2100                                         # beyond GIL_MAX_N: spare slots that stay empty
    one = gil.run_many_large_raw(states=states, times_obs=times, T=T, **kw)
    assert np.all(one["n_recorded"] == len(times)) and np.all(one["n_events"] >= 2 * len(times))
    seg, parts = in_segments(gil, kw, states, times, T, FIB_CUTS, large=True)
    assert len(parts) == 6
    assert_equal_runs(one, seg, case["tag"])
    if case["tag"] == "big_anchors_exit":
        assert sum(int(r["n_exits"][0]) > 0 for r in parts) >= 2


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
    """tests/test_gpu_gillespie.py::oracle_event_loop with beta set to `beta_new` once observation `switch_after` is recorded."""
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
    """beta = 0.3 for the observations [0, 30), 2.5 after: the exact process with beta switched at the checkpoint's time."""
    case = dict(CASES[0], beta=0.3)
    tag, N = case.pop("tag"), case.pop("N")
    kw = dict(xlim=1.0, scale_rates=False, k_on=0.0, k_off=0.0, k_exit=0.0)
    kw.update(case)
    T, obs_dt, n_events = 3.0, 0.05, 12000
    table = np.random.default_rng(zlib.crc32(b"changed_beta")).random((n_events, 4))
    orc = GillespieOracle(init="fixed", N=N, rng=np.random.default_rng(17), **kw)
    pos0, sigma0 = orc.init_particles()
    times = np.arange(0.0, T, obs_dt)
    P = orc.par
    raw = dict(L=kw["L"], K=P.K, periodic=P.periodic, sigma_grid=P.sigma_grid, rate_diffusion=P.rate_diffusion, rate_active=P.rate_active,
               states=[(pos0, sigma0)], T=T, uniforms=table[None])
    snaps, exits, t, ev = oracle_event_loop_switching_beta(orc, pos0, sigma0, table, T, times, n_events, 29, 2.5)
    head = gil.run_resumable_raw(betas=[0.3], times_obs=times[:30], obs_first=0, **raw)
    tail = gil.run_resumable_raw(betas=[2.5], times_obs=times[30:], obs_first=30, checkpoint=head["checkpoint"], **raw)
    r = gil._merge_segments([head, tail], 0)
    assert int(r["n_events"][0]) == ev and int(r["n_recorded"][0]) == len(snaps) and ev > 400, (r["n_events"], ev)
    np.testing.assert_allclose(r["t_final"][0], t, rtol=1e-12)
    for kk, (p, s, b) in enumerate(snaps):
        assert np.array_equal(r["pos"][0, kk, :N], p) and np.array_equal(r["sigma"][0, kk, :N], s), kk
    same = gil.run_resumable_raw(betas=[0.3], times_obs=times[30:], obs_first=30, checkpoint=head["checkpoint"], **raw)
    assert not np.array_equal(same["pos"], tail["pos"])        # the switch is not a no-op


def build_systems(n, **over):
    from PARTICLE_solver_CLASS import ParticleSystem
    kw = dict(L=300, xlim=1.0, rate_diffusion=0.4, rate_active=4.0, init="fixed", N=140, scale_rates=False, local_kernel_sigma=0.02,
              site_capacity=2, k_on=0.0, k_off=0.0, k_exit=0.0, seed=77, mode="gillespie_gpu")
    kw.update(over)
    return [ParticleSystem(beta=0.5 + 0.5 * s, rng=np.random.default_rng(40 + s), **kw) for s in range(n)]


def assert_equal_outputs(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], list):
            assert len(a[k]) == len(b[k]) and all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a[k], b[k])), k
        else:
            assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k], equal_nan=True), k


def test_obs_per_launch_equals_the_single_launch(gil):
    kw = dict(T=2.0, obs_dt=0.1, record_fft=True, record_var=True)
    one_sys = build_systems(3, k_on=3.0, k_off=1.0, k_exit=1.0, anchor_positions=[0.5], anchor_radius=0.1)
    seg_sys = build_systems(3, k_on=3.0, k_off=1.0, k_exit=1.0, anchor_positions=[0.5], anchor_radius=0.1)
    one = gil.run_batched_exact(one_sys, **kw)
    seg, ck = gil.run_batched_exact(seg_sys, obs_per_launch=3, return_checkpoint=True, **kw)
    for a, b, pa, pb in zip(one, seg, one_sys, seg_sys):
        assert_equal_outputs(a, b)
        assert pa.n_events == pb.n_events > 500
    assert any(len(o["exit_times"]) > 0 for o in one)
    assert np.all(ck.next_obs == 20) and ck.streams == "batch" and ck.seed == 77


def test_obs_per_launch_statistics_equal_the_single_launch(gil):
    ens = importlib.import_module(PKG + ".ensemble")
    one = gil.run_batched_exact_statistics(build_systems(3), T=4.0, obs_dt=0.1)
    seg = gil.run_batched_exact_statistics(build_systems(3), T=4.0, obs_dt=0.1, obs_per_launch=7)
    assert len(one) == len(seg) == 3
    for a, b in zip(one, seg):
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k
    ps_kw = dict(L=300, xlim=1.0, rate_diffusion=0.4, rate_active=4.0, scale_rates=False, local_kernel_sigma=0.02, site_capacity=2,
                 k_on=0.0, k_off=0.0, k_exit=0.0, seed=9)
    sweep = dict(ps_kwargs=ps_kw, init_kwargs=dict(init="fixed", N=140), run_kwargs=dict(T=4.0, obs_dt=0.1), rng_seeds=[[1, 2], [3, 4]],
                 dynamics="exact", on_device=True)
    a, b = ens.sweep_over_betas([0.5, 2.0], 2, **sweep), ens.sweep_over_betas([0.5, 2.0], 2, obs_per_launch=9, **sweep)
    for k in ("means", "D_means", "m_means", "rho_means", "block_means"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_continue_run_equals_one_longer_run():
    (long_ps,), (ps,) = build_systems(1), build_systems(1)
    whole = long_ps.run(T=2.0, obs_dt=0.05)
    first = ps.run(T=0.8, obs_dt=0.05)
    assert ps.checkpoint is not None and ps.checkpoint.next_obs[0] == len(first["times_obs"])
    rest = ps.continue_run(T=2.0)
    k = len(first["times_obs"])
    assert len(rest["times_obs"]) == len(whole["times_obs"]) - k and np.array_equal(rest["times_obs"], whole["times_obs"][k:])
    for key in ("pos_list", "bound_list", "particle_count_list"):
        assert all(np.array_equal(x, y) for x, y in zip(first[key] + rest[key], whole[key])), key
    for key in ("rho_p_list", "rho_m_list", "m_local_list", "m_global"):
        assert np.array_equal(np.concatenate([first[key], rest[key]]), whole[key]), key
    assert ps.n_events == long_ps.n_events and ps.checkpoint.t[0] == long_ps.checkpoint.t[0]


def test_save_load_resume_equals_resuming_from_memory(gil, tmp_path):
    systems = build_systems(2)
    _, ck = gil.run_batched_exact(systems, T=2.0, obs_dt=0.1, obs_range=(0, 8), return_checkpoint=True)
    ck.save(tmp_path / "ck.npz")
    back = gil.Checkpoint.load(tmp_path / "ck.npz")
    a, ca = gil.run_batched_exact(build_systems(2), T=2.0, obs_dt=0.1, resume=ck, return_checkpoint=True)
    b, cb = gil.run_batched_exact(build_systems(2), T=2.0, obs_dt=0.1, resume=back, return_checkpoint=True)
    for x, y in zip(a, b):
        assert_equal_outputs(x, y)
        assert len(x["times_obs"]) == 12 and x["pos_list"][-1] is not None
    for k, _, _ in gil.CHECKPOINT_ARRAYS:
        assert np.array_equal(getattr(ca, k), getattr(cb, k)), k
    whole = gil.run_batched_exact(build_systems(2), T=2.0, obs_dt=0.1)
    assert all(np.array_equal(x, y) for x, y in zip(a[0]["pos_list"], whole[0]["pos_list"][8:]))
