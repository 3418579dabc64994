"""GPU suite (-m gpu): ensemble density and field profiles in a MIXED launch of the exact event loop, both shapes
(include/gillespie_mixed_profile.h).

(1) The bin pass against NumPy on the states the SAME launch recorded, every system's field by an oracle of its own sigma:
    columns 0-5, members and the per-system rows exactly, the field column to 2e-9 per site of the bin and member (the allowance
    of tests/test_gpu_gillespie_profile.py, whose helpers are used).  Rows before first_obs, rows never reached and bins beyond
    n_bins_used are zero.  The cases are the smallest that reach what the combination could get wrong: systems shorter than
    n_cap (slots that a mixed launch never loads), the system's own field mode next to the launch's, groups that cross variants,
    a launch order that is not the identity (the system index, not the workgroup's), the profile slots behind the longest
    table's layout, 256 threads, the large shape with the table in LDS and, in one launch, a table read from global memory next
    to one kept in LDS and the global mean.
(2) Recording changes nothing else: every other output is gilx_run's / gilxm_run's, bit for bit, times included.
(3) The per-variant gilp_run launches the mixed launch replaces give its group rows exactly, in both shapes; a repeat and a
    permuted launch order too.
(4) A few hundred workgroups of three variants add into three groups.
(5) Systems that stop early, and first_obs > 0.
(6) The two sweep drivers with one_launch=True return what their host loops return.
(7) One mixed launch takes less kernel time than the six launches it replaces."""
import importlib

import numpy as np
import pytest

import test_gpu_gillespie_mixed_many as MM
import test_gpu_gillespie_profile as P

pytestmark = pytest.mark.gpu
PKG = P.PKG
TRAJECTORY_KEYS, PROFILE_KEYS = P.TRAJECTORY_KEYS, P.PROFILE_KEYS
BATCH, LARGE = 0, 1


@pytest.fixture(scope="module")
def gil():
    assert importlib.import_module(PKG + ".capi").device_count() >= 1
    return importlib.import_module(PKG + ".gillespie")


@pytest.fixture(scope="module")
def ens(gil):
    return importlib.import_module(PKG + ".ensemble")


WIDE = dict(L=10050, N=40, site_capacity=2, local_kernel_sigma=0.002, rate_diffusion=0.5, rate_active=4.0, beta=1.0)

# tag, parameters, sigmas of the variants, variant of every system, particle numbers, group ids, (T, obs_dt), bin counts,
# (shape, threads) of the plan, more keywords of the launch
SCENARIOS = [
    ("walls", P.WALLS, [0.05, 0.3, 0.0], [0, 1, 2, 0, 1, 2], [20, 20, 17, 12, 20, 9], [0, 1, 0, 1, 2, 2], (40.0, 2.0), (1, 7, 64), (BATCH, 64),
     dict(order=[3, 0, 5, 1, 4, 2], seeds=[11, 12, 13, 11, 12, 99], streams=[0, 0, 4, 1, 7, 2])),
    ("odd_ring", P.ODD_RING, [1.3, 0.004], [0, 1, 0], [300, 280, 300], [0, 0, 1], (4.0, 0.5), (7,), (BATCH, 64), {}),
    ("anchors", P.ANCHORS, [0.02, 0.1], [0, 1, 1, 0], [100, 100, 80, 90], [0, 1, 0, 1], (8.0, 0.5), (9, 160), (BATCH, 64), {}),
    ("four_waves", P.FOUR_WAVES, [0.004, 0.01], [0, 1], [1100, 1050], [0, 0], (0.8, 0.1), (1000,), (BATCH, 256), {}),
    ("large_table_in_lds", P.LARGE, [0.002, 0.005], [0, 1], [2000, 1900], [0, 1], (0.4, 0.1), (1000,), (LARGE, 1024), dict(order=[1, 0])),
    ("large_wide", WIDE, [0.26, 0.002, 0.0], [0, 1, 2], [40, 40, 40], [0, 1, 0], (3.0, 0.5), (1000,), (LARGE, 1024), {}),
]


def _mixed(case, sigmas, owner, ns, T, obs_dt, seed=5, d_beta=0.05):
    """The keywords of run_mixed_raw / run_mixed_profiles_raw for systems of `ns` particles, system s with sigmas[owner[s]]."""
    kw = P._batch(case, ns, T, obs_dt, seed=seed, d_beta=d_beta)
    del kw["sigma_grid"]
    dx = 1.0 / case["L"]
    return dict(kw, sigma_grids=[sg / dx for sg in sigmas], variant_of_system=list(owner))


def _fields(case, sigmas, owner):
    """Per system: (counts+, counts-) -> the field of its own variant, by the CPU oracle."""
    L, per_variant = case["L"], []
    for sg in sigmas:
        orc = P._oracle(dict(case, local_kernel_sigma=sg))
        if sg * L > 2000 and not case.get("periodic", False):      # the oracle's tap-by-tap loop would take minutes: its definition by FFT
            per_variant.append(lambda cp, cm, orc=orc: MM._field_by_fft(orc, cp, cm))
        else:
            per_variant.append(orc.mean_field)
    return [per_variant[v] for v in owner]


def _check(r, groups, n_groups, L, n_bins, fields, first_obs=0, tag=""):
    """_check_against_states of tests/test_gpu_gillespie_profile.py with a field per system (None: no field was asked for).
    Returns (bound particles seen, dead slots seen)."""
    S, M = r["pos"].shape[:2]
    width = -(-L // n_bins)
    used = -(-L // width)
    assert (r["bin_width"], r["n_bins_used"]) == (width, used)
    sites = np.zeros(n_bins)
    sites[:used] = width
    sites[used - 1] = L - (used - 1) * width
    want, members, field = np.zeros((n_groups, M, 7, n_bins), np.int64), np.zeros((n_groups, M), np.int32), np.zeros((n_groups, M, n_bins))
    seen_bound = seen_dead = 0
    for s in range(S):
        g = groups[s]
        for k in range(M):
            if k < first_obs or k >= r["n_recorded"][s]:
                assert not r["profile_obs"][s, k].any(), (tag, s, k)
                continue
            rows, cp, cm = P._host_counts(r, s, k, L, width, n_bins)
            assert np.array_equal(r["profile_obs"][s, k], rows), (tag, "profile_obs", s, k)
            want[g, k, :6] += np.stack([rows[0], rows[1], rows[2], rows[0] ** 2, rows[1] ** 2, rows[0] * rows[1]])
            members[g, k] += 1
            seen_bound += int(rows[2].sum())
            seen_dead += int(r["n0"][s] - rows[0].sum() - rows[1].sum())
            if fields is not None:
                m = fields[s](cp, cm) if cp.sum() + cm.sum() > 0 else np.zeros(L)
                field[g, k] += np.bincount(np.arange(L) // width, weights=m, minlength=n_bins)
    assert np.array_equal(r["members"], members), (tag, "members")
    assert np.array_equal(r["ensemble_sums"][:, :, :6], want[:, :, :6]), (tag, "columns 0 to 5")
    assert not r["ensemble_sums"][:, :, :, used:].any()
    if fields is None:
        assert not r["ensemble_sums"][:, :, 6].any()
    else:
        err = np.abs(r["ensemble_sums"][:, :, 6] / 2.0 ** 32 - field)
        allowed = 2e-9 * sites[None, None, :] * np.maximum(members, 1)[:, :, None]      # per member: 2e-9 per site of the bin
        worst = float((err / np.where(allowed > 0, allowed, 1.0)).max())
        print(f"{tag} n_bins {n_bins}: largest field error {err.max():.3e}, {worst:.3e} of its allowance; largest |field sum| {np.abs(field).max():.3f}")
        assert np.all(err <= allowed), (tag, "field column", worst)
    return seen_bound, seen_dead


@pytest.mark.parametrize("tag,case,sigmas,owner,ns,groups,run,bins,shape,more", SCENARIOS, ids=[c[0] for c in SCENARIOS])
def test_bin_pass_equals_numpy_on_the_states_of_the_same_launch(gil, tag, case, sigmas, owner, ns, groups, run, bins, shape, more):
    T, obs_dt = run
    kw = _mixed(case, sigmas, owner, ns, T, obs_dt)
    L, n_groups, M = case["L"], max(groups) + 1, len(kw["times_obs"])
    fields = _fields(case, sigmas, owner)
    for n_bins in bins:
        plan = gil.plan_mixed_profiles(L=L, K=kw["K"], periodic=kw["periodic"], sigma_grids=kw["sigma_grids"], variant_of_system=owner,
                                       n_systems=len(ns), n_cap=max(ns), n_obs=M, n_bins=n_bins, n_groups=n_groups, want_field=True, per_system=True)
        assert (plan["shape"], plan["threads"]) == shape
        r = gil.run_mixed_profiles_raw(n_bins=n_bins, want_field=True, group_of_system=groups, per_system=True, **kw, **more)
        print(f"{tag}: events per system {r['n_events'].tolist()}, recorded {r['n_recorded'].tolist()}, exits {r['n_exits'].tolist()}, "
              f"kernel {r['kernel_ms']:.2f} ms, plan {plan}")
        assert np.all(r["n_events"] >= 200) and np.all(r["n_events"] <= 40000)      # the inputs first: a test must not pass on nothing
        assert np.all(r["n_recorded"] == M) and r["n0"].tolist() == list(ns)
        assert r["ensemble_sums"].shape == (n_groups, M, 7, n_bins)
        bound, dead = _check(r, groups, n_groups, L, n_bins, fields, tag=tag)
        if "k_exit" in case:
            assert bound > 20 and dead > 5, (bound, dead)                           # bound counts and dead slots are in play
        assert (r["profile_obs"][:, -1] != r["profile_obs"][:, 0]).any()            # the profile moves with the dynamics
        for s, n in enumerate(ns):                                                  # the slots a system does not have stay empty
            assert not r["flags"][s, :, n:].any()
    if tag == "walls":                                                             # without the field its column stays zero
        r = gil.run_mixed_profiles_raw(n_bins=7, want_field=False, group_of_system=groups, per_system=True, **kw, **more)
        _check(r, groups, n_groups, L, 7, None, tag=tag)
        assert len(set(owner)) < len(owner) and 4 * kw["sigma_grids"][1] > L and kw["sigma_grids"][2] == 0.0
    if tag == "large_wide":
        assert plan["max_tlen"] + 1 > 10000 and gil.plan_mixed_many(L=L, K=kw["K"], periodic=False, sigma_grids=kw["sigma_grids"], n_systems=3,
                                                                      n_cap=40, n_obs=M)["n_global"] == 1


def test_recording_changes_nothing_else(gil):
    rng = np.random.default_rng(8)
    for case, sigmas, owner, ns, T, obs_dt, plain_run, n_bins, more in (
            (P.ANCHORS, [0.02, 0.1], [0, 1, 1], [100, 90, 80], 6.0, 0.5, gil.run_mixed_raw, 160, dict(seeds=[3, 4, 5], streams=[2, 0, 1])),
            (P.FOUR_WAVES, [0.004, 0.01], [1, 0], [1100, 1000], 0.5, 0.1, gil.run_mixed_raw, 33, {}),
            (P.LARGE, [0.002, 0.005], [0, 1], [2000, 1900], 0.3, 0.1, gil.run_mixed_many_raw, 1000, dict(order=[1, 0]))):
        kw = dict(_mixed(case, sigmas, owner, ns, T, obs_dt, seed=21), **more)
        for uniforms in (None, rng.random((len(ns), 6000, 4))):
            plain = plain_run(uniforms=uniforms, **kw)
            r = gil.run_mixed_profiles_raw(n_bins=n_bins, want_field=True, group_of_system=list(range(len(ns))), per_system=True,
                                           uniforms=uniforms, **kw)
            for key in TRAJECTORY_KEYS:
                assert np.array_equal(r[key], plain[key]), (case["L"], key, uniforms is None)
            assert np.all(r["n_events"] >= 500) and r["ensemble_sums"][:, :, :2].sum() == sum(
                int(((plain["flags"][s, k] & 2) != 0).sum()) for s in range(len(ns)) for k in range(int(plain["n_recorded"][s])))
            bare = gil.run_mixed_profiles_raw(n_bins=n_bins, want_field=True, group_of_system=list(range(len(ns))), uniforms=uniforms,
                                              want_states=False, **kw)            # the profile does not need the state outputs
            assert np.array_equal(bare["ensemble_sums"], r["ensemble_sums"]) and np.array_equal(bare["members"], r["members"])


REPLACED = [  # tag, parameters, sigmas, particle number of every variant, (T, obs_dt), n_bins, the unmixed shape's keys are the large ones
    ("batch", P.ANCHORS, [0.02, 0.1, 0.0], [100, 80, 100], (4.0, 0.5), 9, False),
    ("large", P.LARGE, [0.002, 0.005], [2000, 1900], (0.3, 0.1), 1000, True),
]


@pytest.mark.parametrize("tag,case,sigmas,n_of,run,n_bins,large", REPLACED, ids=[c[0] for c in REPLACED])
def test_mixed_launch_equals_the_profile_launches_it_replaces(gil, tag, case, sigmas, n_of, run, n_bins, large):
    """Three systems per variant, the first two in one ensemble group, the third in another; every variant is a group of
    mixed_keys with a key of its own: system j of it draws with (key, j), the large shape with (key + j, 0)."""
    T, obs_dt = run
    per, V = 3, len(sigmas)
    owner = [v for v in range(V) for _ in range(per)]
    ns = [n_of[v] for v in owner]
    keys = [1000 + 17 * v for v in range(V)]
    groups = [2 * v + (j == per - 1) for v in range(V) for j in range(per)]
    kw = _mixed(case, sigmas, owner, ns, T, obs_dt)
    seeds = [keys[v] + (j if large else 0) for v in range(V) for j in range(per)]
    streams = [0 if large else j for v in range(V) for j in range(per)]
    args = dict(n_bins=n_bins, want_field=True, group_of_system=groups, per_system=True)
    mixed = gil.run_mixed_profiles_raw(seeds=seeds, streams=streams, **args, **kw)
    assert np.all(mixed["n_events"] >= 300) and np.all(mixed["n_recorded"] == len(kw["times_obs"]))
    plan = gil.plan_mixed_profiles(L=case["L"], K=kw["K"], periodic=kw["periodic"], sigma_grids=kw["sigma_grids"], variant_of_system=owner,
                                   n_systems=len(ns), n_cap=max(ns), n_obs=len(kw["times_obs"]), n_bins=n_bins, n_groups=2 * V, want_field=True)
    assert plan["shape"] == (LARGE if large else BATCH)
    shared = {k: v for k, v in kw.items() if k not in ("sigma_grids", "variant_of_system", "betas", "states", "seed")}
    for v in range(V):
        mine = [s for s in range(len(ns)) if owner[s] == v]
        one = gil.run_profiles_raw(sigma_grid=kw["sigma_grids"][v], betas=[kw["betas"][s] for s in mine], states=[kw["states"][s] for s in mine],
                                   seed=keys[v], n_bins=n_bins, want_field=True, group_of_system=[0, 0, 1], per_system=True, **shared)
        assert np.array_equal(one["ensemble_sums"], mixed["ensemble_sums"][2 * v:2 * v + 2]), (tag, v, "ensemble_sums")
        assert np.array_equal(one["members"], mixed["members"][2 * v:2 * v + 2]), (tag, v, "members")
        assert np.array_equal(one["profile_obs"], mixed["profile_obs"][mine]) and one["ensemble_sums"][:, :, 6].any()
        for key in ("n_events", "t_final", "n_recorded"):
            assert np.array_equal(one[key], mixed[key][mine]), (tag, v, key)
        assert np.array_equal(one["pos"], mixed["pos"][mine][:, :, :n_of[v]])
    again = gil.run_mixed_profiles_raw(seeds=seeds, streams=streams, **args, **kw)
    other = gil.run_mixed_profiles_raw(seeds=seeds, streams=streams, order=list(np.random.default_rng(1).permutation(len(ns))), **args, **kw)
    for key in PROFILE_KEYS + TRAJECTORY_KEYS:
        assert np.array_equal(mixed[key], again[key]) and np.array_equal(mixed[key], other[key]), (tag, key)


def test_groups_and_contention(gil):
    """300 workgroups of three variants add into three rows of sums that cross the variants."""
    S = 300
    rng = np.random.default_rng(2)
    owner, groups = rng.integers(0, 3, S), rng.integers(0, 3, S).astype(np.int32)
    kw = _mixed(P.WALLS, [0.05, 0.3, 0.0], owner, [20] * S, 30.0, 2.5, seed=77, d_beta=0.004)
    r = gil.run_mixed_profiles_raw(n_bins=16, want_field=True, group_of_system=groups, per_system=True, want_states=False, **kw)
    M = len(kw["times_obs"])
    assert np.all(r["n_events"] >= 400) and np.all(r["n_recorded"] == M)
    assert r["members"].tolist() == [[int((groups == g).sum())] * M for g in range(3)] and min(r["members"][:, 0]) > 60
    rows = r["profile_obs"].astype(np.int64)
    cols = np.stack([rows[:, :, 0], rows[:, :, 1], rows[:, :, 2], rows[:, :, 0] ** 2, rows[:, :, 1] ** 2, rows[:, :, 0] * rows[:, :, 1]], axis=2)
    for g in range(3):
        assert np.array_equal(r["ensemble_sums"][g, :, :6], cols[groups == g].sum(axis=0)), g
    assert r["ensemble_sums"][:, :, 6].any() and np.all(r["ensemble_sums"][:, :, :2].sum(axis=(2, 3)) == 20 * r["members"])
    again = gil.run_mixed_profiles_raw(n_bins=16, want_field=True, group_of_system=groups, per_system=True, want_states=False, **kw)
    for key in PROFILE_KEYS + ("n_events", "t_final"):
        assert np.array_equal(r[key], again[key]), key


def test_systems_that_stop_early_and_first_obs(gil):
    """An empty system has no rate: its loop ends after observation 0.  A horizon T below the last observation time ends all."""
    sigmas, owner, groups = [0.05, 0.0], [0, 1, 1, 0, 0], [0, 0, 1, 1, 1]
    kw = _mixed(P.WALLS, sigmas, owner, [20, 5, 18, 20, 5], 24.0, 2.0)
    kw["states"][1] = kw["states"][4] = (np.zeros(0, np.int64), np.zeros(0, np.int8))
    fields = _fields(P.WALLS, sigmas, owner)
    r = gil.run_mixed_profiles_raw(n_bins=7, want_field=True, group_of_system=groups, per_system=True, **kw)
    assert r["n_recorded"].tolist() == [12, 1, 12, 12, 1] and r["n0"].tolist() == [20, 0, 18, 20, 0]
    assert r["members"].tolist() == [[2] + [1] * 11, [3] + [2] * 11]
    _check(r, groups, 2, 64, 7, fields, tag="empty member")
    times = np.arange(0.0, 24.0, 2.0)
    cut = gil.run_mixed_profiles_raw(n_bins=7, group_of_system=groups, per_system=True, **dict(kw, T=12.8))
    assert np.all(cut["n_recorded"][[0, 2, 3]] == np.sum(times <= 12.8)) and cut["n_recorded"].max() == 7
    assert cut["members"][0].tolist() == [2] + [1] * 6 + [0] * 5 and not cut["ensemble_sums"][:, 7:].any()
    _check(cut, groups, 2, 64, 7, None, tag="short horizon")
    assert np.array_equal(cut["ensemble_sums"][:, :7, :6], r["ensemble_sums"][:, :7, :6])     # the same trajectories up to there
    # first_obs > 0
    groups = [0, 1, 1, 0]
    kw = _mixed(P.ANCHORS, [0.02, 0.1], [0, 1, 0, 1], [100, 100, 80, 90], 3.0, 0.25)
    args = dict(n_bins=9, want_field=True, group_of_system=groups, per_system=True)
    full, late = gil.run_mixed_profiles_raw(first_obs=0, **args, **kw), gil.run_mixed_profiles_raw(first_obs=5, **args, **kw)
    assert np.all(full["n_recorded"] == 12) and full["members"].tolist() == [[2] * 12] * 2
    for key in PROFILE_KEYS:
        assert not late[key][:, :5].any(), key
        assert np.array_equal(late[key][:, 5:], full[key][:, 5:]) and full[key][:, :5].any(), key
    for key in TRAJECTORY_KEYS:
        assert np.array_equal(late[key], full[key]), key
    _check(late, groups, 2, 160, 9, _fields(P.ANCHORS, [0.02, 0.1], [0, 1, 0, 1]), first_obs=5, tag="first_obs")
    none = gil.run_mixed_profiles_raw(first_obs=12, **args, **kw)
    assert not any(none[key].any() for key in PROFILE_KEYS)


def _same(one, loop, outer, betas, members):
    assert list(one) == list(loop) == outer
    for o in outer:
        assert list(one[o]) == list(loop[o]) == betas
        for b in betas:
            a, h = one[o][b], loop[o][b]
            assert set(a) == set(h) and a["members"].tolist() == members
            for key in a:                                          # integer sums divided by the same counts: exact, NaN where NaN
                np.testing.assert_array_equal(np.asarray(a[key], dtype=float), np.asarray(h[key], dtype=float), err_msg=f"{o} {b} {key}")


def test_sweep_drivers_in_one_launch_equal_their_host_loops(ens):
    ps = dict(L=200, xlim=1.0, scale_rates=False, site_capacity=2, periodic=True, rate_diffusion=0.5, rate_active=3.0)
    betas, seeds = [0.0, 1.8], [[100 * b + r for r in range(2)] for b in range(2)]
    kw = dict(beta_values=betas, n_runs_per_beta=2, run_kwargs=dict(T=5.0, obs_dt=0.5), n_bins=20, rng_seeds=seeds)
    sigmas = [0.02, 0.0, 0.6]
    args = dict(sigma_values=sigmas, ps_kwargs=ps, init_kwargs=dict(init="fixed", N=100), want_field=True, **kw)
    one, loop = ens.profile_sweep_over_sigmas(one_launch=True, **args), ens.profile_sweep_over_sigmas(one_launch=False, **args)
    _same(one, loop, sigmas, betas, [2] * 10)
    assert np.all(np.abs(one[0.02][1.8]["field_mean"]) <= 1.0) and one[0.02][1.8]["field_mean"].any()
    assert not np.array_equal(one[0.02][1.8]["signed_mean"], one[0.6][1.8]["signed_mean"])
    assert np.all(one[0.0][0.0]["total_mean"].sum(axis=1) == 100.0)
    # seeded systems: every sigma has the key 4242 as in its own launch
    args = dict(args, ps_kwargs=dict(ps, seed=4242))
    _same(ens.profile_sweep_over_sigmas(one_launch=True, **args), ens.profile_sweep_over_sigmas(one_launch=False, **args), sigmas, betas, [2] * 10)
    numbers = [60, 100, 140]
    args = dict(n_part_values=numbers, ps_kwargs=dict(ps, local_kernel_sigma=0.02), init_kwargs=dict(init="fixed"), **kw)
    one, loop = ens.profile_sweep_over_densities(one_launch=True, **args), ens.profile_sweep_over_densities(one_launch=False, **args)
    _same(one, loop, numbers, betas, [2] * 10)
    assert [float(one[n][0.0]["total_mean"][3].sum()) for n in numbers] == [60.0, 100.0, 140.0]
    # the large shape
    big = dict(L=4200, xlim=1.0, scale_rates=False, site_capacity=2, rate_diffusion=0.3, rate_active=4.0)
    args = dict(sigma_values=[0.002, 0.005], beta_values=[0.8], n_runs_per_beta=2, ps_kwargs=big, init_kwargs=dict(init="fixed", N=2000),
                run_kwargs=dict(T=0.3, obs_dt=0.1), n_bins=100, rng_seeds=[[7, 8]], want_field=True)
    with pytest.raises(ValueError, match="is a large shape"):
        ens.profile_sweep_over_sigmas(one_launch=True, **args)
    one = ens.profile_sweep_over_sigmas(one_launch=True, allow_large=True, **args)
    _same(one, ens.profile_sweep_over_sigmas(one_launch=False, **args), [0.002, 0.005], [0.8], [2] * 3)
    assert one[0.002][0.8]["field_mean"].any()


def test_one_mixed_launch_takes_less_kernel_time_than_the_six_it_replaces(gil):
    """6 sigma x 8 systems of L = 1000, N = 500: each replaced launch occupies 8 of the device's compute units."""
    case = dict(L=1000, N=500, site_capacity=2, local_kernel_sigma=0.01, rate_diffusion=0.3, rate_active=4.0, beta=0.8)
    sigmas, per = [0.002, 0.004, 0.008, 0.016, 0.032, 0.0], 8
    owner = [v for v in range(6) for _ in range(per)]
    kw = _mixed(case, sigmas, owner, [500] * 48, 1.0, 0.1, d_beta=0.01)
    groups = list(owner)
    args = dict(n_bins=250, want_field=True, want_states=False)
    seeds, streams = [50 + v for v in owner], [j for _ in range(6) for j in range(per)]
    gil.run_mixed_profiles_raw(group_of_system=groups, seeds=seeds, streams=streams, **args, **kw)      # first launch: code objects load
    mixed = gil.run_mixed_profiles_raw(group_of_system=groups, seeds=seeds, streams=streams, **args, **kw)
    assert np.all(mixed["n_events"] >= 1000)
    shared = {k: v for k, v in kw.items() if k not in ("sigma_grids", "variant_of_system", "betas", "states", "seed")}
    total = 0.0
    for v in range(6):
        mine = slice(per * v, per * (v + 1))
        one = gil.run_profiles_raw(sigma_grid=kw["sigma_grids"][v], betas=kw["betas"][mine], states=kw["states"][mine], seed=50 + v, **args, **shared)
        assert np.array_equal(one["ensemble_sums"][0], mixed["ensemble_sums"][v]) and np.array_equal(one["n_events"], mixed["n_events"][mine])
        total += one["kernel_ms"]
    print(f"one mixed launch {mixed['kernel_ms']:.2f} ms, the six launches it replaces {total:.2f} ms: ratio {total / mixed['kernel_ms']:.2f}")
    assert mixed["kernel_ms"] < total
