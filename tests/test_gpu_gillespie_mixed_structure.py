"""GPU suite (-m gpu): mixed batches of the exact event loop WITH the structure sums and their window reduction on the device
(include/gillespie_mixed_structure.h).

1.  Rows of a mixed launch against NumPy on the states the same launch recorded, system by system, each with its own field
    (bars of tests/test_gpu_gillespie_structure.py: n and sum occ^2 exact, sum m and sum m^2 to rtol 1e-9, Fourier sums to
    1e-9 * max(n, 1) absolute).
2.  Window sums against NumPy on the rows of the same launch: a0 to 4 ulp of hypot(re, im) / n; sum d and sum d^2 within
    (M_w + 8) * 2^-52 of sum |d| and sum d^2 -- the bound of a sequential sum of M_w terms, each term formed as the header
    says (sqrt(re * re + im * im) / n, minus a0); n_window; head rows bit-equal to row entries 0..3.
3.  Without rows and states: the same window, head, scalars, events and times, bit for bit.
4.  A mixed launch with Philox against the per-variant run_structure_raw launches it replaces.
5.  The launch order changes nothing.
6.  n_cap > 1024: 256 threads for the whole launch.  More systems than modes.
7.  first_obs and observations the loop never reached.
8.  Particles leave during the window.
9.  run_batched_exact_structure_mixed: the device reduction against the rows reduced on the host, and against
    run_batched_exact_structure on a uniform batch.
10. sweep_sigmas_for_structures in one launch against the host loop over sigma.
11. The mixed launch takes less kernel time than the launches it replaces, and without rows fewer bytes come back."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"

T, OBS_DT = 3.0, 0.05
SHARED = dict(xlim=1.0, scale_rates=False, k_on=0.0, k_off=0.0, k_exit=0.0, site_capacity=2, rate_diffusion=0.5, rate_active=4.0)
# (local_kernel_sigma, N, beta): the batches of tests/test_gpu_gillespie_mixed.py, and an odd ring
BATCHES = dict(
    walls=dict(L=120, periodic=False, systems=[(0.02, 90, 1.1), (0.3, 70, 2.0),          # 0.3: folded table, reach beyond L
                                               (0.0, 60, 1.5),                            # global mean
                                               (0.004, 150, 0.6), (1e-4, 40, 1.0)]),      # a narrow table, the single tap
    ring=dict(L=150, periodic=True, systems=[(0.03, 100, 0.6), (0.3, 100, 2.0), (0.0, 100, 1.5), (1e-4, 100, 1.0)]),   # one N
    odd_ring=dict(L=97, periodic=True, systems=[(0.04, 70, 1.2), (0.0, 55, 0.8), (0.3, 70, 2.0)]),
)
RUNS = dict(walls=2, ring=2, odd_ring=1)
EXIT = dict(L=160, periodic=False, systems=[(0.02, 100, 0.9), (0.0, 93, 1.2), (0.3, 80, 0.7)],
            extra=dict(anchor_positions=[0.3, 0.7], anchor_radius=0.08, k_on=3.0, k_off=1.0, k_exit=0.5, rate_diffusion=0.6))
STATE_KEYS = ("scalars", "n_events", "n_recorded", "n_exits", "t_final")


@pytest.fixture(scope="module")
def gil():
    assert importlib.import_module(PKG + ".capi").device_count() >= 1
    return importlib.import_module(PKG + ".gillespie")


@pytest.fixture(scope="module")
def psys(gil):
    return importlib.import_module(PKG + ".particle_system")


def _batch_kw(gil, psys, batch, runs=1, extra=None, times=None, t_end=T):
    """The systems of a batch (`runs` per variant, a group each) and the keywords of run_mixed_structure_raw for them."""
    systems, group = [], []
    shared = dict(SHARED, **(extra or {}))
    for g, (sigma, N, beta) in enumerate(batch["systems"]):
        for run in range(runs):
            systems.append(psys.ParticleSystem(L=batch["L"], periodic=batch["periodic"], beta=beta + 0.1 * run, local_kernel_sigma=sigma,
                                               init="fixed", N=N, rng=np.random.default_rng(1000 * g + run), seed=77 + g, **shared))
            group.append(g)
    first = systems[0]
    inits = [ps.init_particles() for ps in systems]
    sig, _, owner = gil.mixed_variants([ps._sigma_grid for ps in systems])
    seeds, streams = gil.mixed_keys(systems, group)
    common = dict(L=first.L, K=first.K, periodic=first.periodic, rate_diffusion=first.rate_diffusion, rate_active=first.rate_active,
                  times_obs=np.arange(0.0, T, OBS_DT) if times is None else times, T=t_end, k_on=first.k_on, k_off=first.k_off,
                  k_exit=first.k_exit, anchor_mask=first.is_anchor_site)
    kw = dict(sigma_grids=sig, variant_of_system=owner, betas=[float(ps.beta) for ps in systems], states=inits, seeds=seeds,
              streams=streams, **common)
    return dict(systems=systems, group=np.array(group), inits=inits, seeds=seeds, common=common, kw=kw)


@pytest.fixture(scope="module")
def launches(gil, psys):
    """The launches tests 1 to 5 share: per batch, all modes and twelve, rows and states, from observation 0 on."""
    out = {}
    for name, batch in BATCHES.items():
        b = _batch_kw(gil, psys, batch, RUNS[name])
        b["full"] = gil.run_mixed_structure_raw(k_max=batch["L"], **b["kw"])
        b["twelve"] = gil.run_mixed_structure_raw(k_max=12, **b["kw"])
        out[name] = b
    return out


def _check_rows(systems, r, k_max, first_obs=0, min_recorded=2, field=True):
    """Every recorded row against NumPy on the state of the same observation, with the system's own field.  Returns the
    smallest and the largest live count seen."""
    S, M = r["structure"].shape[:2]
    assert r["structure"].shape == (S, M, 4 + 2 * k_max) and S == len(systems)
    n_lo, n_hi = None, 0
    for s, ps in enumerate(systems):
        L, n0, n_rec = ps.L, int(r["n0"][s]), int(r["n_recorded"][s])
        assert n_rec >= min_recorded
        assert not r["pos"][s, :, n0:].any() and not r["flags"][s, :, n0:].any()      # slots beyond n0
        for k in range(M):
            row = r["structure"][s, k]
            if k < first_obs or k >= n_rec:
                assert not row.any(), (s, k)
                continue
            live = (r["flags"][s, k] & 2) != 0
            p, sg = r["pos"][s, k][live].astype(np.int64), r["sigma"][s, k][live]
            n = p.size
            n_lo, n_hi = (n if n_lo is None else min(n_lo, n)), max(n_hi, n)
            cp, cm = np.bincount(p[sg > 0], minlength=L), np.bincount(p[sg < 0], minlength=L)
            counts = cp + cm
            assert row[0] == n and row[1] == int((counts * counts).sum()), (s, k)
            if field:
                m = np.asarray(ps.compute_local_m_field(cp, cm), dtype=float)
                np.testing.assert_allclose(row[2], m.sum(), rtol=1e-9, err_msg=f"sum m, system {s} observation {k}")
                np.testing.assert_allclose(row[3], (m * m).sum(), rtol=1e-9, err_msg=f"sum m^2, system {s} observation {k}")
            z = np.fft.fft(counts)[:k_max]
            err = max(np.abs(row[4::2] - z.real).max(), np.abs(row[5::2] - z.imag).max())
            assert err <= 1e-9 * max(n, 1), (s, k, err)
    return n_lo, n_hi


def _check_window(r, first_obs, rows=None, tag=""):
    """window, n_window, n_empty and head of every system against NumPy on the rows (of the same launch unless given)."""
    rows = r["structure"] if rows is None else rows
    S, M = rows.shape[:2]
    worst = [0.0, 0.0, 0.0]
    for s in range(S):
        n_rec = int(r["n_recorded"][s])
        assert np.array_equal(r["head"][s, first_obs:n_rec], rows[s, first_obs:n_rec, :4]), (tag, s)      # bit for bit
        assert not r["head"][s, n_rec:].any() and np.all(r["head"][s, :n_rec, 0] == r["scalars"][s, :n_rec, 0])
        win = rows[s, first_obs:n_rec]
        alive = win[:, 0] > 0
        win = win[alive]
        Mw = len(win)
        assert int(r["n_window"][s]) == Mw and int(r["n_empty"][s]) == int((~alive).sum()), (tag, s)
        w = r["window"][s]
        if Mw == 0:
            assert not w.any()
            continue
        n, re, im = win[:, :1], win[:, 4::2], win[:, 5::2]
        a_ref = np.hypot(re, im) / n
        assert np.all(np.abs(w[:, 0] - a_ref[0]) <= 4 * np.spacing(a_ref[0])), (tag, s)
        a = np.sqrt(re * re + im * im) / n                     # the header's expression: three roundings, a root, a division
        d = a - a[0]
        e1, e2 = np.abs(w[:, 1] - d.sum(axis=0)), np.abs(w[:, 2] - (d * d).sum(axis=0))
        b1, b2 = (Mw + 8) * 2.0 ** -52 * np.abs(d).sum(axis=0), (Mw + 8) * 2.0 ** -52 * (d * d).sum(axis=0)
        worst = [max(worst[0], float((np.abs(w[:, 0] - a_ref[0]) / np.spacing(a_ref[0])).max())),
                 max(worst[1], float((e1 / np.maximum(b1, 1e-300)).max())), max(worst[2], float((e2 / np.maximum(b2, 1e-300)).max()))]
        assert np.all(e1 <= b1), (tag, s, float((e1 - b1).max()))
        assert np.all(e2 <= b2), (tag, s, float((e2 - b2).max()))
        assert w[0, 1] == 0.0 and w[0, 2] == 0.0 and w[0, 0] == 1.0        # mode 0: n / n at every observation
    print(tag, "a0 error / ulp", worst[0], "sum d error / bound", worst[1], "sum d^2 error / bound", worst[2])


@pytest.mark.parametrize("name", list(BATCHES))
def test_rows_equal_numpy_on_the_states_of_the_same_launch(launches, name):
    b, L = launches[name], BATCHES[name]["L"]
    full, twelve = b["full"], b["twelve"]
    M = len(b["common"]["times_obs"])
    assert np.all(full["n_recorded"] == M) and np.all(full["n_events"] > 200)
    n_lo, _ = _check_rows(b["systems"], full, L)
    assert n_lo >= 40
    # twelve modes: the same trajectory, so the site sums are the bits of the launch above; the Fourier sums against NumPy
    for key in STATE_KEYS + ("pos", "sigma", "flags"):
        assert np.array_equal(twelve[key], full[key]), key
    assert np.array_equal(twelve["structure"][:, :, :4], full["structure"][:, :, :4])
    _check_rows(b["systems"], twelve, 12, field=False)
    if name == "walls":
        assert len({int(n) for n in full["n0"]}) == 5               # slots beyond n0 in four of the five variants


@pytest.mark.parametrize("name", list(BATCHES))
def test_window_sums_equal_numpy_on_the_rows_of_the_same_launch(launches, name):
    b = launches[name]
    _check_window(b["full"], 0, tag=f"{name} all modes")
    _check_window(b["twelve"], 0, tag=f"{name} twelve modes")
    M = len(b["common"]["times_obs"])
    assert np.all(b["full"]["n_window"] == M) and not b["full"]["n_empty"].any()
    assert b["full"]["window"].shape == (len(b["systems"]), BATCHES[name]["L"], 3) and np.all(b["full"]["window"][:, 1:, 2] > 0)


@pytest.mark.parametrize("name", ["walls", "odd_ring"])
def test_without_rows_and_states_the_same_sums(gil, launches, name):
    b = launches[name]
    bare = gil.run_mixed_structure_raw(k_max=BATCHES[name]["L"], want_rows=False, want_states=False, **b["kw"])
    assert bare["structure"] is None and bare["pos"] is None
    for key in ("window", "head", "n_window", "n_empty") + STATE_KEYS:
        assert np.array_equal(bare[key], b["full"][key]), key
    assert bare["bytes_back"] < b["full"]["bytes_back"]


@pytest.mark.parametrize("name", ["walls", "ring"])
def test_mixed_launch_equals_the_structure_launches_it_replaces(gil, launches, name):
    b, batch = launches[name], BATCHES[name]
    one_n = len({N for _, N, _ in batch["systems"]}) == 1
    assert one_n == (name == "ring")
    r = b["full"]
    for g in range(len(batch["systems"])):
        mine = np.flatnonzero(b["group"] == g)
        ps = b["systems"][mine[0]]
        alone = gil.run_structure_raw(sigma_grid=ps._sigma_grid, betas=[float(b["systems"][s].beta) for s in mine],
                                      states=[b["inits"][s] for s in mine], seed=b["seeds"][mine[0]], k_max=batch["L"], **b["common"])
        for j, s in enumerate(mine):
            n0 = len(b["inits"][s][0])
            for key in ("pos", "sigma", "flags"):
                assert np.array_equal(r[key][s, :, :n0], alone[key][j, :, :n0]), (g, key)
            for key in ("scalars", "n_events", "n_recorded", "n_exits"):
                assert np.array_equal(r[key][s], alone[key][j]), (g, key)
            if one_n:
                assert r["t_final"][s] == alone["t_final"][j]
            else:
                np.testing.assert_allclose(r["t_final"][s], alone["t_final"][j], rtol=1e-12)
            # the integers above are equal, so the states are at every observation: the rows must be, bit for bit
            assert np.array_equal(r["structure"][s], alone["structure"][j]), (g, s)


@pytest.mark.parametrize("name", ["walls", "ring"])
def test_order_is_only_an_order(gil, launches, name):
    b = launches[name]
    S = len(b["systems"])
    for order in (np.arange(S)[::-1], np.random.default_rng(4).permutation(S)):
        r = gil.run_mixed_structure_raw(k_max=BATCHES[name]["L"], order=order, **b["kw"])
        for key in ("structure", "window", "head", "n_window", "n_empty", "pos", "sigma", "flags", "exits") + STATE_KEYS:
            assert np.array_equal(r[key], b["full"][key]), key


def test_four_wavefronts_per_system_above_1024_slots(gil, psys):
    """n_cap > 1024 selects the 256-thread instantiation for the whole launch, also for its small system: k_max = 16 splits the
    slots over the wavefronts, k_max = L takes three passes of 256 modes."""
    L = 600
    batch = dict(L=L, periodic=False, systems=[(0.02, 1100, 0.8), (0.0, 40, 1.5)])
    times = np.arange(0.0, 1.0, 0.1)
    b = _batch_kw(gil, psys, batch, times=times, t_end=1.0)
    assert gil.plan_mixed_structure(L=L, K=2, periodic=False, sigma_grids=b["kw"]["sigma_grids"], n_systems=2, n_cap=1100, n_obs=10,
                                    k_max=16)["threads"] == 256
    for k_max in (16, L):
        r = gil.run_mixed_structure_raw(k_max=k_max, **b["kw"])
        assert np.all(r["n_recorded"] == 10) and np.all(r["n_events"] > 100)
        _check_rows(b["systems"], r, k_max, min_recorded=10)
        _check_window(r, 0, tag=f"256 threads, k_max {k_max}")
        assert np.all(r["n_window"] == 10)


def test_more_systems_than_modes(gil, psys, launches):
    """Ten systems, four modes: the window is [systems][modes][3] whichever of the two is larger, from the raw entry point and
    through the public function with both reductions."""
    b = launches["walls"]
    S = len(b["systems"])
    r = gil.run_mixed_structure_raw(k_max=4, **b["kw"])
    assert S == 10 and r["window"].shape == (S, 4, 3) and r["head"].shape[:2] == r["structure"].shape[:2] == (S, 60)
    assert np.array_equal(r["structure"][:, :, :12], b["twelve"]["structure"][:, :, :12])        # modes 0..3 of the twelve-mode launch
    assert np.array_equal(r["window"], b["twelve"]["window"][:, :4]) and np.array_equal(r["head"], b["twelve"]["head"])
    _check_window(r, 0, tag="ten systems, four modes")
    assert np.all(r["n_window"] == 60) and np.all(r["window"][:, 1:, 2] > 0)                      # every system's own sums, the last included

    def systems():
        return _batch_kw(gil, psys, BATCHES["walls"], RUNS["walls"])["systems"]

    group = [int(g) for g in b["group"]]
    dev = gil.run_batched_exact_structure_mixed(systems(), T=T, obs_dt=OBS_DT, start_fraction=0.5, k_max=4, groups=group)
    host = gil.run_batched_exact_structure_mixed(systems(), T=T, obs_dt=OBS_DT, start_fraction=0.5, k_max=4, groups=group, reduce="rows")
    assert len(dev) == len(host) == S
    for d, h in zip(dev, host):
        assert d["fft_mean"].shape == d["fft_std"].shape == (4,)
        _same_result(d, h, BATCHES["walls"]["L"])
    assert not np.array_equal(dev[0]["fft_mean"], dev[S - 1]["fft_mean"])


def test_first_obs_and_unreached_observations(gil, launches):
    b = launches["ring"]
    full, M, first = b["full"], len(b["common"]["times_obs"]), 25
    late = gil.run_mixed_structure_raw(k_max=150, first_obs=first, **b["kw"])
    assert not late["structure"][:, :first].any() and np.array_equal(late["structure"][:, first:], full["structure"][:, first:])
    assert np.array_equal(late["head"], full["head"])                  # the head rows start at observation 0 whatever first_obs is
    assert np.all(late["n_window"] == M - first)
    _check_window(late, first, tag="first_obs 25")
    _check_window(late, first, rows=full["structure"], tag="first_obs 25 on the rows from 0")   # nothing before first_obs went in
    assert not np.array_equal(late["window"], full["window"])
    none = gil.run_mixed_structure_raw(k_max=150, first_obs=M, **b["kw"])
    assert not none["structure"].any() and not none["window"].any() and not none["n_window"].any()
    assert np.array_equal(none["head"], full["head"]) and np.array_equal(none["n_events"], full["n_events"])
    short = gil.run_mixed_structure_raw(k_max=150, first_obs=first, **dict(b["kw"], T=2.32))   # observations from t = 2.35 on are never reached
    for s in range(len(b["systems"])):
        n_rec = int(short["n_recorded"][s])
        assert first + 10 <= n_rec <= 47
        assert int(short["n_window"][s]) == n_rec - first
        assert not short["structure"][s, n_rec:].any() and not short["structure"][s, :first].any() and not short["head"][s, n_rec:].any()
        assert np.array_equal(short["structure"][s, first:n_rec], full["structure"][s, first:n_rec])   # same key: same trajectory up to there
    _check_window(short, first, tag="T before the last observation")


def test_particles_leave_during_the_window(gil, psys):
    b = _batch_kw(gil, psys, EXIT, extra=EXIT["extra"])
    first = 20
    r = gil.run_mixed_structure_raw(k_max=EXIT["L"], first_obs=first, **b["kw"])
    assert np.all(r["n_recorded"] == 60) and np.all(r["n_exits"] > 0)
    for s in range(3):
        n = r["head"][s, first:, 0]
        assert n[-1] < n[0] and n[-1] >= 1                             # n_t falls during the window, nobody runs empty
    n_lo, n_hi = _check_rows(b["systems"], r, EXIT["L"], first_obs=first)
    assert n_lo < n_hi
    _check_window(r, first, tag="anchors_exit")
    assert np.all(r["n_window"] == 60 - first) and not r["n_empty"].any()


def _same_result(a, b, L):
    fold = lambda k: min(k, L - k)
    assert list(a)[:8] == list(b)[:8]
    for key in ("var_mean", "var_std", "low_k_power", "m_local_var", "lowk_variance"):
        np.testing.assert_allclose(a[key], b[key], rtol=1e-9, atol=1e-12, err_msg=key)
    np.testing.assert_allclose(a["fft_mean"], b["fft_mean"], rtol=1e-9)
    np.testing.assert_allclose(a["fft_std"], b["fft_std"], rtol=1e-8, atol=1e-9)
    if fold(a["dominant_k"]) != fold(b["dominant_k"]):                  # two candidates that tie within the bar
        np.testing.assert_allclose(a["fft_mean"][a["dominant_k"]], b["fft_mean"][b["dominant_k"]], rtol=1e-9)


def test_public_function_device_reduction_against_rows(gil, psys):
    kw = dict(L=256, xlim=1.0, rate_diffusion=0.3, rate_active=2.0, init="fixed", scale_rates=False, site_capacity=2, k_on=0.0, k_off=0.0,
              k_exit=0.0, seed=77)
    cases = [(0.02, 200, 0.5), (0.0, 150, 2.5), (0.3, 200, 3.0), (0.02, 120, 1.5)]

    def systems(cs=cases):
        return [psys.ParticleSystem(beta=b, N=n, local_kernel_sigma=sg, rng=np.random.default_rng(900 + i), **kw) for i, (sg, n, b) in enumerate(cs)]

    groups = [0, 1, 2, 0]
    for k_max in (None, 12):
        dev = gil.run_batched_exact_structure_mixed(systems(), T=3.0, obs_dt=0.1, start_fraction=0.4, k_max=k_max, groups=groups)
        host = gil.run_batched_exact_structure_mixed(systems(), T=3.0, obs_dt=0.1, start_fraction=0.4, k_max=k_max, groups=groups, reduce="rows")
        assert len(dev) == len(host) == 4 and dev[0]["fft_mean"].shape == (256 if k_max is None else 12,)
        for d, h in zip(dev, host):
            assert list(d) == ["var_mean", "var_std", "fft_mean", "fft_std", "dominant_k", "low_k_power", "m_local_var", "lowk_variance"]
            _same_result(d, h, 256)
        assert dev[0]["var_mean"] != dev[1]["var_mean"]
    ser_d = gil.run_batched_exact_structure_mixed(systems(), T=3.0, obs_dt=0.1, start_fraction=0.4, k_max=12, groups=groups, return_series=True)
    ser_h = gil.run_batched_exact_structure_mixed(systems(), T=3.0, obs_dt=0.1, start_fraction=0.4, k_max=12, groups=groups, return_series=True,
                                                  reduce="rows")
    for d, h, d0 in zip(ser_d, ser_h, dev):
        assert d["var_series"].shape == d["m_series"].shape == d["times_obs"].shape == (30,) and "fft_amp_series" not in d
        assert h["fft_amp_series"].shape == (30, 12)
        assert np.array_equal(d["var_series"], h["var_series"]) and np.array_equal(d["m_series"], h["m_series"])
        assert np.all(np.abs(d["m_series"]) <= 1.0) and np.all(d["var_series"] > 0)
        _same_result(d, h, 256)
        assert np.array_equal(d["fft_mean"], d0["fft_mean"])            # the window's results do not depend on the series
    # a uniform batch: one variant, against the unmixed public function (its launch: key of the first system, index = place)
    uniform = [(0.02, 200, 0.5), (0.02, 150, 2.5), (0.02, 200, 3.0)]
    dev = gil.run_batched_exact_structure_mixed(systems(uniform), T=3.0, obs_dt=0.1, start_fraction=0.4)
    ref = gil.run_batched_exact_structure(systems(uniform), T=3.0, obs_dt=0.1, start_fraction=0.4)
    for d, h in zip(dev, ref):
        _same_result(d, h, 256)


PS_KW = dict(L=300, xlim=1.0, site_capacity=1, scale_rates=False, rate_diffusion=0.5, rate_active=4.0, seed=5)
BETAS, N_RUNS, RUN_KW = [0.6, 1.2, 2.0], 2, dict(T=6.0, obs_dt=0.1)
RNG_SEEDS = [[31, 32], [41, 42], [51, 52]]


def test_sigma_structure_sweep_in_one_launch_equals_the_host_loop():
    ens = importlib.import_module(PKG + ".ensemble")
    sigmas = [0.02, 0.5, 0.0, 1e-4]
    args = (sigmas, BETAS, N_RUNS, PS_KW, dict(N=120, init="fixed"), RUN_KW)
    loop = ens.sweep_sigmas_for_structures(*args, rng_seeds=RNG_SEEDS, one_launch=False)
    one, series = ens.sweep_sigmas_for_structures(*args, rng_seeds=RNG_SEEDS, return_series=True)
    assert list(one) == list(loop) == list(series) == sigmas
    M = 60
    for sigma in sigmas:
        assert list(one[sigma]) == list(loop[sigma]) == list(series[sigma]) == BETAS
        for beta in BETAS:
            a, b = one[sigma][beta], loop[sigma][beta]
            assert list(a) == list(b) and len(a["raw"]) == len(b["raw"]) == N_RUNS
            for x, y in zip(a["raw"], b["raw"]):
                _same_result(x, y, 300)
            for key in ("var_mean", "var_se", "low_k_power_mean", "low_k_power_se", "m_local_var_mean", "m_local_var_se", "lowk_var_mean",
                        "lowk_var_se"):
                np.testing.assert_allclose(a[key], b[key], rtol=1e-9, atol=1e-12, err_msg=key)
            np.testing.assert_allclose(a["fft_mean_mean"], b["fft_mean_mean"], rtol=1e-9)
            s = series[sigma][beta]
            assert s["m_abs_series"].shape == s["var_series"].shape == s["times_obs"].shape == (M,)
            assert np.all(s["m_abs_series"] >= 0) and np.all(s["m_abs_series"] <= 1) and np.all(s["var_series"] > 0)
    assert not np.array_equal(one[0.02][1.2]["fft_mean_mean"], one[0.0][1.2]["fft_mean_mean"])
    assert one[0.02][1.2]["low_k_power_mean"] != one[0.0][1.2]["low_k_power_mean"]    # (var(total) cannot differ: K = 1 makes sum c^2 = n)


def test_one_launch_takes_less_kernel_time_and_fewer_bytes(gil):
    """Eight widths, eight systems each: 64 one-wavefront workgroups are all resident at once, so the mixed launch should take
    about as long as its slowest system, where the eight structure launches run one after the other.  A condition, not a
    figure: the ratio is below 1; likewise the bytes that come back without the rows."""
    L, N, k_max = 1000, 300, 64
    rng = np.random.default_rng(12)
    widths = [w * L for w in (0.0, 1e-4, 0.002, 0.005, 0.01, 0.02, 0.05, 0.3)]
    common = dict(L=L, K=1, periodic=False, rate_diffusion=0.5, rate_active=4.0, times_obs=np.arange(0.0, 2.0, 0.1), T=2.0, want_states=False)
    groups = [[(rng.choice(L, size=N, replace=False), rng.choice([1, -1], size=N).astype(np.int8)) for _ in range(8)] for _ in widths]
    tiny = [(np.array([3, 9]), np.array([1, -1], np.int8))]
    gil.run_structure_raw(sigma_grid=widths[5], betas=[1.0], states=tiny, seed=1, k_max=k_max, **common)    # both kernels loaded before the clock counts
    gil.run_mixed_structure_raw(sigma_grids=[widths[5]], variant_of_system=[0], betas=[1.0], states=tiny, seed=1, k_max=k_max, **common)
    apart = [gil.run_structure_raw(sigma_grid=w, betas=[1.0] * 8, states=g, seed=100 + i, k_max=k_max, first_obs=10, **common)
             for i, (w, g) in enumerate(zip(widths, groups))]
    mixed_kw = dict(sigma_grids=widths, variant_of_system=np.repeat(np.arange(8), 8).astype(np.int32), betas=[1.0] * 64,
                    states=[st for g in groups for st in g], seeds=np.repeat(100 + np.arange(8), 8), streams=np.tile(np.arange(8), 8),
                    k_max=k_max, first_obs=10, **common)
    mixed = gil.run_mixed_structure_raw(want_rows=False, **mixed_kw)
    with_rows = gil.run_mixed_structure_raw(want_rows=True, **mixed_kw)
    assert np.array_equal(mixed["scalars"], np.concatenate([a["scalars"] for a in apart]))                 # the same work
    assert np.array_equal(with_rows["structure"], np.concatenate([a["structure"] for a in apart]))
    assert np.array_equal(mixed["window"], with_rows["window"])
    total = sum(a["kernel_ms"] for a in apart)
    print(f"mixed {mixed['kernel_ms']:.3f} ms, eight launches {total:.3f} ms, ratio {mixed['kernel_ms'] / total:.3f}")
    print(f"bytes back: {mixed['bytes_back']} without rows, {with_rows['bytes_back']} with rows")
    assert mixed["kernel_ms"] < total
    assert mixed["bytes_back"] < with_rows["bytes_back"]
