"""CPU suite: the exact loop with anchor-capture and cluster statistics (include/gillespie_capture.h) as far as it can be checked
without a GPU -- the library exports what the header declares, gilc_plan_info is mirrored faithfully, the plan (pure host
arithmetic) picks the shape and reports the bytes the header documents, every refusal by its text, and the host side of the
study: the site -> anchor lookup and `capture_observables` against restatements of PARTICLE_solver_CLASS.py:766-976."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"
ERR_ARG, ERR_NODEVICE = -1, -4
BATCH, LARGE = 0, 1


@pytest.fixture(scope="module")
def capi():
    mod = importlib.import_module(PKG + ".capi")
    if not os.path.exists(mod.LIB_PATH):
        importlib.import_module(PKG + ".build").build()
    return mod


@pytest.fixture(scope="module")
def gil(capi):
    return importlib.import_module(PKG + ".gillespie")


@pytest.fixture(scope="module")
def obs(capi):
    return importlib.import_module(PKG + ".observables")


def test_capture_header_symbols_exported_and_plan_info_layout(capi, gil):
    with open(os.path.join(os.path.dirname(capi.HEADER_PATH), "gillespie_capture.h")) as fh:
        text = fh.read()
    names = sorted(set(re.findall(r"\b(gilc_[a-z_0-9]+)\s*\(", text)))
    assert names == ["gilc_last_error", "gilc_plan", "gilc_run"]
    lib = C.CDLL(capi.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/gillespie_capture.h but not exported"
    assert not hasattr(lib, "gilc_large_run") and not hasattr(lib, "gilc_large_plan")     # the bridge between the two sources stays inside
    assert '#include "gillespie.h"' in text and "typedef struct gil_params" not in text     # gil_params is reused, not restated
    for name, value in (("GILC_NFIXED", 9), ("GILC_MAX_GROUPS", 32), ("GILC_MAX_CBINS", 64), ("GILC_MAX_HBINS", 256)):
        assert re.search(rf"#define {name} {value}\b", text), name
    assert gil.GILC_NFIXED == 9 and len(gil.CAPTURE_COLUMNS) == 9
    body = re.search(r"typedef struct gilc_plan_info \{(.*?)\} gilc_plan_info;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [d.split()[-1] for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in gil.GilcPlanInfo._fields_]
    assert C.sizeof(gil.GilcPlanInfo) == 4 * 4 + 2 * 8


def _lds_of_loop(L, n_cap, tlen, nt):
    """gillespie_hip.hip's LDS of one system, by the formula of its host driver (batch_shape)."""
    return (2 * L + ((tlen + 2) & ~1) + n_cap + (n_cap & 1) + 8 + 5 * nt + 8) * 8 + (3 * n_cap + 16) * 4 + ((n_cap + 15) & ~15) + 2 * ((L + 15) & ~15)


def _capture_bytes(nt, G, c_bins, h_bins, n_cap=0):
    """the capture slots the header documents, plus the bind times where they live in LDS"""
    return 8 * (12 + nt // 64 + 2 * h_bins + G + c_bins) + 8 * n_cap


def test_plan_row_length_and_shape(gil):
    """sigma_grid = 5 with walls: taps at distances 0 .. 20, table_len 21."""
    kw = dict(K=1, periodic=False, sigma_grid=5.0, n_systems=7, n_obs=41, n_groups=3, c_bins=16, h_bins=40)
    for L, n_cap, nt in ((160, 100, 64), (900, 1100, 256), (4096, 2048, 256)):
        p = gil.plan_capture(L=L, n_cap=n_cap, **kw)
        assert p["row_len"] == 9 + 3 + 16
        lds = ((_lds_of_loop(L, n_cap, 21, nt) + 7) & ~7) + _capture_bytes(nt, 3, 16, 40, n_cap)
        fits = lds <= 160 * 1024                                   # (4096, 2048): whatever the arithmetic gives
        assert p["shape"] == (BATCH if fits else LARGE), (L, n_cap, lds)
        if fits:
            assert (p["threads"], p["lds_bytes"], p["work_bytes"]) == (nt, lds, L * 4)
        if L < 4096:
            assert fits
    big = gil.plan_many_large(L=4200, n_cap=2000, n_obs=41, K=1, periodic=False, sigma_grid=5.0, n_systems=7)
    p = gil.plan_capture(L=4200, n_cap=2000, **kw)
    assert p["shape"] == LARGE and p["threads"] == 1024 and p["row_len"] == 28
    assert p["lds_bytes"] == big["lds_bytes"] + _capture_bytes(1024, 3, 16, 40)
    assert p["work_bytes"] == 7 * (big["work_bytes_per_system"] + 8 * 2000) + 4200 * 4
    rest = 7 * (41 * 12 * 8 + 2000 * 24 + 24 + 41 * 28 * 8 + 2 * 40 * 8 + 32)
    assert p["output_bytes"] == rest + 7 * 41 * 2000 * 6
    assert gil.plan_capture(L=4200, n_cap=2000, want_states=False, **kw)["output_bytes"] == rest
    p = gil.plan_capture(L=1000, n_cap=2100, **dict(kw, n_groups=0))      # more slots than a workgroup holds
    assert p["shape"] == LARGE and p["row_len"] == 25
    # the capture slots tip a system that the plain loop still holds over the 160 KB
    tight = dict(K=1, periodic=False, sigma_grid=600.0, n_systems=1, n_obs=2, L=4096, n_cap=2048)     # table_len int(4 * 600 + 0.5) + 1
    own = (_lds_of_loop(4096, 2048, 2401, 256) + 7) & ~7
    assert own + _capture_bytes(256, 0, 2, 1, 2048) <= 160 * 1024 < own + _capture_bytes(256, 32, 64, 256, 2048)
    p = gil.plan_capture(n_groups=0, c_bins=2, h_bins=1, **tight)
    assert p["shape"] == BATCH and p["lds_bytes"] == own + _capture_bytes(256, 0, 2, 1, 2048)
    assert gil.plan_capture(n_groups=32, c_bins=64, h_bins=256, **tight)["shape"] == LARGE


def test_plan_refusals_name_the_number(capi, gil):
    kw = dict(L=1000, K=1, periodic=False, sigma_grid=5.0, n_systems=2, n_cap=900, n_obs=41)
    for bad, text in ((dict(n_groups=33), "gilc_plan: n_groups = 33 is outside [0, 32]"),
                      (dict(n_groups=-1), "gilc_plan: n_groups = -1 is outside [0, 32]"),
                      (dict(c_bins=1), "gilc_plan: c_bins = 1 is outside [2, 64]"),
                      (dict(c_bins=65), "gilc_plan: c_bins = 65 is outside [2, 64]"),
                      (dict(h_bins=0), "gilc_plan: h_bins = 0 is outside [1, 256]"),
                      (dict(h_bins=257), "gilc_plan: h_bins = 257 is outside [1, 256]"),
                      (dict(first_obs=42), "gilc_plan: first_obs = 42 is outside [0, n_obs = 41]"),
                      (dict(first_obs=-1), "gilc_plan: first_obs = -1 is outside [0, n_obs = 41]")):
        with pytest.raises(capi.ApsError) as exc:
            gil.plan_capture(**kw, **bad)
        assert exc.value.code == ERR_ARG and str(exc.value).endswith(text), (bad, str(exc.value))
    assert gil.plan_capture(n_groups=32, c_bins=64, h_bins=256, first_obs=41, **kw)["row_len"] == 9 + 32 + 64
    assert gil.plan_capture(n_groups=0, c_bins=2, h_bins=1, **kw)["row_len"] == 11
    with pytest.raises(capi.ApsError) as exc:                            # the large shape's own limits
        gil.plan_capture(**dict(kw, L=(1 << 25) + 1))
    assert str(exc.value).endswith("gilc_plan: L must be in [2, 2^25]")
    with pytest.raises(capi.ApsError) as exc:
        gil.plan_capture(c_bins=64, want_states=False, **dict(kw, L=1 << 25, K=4, n_cap=1 << 20, n_systems=65535, sigma_grid=0.0))
    assert "bytes of work memory and" in str(exc.value) and str(exc.value).endswith(f"more than the {1 << 38} bytes a plan accepts")


def test_run_refusals_come_before_any_device(gil):
    lib = gil._lib()
    L = 64
    keep = [np.array([0.5]), np.array([0.0, 0.01]), np.array([1], np.int32), np.array([0], np.int32), np.array([1], np.int8),
            np.zeros(2 * (9 + 2 + 4), np.int64), np.zeros(2 * 4, np.int64), np.zeros(4)]
    mask = np.zeros(L, np.uint8)
    mask[10:20] = 1
    par = gil.GilParams(L=L, K=1, periodic=1, n_systems=1, n_cap=1, n_obs=2, ref_obs=-1, rate_diffusion=0.1, rate_active=1.0, T=0.01,
                        max_events=16, beta=keep[0].ctypes.data, times_obs=keep[1].ctypes.data, anchor_mask=mask.ctypes.data)
    ms = C.c_double()

    def call(groups=None, n_groups=2, c_bins=4, h_bins=4, h_dt=0.1, first_obs=0, rows=keep[5], p=par):
        rc = lib.gilc_run(C.byref(p), gil._p(groups), n_groups, c_bins, h_bins, h_dt, first_obs, gil._p(keep[2]), gil._p(keep[3]),
                          gil._p(keep[4]), *[None] * 11, gil._p(rows), gil._p(keep[6]), gil._p(keep[7]), C.byref(ms))
        return rc, lib.gilc_last_error().decode()

    assert call(rows=None) == (ERR_ARG, "gilc_run: null argument")       # the capture outputs are required
    assert call(n_groups=33) == (ERR_ARG, "gilc_run: n_groups = 33 is outside [0, 32]")
    assert call(c_bins=1) == (ERR_ARG, "gilc_run: c_bins = 1 is outside [2, 64]")
    assert call(h_bins=300) == (ERR_ARG, "gilc_run: h_bins = 300 is outside [1, 256]")
    assert call(first_obs=3) == (ERR_ARG, "gilc_run: first_obs = 3 is outside [0, n_obs = 2]")
    for h_dt in (0.0, -0.5, float("inf"), float("nan")):
        rc, text = call(h_dt=h_dt)
        assert rc == ERR_ARG and text.startswith("gilc_run: h_dt = ") and text.endswith(" must be positive and finite"), text
    assert "-0.5" in call(h_dt=-0.5)[1]
    groups = np.full(L, -1, np.int32)
    groups[10:15], groups[15:20] = 0, 1
    groups[17] = 2
    assert call(groups) == (ERR_ARG, "gilc_run: group id 2 at site 17 is outside [-1, n_groups = 2)")
    groups[17] = -2
    assert call(groups) == (ERR_ARG, "gilc_run: group id -2 at site 17 is outside [-1, n_groups = 2)")
    groups[17], groups[20] = 1, 1
    assert call(groups) == (ERR_ARG, "gilc_run: site 20 carries group 1 but anchor_mask does not mark it")
    groups[20] = -1
    bare = gil.GilParams.from_buffer_copy(par)
    bare.anchor_mask = None
    assert call(groups, p=bare) == (ERR_ARG, "gilc_run: site 10 carries group 0 but anchor_mask does not mark it")
    rc, text = call(groups)                                              # acceptable: only the device is missing, or it runs
    assert (rc, text) == (ERR_NODEVICE, "gilc_run: no HIP device") or rc == 0


def test_run_capture_raw_fails_loudly_without_a_gpu(capi, gil):
    if capi.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(capi.ApsError) as exc:
        gil.run_capture_raw(L=64, K=1, periodic=True, sigma_grid=0.0, rate_diffusion=0.1, rate_active=1.0, betas=[0.5],
                            states=[(np.array([0]), np.array([1]))], times_obs=[0.0, 0.01], T=0.01, max_events=16)
    assert exc.value.code == ERR_NODEVICE and "gilc_run: no HIP device" in str(exc.value)


class _Anchored:
    """What anchor_groups reads of a ParticleSystem."""

    def __init__(self, L, centres, reach):
        self.L, self.anchor_idxs = L, np.array(centres, dtype=int)
        mask = np.zeros(L, bool)
        for c in centres:
            mask[max(0, c - reach):min(L - 1, c + reach) + 1] = True
        self.anchor_idx_array = np.flatnonzero(mask)


def _site_to_gid(ps):
    """PARTICLE_solver_CLASS.py:923-928, restated."""
    site_to_gid = np.full(ps.L, -1, dtype=int)
    centers = np.array(ps.anchor_idxs, dtype=int)
    for s in np.array(ps.anchor_idx_array, dtype=int):
        site_to_gid[s] = int(np.argmin(np.abs(centers - s)))
    return site_to_gid


def test_anchor_groups_equal_the_reference_lookup(obs):
    for ps in (_Anchored(100, [20, 30, 45], 8), _Anchored(64, [5, 9, 60], 6), _Anchored(200, [50, 58, 66], 12)):   # overlapping radii
        got = obs.anchor_groups(ps)
        assert got.dtype == np.int32 and np.array_equal(got, _site_to_gid(ps)) and set(got) == {-1, 0, 1, 2}
    tie = _Anchored(40, [10, 16], 5)                                     # site 13 is three from both centres: the first one
    got = obs.anchor_groups(tie)
    assert got[13] == 0 and got[14] == 1 and np.array_equal(got, _site_to_gid(tie))
    psys = importlib.import_module(PKG + ".particle_system")
    real = psys.ParticleSystem(L=300, xlim=1.0, rate_diffusion=0.2, rate_active=5.0, beta=0.7, init="fixed", N=10, scale_rates=False,
                               anchor_positions=[0.25, 0.60, 0.80], anchor_radius=0.03)
    got = obs.anchor_groups(real)
    assert np.array_equal(got, _site_to_gid(real)) and np.array_equal(got >= 0, real.is_anchor_site) and got.max() == 2
    none = psys.ParticleSystem(L=50, xlim=1.0, rate_diffusion=0.2, rate_active=5.0, beta=0.7, init="fixed", N=10, scale_rates=False)
    assert np.array_equal(obs.anchor_groups(none), np.full(50, -1))


def _cumulative_exits_reference(times, exit_t, exit_x, site_to_gid, L, nA):
    """PARTICLE_solver_CLASS.py:931-954, restated."""
    gid = np.array([site_to_gid[x] if 0 <= x < L else -1 for x in exit_x])
    dt = times[1] - times[0] if len(times) > 1 else 1.0
    edges = np.concatenate([times, [times[-1] + dt]])
    centers_t = edges[:-1] + 0.5 * np.diff(edges)
    counts = np.zeros((len(centers_t), nA), dtype=int)
    for t, g in zip(exit_t, gid):
        if g >= 0:
            b = np.searchsorted(edges, t, side="right") - 1
            if 0 <= b < len(centers_t):
                counts[b, g] += 1
    cumA = np.cumsum(counts, axis=0)
    return cumA, cumA.sum(axis=1)


def test_capture_observables_on_a_hand_built_run(obs):
    L, dx = 12, 1.0 / 12
    times = np.arange(6) * 0.5
    occ = np.array([[1, 2, 0, 0, 1, 1, 1, 0, 0, 0, 0, 1],               # touches both ends of the (periodic) lattice: two clusters, 2 and 1
                    [0, 1, 1, 0, 0, 1, 0, 1, 0, 0, 1, 0],
                    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                    [3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
                    [0, 1, 1, 1, 1, 1, 0, 0, 1, 0, 0, 0],
                    [1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 1]])
    count = [10, 9, 9, 7, 7, 6]
    groups = np.full(L, -1)
    groups[2:5], groups[8:10] = 0, 1
    exit_t = [0.3, 1.0, 1.2, 2.4, 2.6, 2.6]                              # 1.0 is an observation time: it falls in the bin above it
    exit_x = [3, 8, 6, 4, 9, 2]                                          # site 6 belongs to no anchor
    out = dict(times_obs=times, total_list=occ / (np.maximum(occ.sum(axis=1, keepdims=True), 1) * dx), particle_count_list=count,
               exit_times=exit_t, exit_positions=exit_x)
    got = obs.capture_observables(out, groups, c_bins=4)
    assert np.array_equal(got["occupied_sites"], [6, 5, 0, 12, 6, 7]) and np.array_equal(got["n_clusters"], [3, 4, 0, 1, 2, 6])
    assert np.array_equal(got["largest_cluster"], [3, 2, 0, 12, 5, 2]) and np.array_equal(got["sum_size2"], [14, 7, 0, 144, 26, 9])
    assert np.array_equal(got["cluster_hist"], [[1, 1, 1, 0], [3, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1], [1, 0, 0, 1], [5, 1, 0, 0]])
    cum, total = _cumulative_exits_reference(times, exit_t, exit_x, groups, L, 2)
    assert np.array_equal(got["cumulative_exits"], cum) and np.array_equal(got["cumulative_exits_total"], total)
    assert np.array_equal(cum, [[1, 0], [1, 0], [1, 1], [1, 1], [2, 1], [3, 2]])       # the exit at t = 1.0 sits in bin 2, not bin 1
    n_t = np.array(count, dtype=float)
    flux = np.clip(-np.gradient(n_t, times), 0, None)
    np.testing.assert_allclose(got["survival"], n_t / 10.0, rtol=0, atol=0)
    np.testing.assert_allclose(got["fpt_pdf"], flux / 10.0, rtol=1e-15)
    np.testing.assert_allclose(got["fpt_pdf_cond"], flux / 4.0, rtol=1e-15)
    assert got["exit_position_hist"].shape == (50,) and got["exit_position_hist"].sum() == 6
    assert np.array_equal(got["exit_position_hist"], np.histogram(np.array(exit_x) / L, bins=50, range=(0.0, 1.0))[0])
    nobody_left = dict(out, particle_count_list=[10] * 6, exit_times=[], exit_positions=[])
    quiet = obs.capture_observables(nobody_left, groups, c_bins=4)
    assert not quiet["fpt_pdf_cond"].any() and not quiet["cumulative_exits"].any() and quiet["cumulative_exits"].shape == (6, 2)


def test_device_capture_maps_rows_to_the_reference_bins(obs):
    """Row k counts the exits before times_obs[k]: the reference's bin b is row b + 1, its last bin the last row."""
    times = np.arange(4) * 0.5
    G, c_bins = 2, 3
    rows = np.zeros((4, 9 + G + c_bins), np.int64)
    rows[:, 9], rows[:, 10] = [0, 1, 1, 3], [0, 0, 2, 2]
    rows[:, 5:9] = [[4, 2, 3, 10], [4, 2, 3, 10], [3, 3, 1, 3], [2, 1, 2, 4]]
    rows[:, 11:] = [[1, 0, 1], [1, 0, 1], [3, 0, 0], [0, 1, 0]]
    exits = np.array([[0.2, 3.0, 0], [0.7, 9.0, 1], [0.8, 9.0, 2], [1.1, 3.0, 3], [1.2, 4.0, 4]])
    hist = np.array([[2, 1, 0], [0, 0, 5]], np.int64)
    sums = np.array([[0.9, 0.35], [6.0, 7.4]])
    got = obs.DeviceCapture(times, 12, G, c_bins, 0.25).result([8, 7, 5, 3], rows, exits, hist, sums)
    assert np.array_equal(got["cumulative_exits"], [[1, 0], [1, 2], [3, 2], [3, 2]]) and np.array_equal(got["cumulative_exits_total"], [1, 3, 5, 5])
    assert np.array_equal(got["largest_cluster"], [3, 3, 1, 2]) and np.array_equal(got["cluster_hist"], rows[:, 11:])
    assert np.array_equal(got["life_count"], [3, 5]) and np.array_equal(got["life_edges"], [0.0, 0.25, 0.5, 0.75])
    np.testing.assert_allclose(got["life_mean"], [0.3, 1.2], rtol=1e-15)
    np.testing.assert_allclose(got["life_var"], [0.35 / 3 - 0.09, 7.4 / 5 - 1.44], rtol=1e-12)
    np.testing.assert_allclose(got["survival"], [1.0, 7 / 8, 5 / 8, 3 / 8], rtol=1e-15)
    empty = obs.DeviceCapture(times, 12, G, c_bins, 0.25).result([8, 8, 8, 8], rows * 0, exits[:0], hist * 0, sums * 0)
    assert np.all(np.isnan(empty["life_mean"])) and not empty["exit_position_hist"].any()
