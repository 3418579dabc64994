"""CPU suite: mixed batches of LARGE systems of the exact event loop (include/gillespie_mixed_many.h) as far as they can be
checked without a GPU -- the library exports what the header declares, gilxm_plan_info is mirrored faithfully, the plan (pure
host arithmetic) gives the numbers the header documents, every refusal by its text, the large shape's keys, and that the large
shape is still refused wherever `allow_large` is left out.

One refusal of the header cannot be provoked through the ABI: a launch over 160 KB of LDS.  The table region holds at most 10000
doubles (a longer table stays in global memory), and n_cap <= 2^20 gives at most 4096 rate blocks, so the largest launch needs
8 * (10000 + 4144) + 4 * (8192 + 32) = 146048 bytes, below the 163840 of a workgroup; `test_plan_numbers` pins that number.  The
check guards the day one of the limits moves."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"
ERR_ARG, ERR_NODEVICE = -1, -4
LDS_LIMIT = 160 * 1024
PLAN_MAX = 2 ** 38


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
def ens(capi):
    return importlib.import_module(PKG + ".ensemble")


@pytest.fixture(scope="module")
def psys(capi):
    return importlib.import_module(PKG + ".particle_system")


def _struct_fields(text, name):
    body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [d.split()[-1].lstrip("*") for d in body.split(";") if d.strip()]


def test_header_symbols_exported_and_struct_layout(capi, gil):
    with open(os.path.join(os.path.dirname(capi.HEADER_PATH), "gillespie_mixed_many.h")) as fh:
        text = fh.read()
    names = sorted(set(re.findall(r"\b(gilxm_[a-z_0-9]+)\s*\(", text)))
    assert names == ["gilxm_last_error", "gilxm_plan", "gilxm_run"]
    lib = C.CDLL(capi.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/gillespie_mixed_many.h but not exported"
    with open(capi.LIB_PATH, "rb") as fh:                          # nothing else with the prefix leaves the library
        exported = set(re.findall(rb"\x00(gilxm_[a-z_0-9]+)\x00", fh.read()))
    assert {e.decode() for e in exported if hasattr(lib, e.decode())} == set(names)
    # gil_params and gilx_variants are reused, not restated
    assert '#include "gillespie.h"' in text and '#include "gillespie_mixed.h"' in text
    assert "typedef struct gil_params" not in text and "typedef struct gilx_variants" not in text
    assert _struct_fields(text, "gilxm_plan_info") == [f[0] for f in gil.GilxmPlanInfo._fields_]
    assert C.sizeof(gil.GilxmPlanInfo) == 6 * 4 + 3 * 8
    assert gil.GilxmPlanInfo.lds_bytes.offset == 20 and gil.GilxmPlanInfo.table_doubles.offset == 24
    assert gil.GilxmPlanInfo.output_bytes.offset == 40
    # registered with the other entry points and plans, with gilx_run's argument list
    assert gil.ENTRIES["gilxm_run"].front == gil.ENTRIES["gilx_run"].front and gil.ENTRIES["gilxm_run"].last_error == "gilxm_last_error"
    assert gil.PLANS["gilxm_plan"][0] == "gilxm_last_error" and gil.PLANS["gilxm_plan"][2] is gil.GilxmPlanInfo
    with open(os.path.join(os.path.dirname(capi.HEADER_PATH), "gillespie_mixed.h")) as fh:
        assert "gillespie_mixed_many.h" in fh.read()               # the batch shape's header points here


def _lds(max_tlen_lds, n_blocks):
    """The header's formula for the dynamic LDS of a workgroup."""
    region = ((max_tlen_lds + 2) & ~1) if max_tlen_lds >= 0 else 0
    return 8 * (region + 32 + 4 * 1024 + 4 + 12) + 4 * (2 * n_blocks + 32)


def _work(L, K, N):
    return N * 21 + L * 24 + L * K * 4 + -(-N // 256) * 8


def _outputs(S, O, N, states):
    return S * ((O * N * 6 if states else 0) + O * 12 * 8 + N * 24 + 24)


def test_plan_numbers(gil):
    """sigma_grid = 5 with walls: taps at distances 0 .. 20, table length 21; 2: length 9; 0.012: the single tap; 0: no table
    (the lengths test_gillespie_mixed_cpu.py states for the batch shape: the tables come from the same host code)."""
    kw = dict(L=8192, K=1, periodic=False, n_systems=7, n_obs=41)
    # every variant in LDS: the region is the longest table's, all tables back to back with their closing zeros
    p = gil.plan_mixed_many(sigma_grids=[5.0, 0.0, 0.012, 2.0], n_cap=6144, variant_of_system=[0, 1, 2, 3, 3, 3, 0], **kw)
    assert p == dict(n_systems=7, n_blocks=24, max_tlen=21, max_tlen_lds=21, n_global=0, lds_bytes=_lds(21, 24),
                     table_doubles=22 + 1 + 2 + 10, work_bytes_per_system=_work(8192, 1, 6144), output_bytes=_outputs(7, 41, 6144, True))
    assert p["lds_bytes"] == 8 * (22 + 4144) + 4 * 80                     # by hand
    p = gil.plan_mixed_many(sigma_grids=[2.0, 0.0], n_cap=300, want_states=False, **kw)
    assert (p["n_blocks"], p["max_tlen"], p["max_tlen_lds"], p["lds_bytes"]) == (2, 9, 9, _lds(9, 2))
    assert p["output_bytes"] == _outputs(7, 41, 300, False)
    # a variant beyond the 10000 entries kept in LDS is read from global memory: the region does not grow with it
    wide = dict(L=40000, K=2, periodic=False, n_systems=3, n_cap=500, n_obs=5)
    alone = gil.plan_many_large(sigma_grid=4000.0, **wide)
    assert alone["table_in_lds"] == 0 and alone["table_len"] > 10000
    p = gil.plan_mixed_many(sigma_grids=[4000.0, 5.0, 0.0], **wide)
    assert (p["max_tlen"], p["max_tlen_lds"], p["n_global"]) == (alone["table_len"], 21, 1)
    assert p["lds_bytes"] == _lds(21, 2) and p["table_doubles"] == alone["table_len"] + 1 + 22 + 1
    assert p["work_bytes_per_system"] == _work(40000, 2, 500) == alone["work_bytes_per_system"]
    p = gil.plan_mixed_many(sigma_grids=[4000.0], **wide)                 # no variant in LDS: no region at all
    assert (p["max_tlen_lds"], p["n_global"], p["lds_bytes"]) == (-1, 1, _lds(-1, 2)) and p["lds_bytes"] == alone["lds_bytes"]
    # the longest table that still lies in LDS has 9999 taps (10000 entries with the closing zero)
    edge = gil.plan_many_large(sigma_grid=1.0e7, **dict(wide, L=9998))    # wider than the box: L + 1 taps
    assert (edge["table_len"], edge["table_in_lds"]) == (9999, 1)
    p = gil.plan_mixed_many(sigma_grids=[1.0e7, 0.0], **dict(wide, L=9998))
    assert (p["max_tlen_lds"], p["n_global"], p["lds_bytes"]) == (9999, 0, edge["lds_bytes"])
    over = gil.plan_many_large(sigma_grid=1.0e7, **dict(wide, L=9999))
    assert (over["table_len"], over["table_in_lds"]) == (10000, 0)
    p = gil.plan_mixed_many(sigma_grids=[1.0e7, 0.0], **dict(wide, L=9999))
    assert (p["max_tlen"], p["max_tlen_lds"], p["n_global"], p["lds_bytes"]) == (10000, 0, 1, _lds(0, 2))
    # sigma = 0 alone: the global mean field, a table of the closing zero only
    p = gil.plan_mixed_many(sigma_grids=[0.0], **wide)
    assert (p["max_tlen"], p["max_tlen_lds"], p["n_global"], p["table_doubles"], p["lds_bytes"]) == (0, 0, 0, 1, _lds(0, 2))
    # any L >= 2 is accepted, as gilm_run accepts it
    p = gil.plan_mixed_many(L=2, K=1, periodic=True, n_systems=1, n_cap=1, n_obs=1, sigma_grids=[0.0, 1.0])
    assert p["n_blocks"] == 1 and p["work_bytes_per_system"] == _work(2, 1, 1)
    # the largest launch there is stays below the 160 KB (module docstring)
    p = gil.plan_mixed_many(L=9998, K=1, periodic=False, n_systems=1, n_obs=1, n_cap=2 ** 20, sigma_grids=[1.0e7])
    assert (p["n_blocks"], p["max_tlen_lds"], p["lds_bytes"]) == (4096, 9999, 146048) and p["lds_bytes"] <= LDS_LIMIT


@pytest.mark.parametrize("sigma_grid,periodic", [(5.0, False), (0.0, False), (0.012, True), (300.0, True), (4000.0, False)])
def test_one_variant_is_the_plan_of_gilm_run(gil, sigma_grid, periodic):
    kw = dict(L=30000, K=2, periodic=periodic, n_systems=4, n_cap=5000, n_obs=3)
    m = gil.plan_many_large(sigma_grid=sigma_grid, **kw)
    x = gil.plan_mixed_many(sigma_grids=[sigma_grid], **kw)
    assert (x["lds_bytes"], x["work_bytes_per_system"], x["n_blocks"], x["max_tlen"], x["n_systems"], x["output_bytes"]) == \
           (m["lds_bytes"], m["work_bytes_per_system"], m["n_blocks"], m["table_len"], m["n_systems"], m["output_bytes"])
    assert x["n_global"] == 1 - m["table_in_lds"] and x["max_tlen_lds"] == (m["table_len"] if m["table_in_lds"] else -1)
    assert x["table_doubles"] == m["table_len"] + 1


def test_plan_refusals_name_the_value(capi, gil):
    kw = dict(L=5000, K=1, periodic=False, n_systems=3, n_cap=90, n_obs=11)
    nan, inf = float("nan"), float("inf")
    work = 65535 * _work(2 ** 25, 1, 1)
    for bad, text in (
            (dict(sigma_grids=[1.0], L=1), "gilxm_plan: L = 1 is outside [2, 2^25 = 33554432]"),
            (dict(sigma_grids=[1.0], L=2 ** 25 + 1), "gilxm_plan: L = 33554433 is outside [2, 2^25 = 33554432]"),
            (dict(sigma_grids=[1.0], K=0), "gilxm_plan: site capacity K = 0 is outside [1, 32]"),
            (dict(sigma_grids=[1.0], K=33), "gilxm_plan: site capacity K = 33 is outside [1, 32]"),
            (dict(sigma_grids=[1.0], L=2 ** 25, K=8), "gilxm_plan: L * K = 268435456 exceeds 2^27 = 134217728 (site map)"),
            (dict(sigma_grids=[1.0], n_systems=0), "gilxm_plan: n_systems = 0 is outside [1, GILM_MAX_SYSTEMS = 65535]"),
            (dict(sigma_grids=[1.0], n_systems=65536), "gilxm_plan: n_systems = 65536 is outside [1, GILM_MAX_SYSTEMS = 65535]"),
            (dict(sigma_grids=[1.0], n_cap=0), "gilxm_plan: n_cap = 0 is outside [1, 2^20 = 1048576]"),
            (dict(sigma_grids=[1.0], n_cap=2 ** 20 + 1), "gilxm_plan: n_cap = 1048577 is outside [1, 2^20 = 1048576]"),
            (dict(sigma_grids=[1.0], n_obs=0), "gilxm_plan: n_obs = 0 must be at least 1"),
            (dict(sigma_grids=[]), "gilxm_plan: n_variants = 0 is outside [1, 4096]"),
            (dict(sigma_grids=[1.0] * 4097), "gilxm_plan: n_variants = 4097 is outside [1, 4096]"),
            (dict(sigma_grids=[1.0, 2.0], variant_of_system=[0, 2, 1]), "gilxm_plan: variant index 2 of system 1 is outside [0, n_variants = 2)"),
            (dict(sigma_grids=[1.0, 2.0], variant_of_system=[-1, 0, 1]), "gilxm_plan: variant index -1 of system 0 is outside [0, n_variants = 2)"),
            (dict(sigma_grids=[1.0, -0.5]), "gilxm_plan: sigma_grid = -0.500000 of variant 1 must be finite and not negative"),
            (dict(sigma_grids=[nan]), "gilxm_plan: sigma_grid = nan of variant 0 must be finite and not negative"),
            (dict(sigma_grids=[0.0, 1.0, inf]), "gilxm_plan: sigma_grid = inf of variant 2 must be finite and not negative"),
            (dict(sigma_grids=[1.0], order=[0, 1, 3]), "gilxm_plan: order is not a permutation: order[2] = 3 is outside [0, n_systems = 3)"),
            (dict(sigma_grids=[1.0], order=[2, 0, 2]), "gilxm_plan: order is not a permutation: system 2 appears twice (second time at 2)"),
            (dict(sigma_grids=[1.0], L=2 ** 25, n_systems=65535, n_cap=1, n_obs=1),
             f"gilxm_plan: the batch needs {work} bytes of work memory and {_outputs(65535, 1, 1, True)} bytes of outputs, "
             f"more than the {PLAN_MAX} bytes a plan accepts")):
        with pytest.raises(capi.ApsError) as exc:
            gil.plan_mixed_many(**dict(kw, **bad))
        assert exc.value.code == ERR_ARG and str(exc.value).endswith(text), (bad, str(exc.value))
    assert work + _outputs(65535, 1, 1, True) > PLAN_MAX
    assert gil.plan_mixed_many(sigma_grids=[1.0] * 4096, order=[2, 0, 1], **kw)["table_doubles"] == 4096 * 6
    with pytest.raises(ValueError):
        gil.plan_mixed_many(sigma_grids=[1.0], variant_of_system=[0, 0], **kw)      # one index per system
    # the batch shape's plan keeps refusing the large shape, with its own text
    with pytest.raises(capi.ApsError) as exc:
        gil.plan_mixed(sigma_grids=[1.0], **kw)
    assert str(exc.value).endswith("gilx_plan: L = 5000 is beyond GIL_MAX_L = 4096: the large-system shape takes no mixed batches")


def test_run_refusals_come_before_any_device(capi, gil):
    lib = gil._lib()
    keep = [np.array([0.5, 0.5]), np.array([0.0, 0.01]), np.array([1, 1], np.int32), np.array([0, 3], np.int32), np.array([1, -1], np.int8)]
    par = gil.GilParams(L=5000, K=1, periodic=1, n_systems=2, n_cap=1, n_obs=2, ref_obs=-1, rate_diffusion=0.1, rate_active=1.0, T=0.01,
                        max_events=16, beta=keep[0].ctypes.data, times_obs=keep[1].ctypes.data)
    ms = C.c_double()

    def call(sigma=(0.0, 2.0), vos=(0, 1), order=None, p=par, n0=keep[2], pos0=keep[3]):
        desc, alive = gil._mixed_descriptor(2, 1, list(sigma), None if vos is None else list(vos), order=order)
        rc = lib.gilxm_run(C.byref(p), C.byref(desc), gil._p(n0), gil._p(pos0), gil._p(keep[4]), *[None] * 11, C.byref(ms))
        return rc, lib.gilxm_last_error().decode()

    assert call(vos=None) == (ERR_ARG, "gilxm_run: null argument")       # every system needs its variant
    assert call(vos=(0, 2)) == (ERR_ARG, "gilxm_run: variant index 2 of system 1 is outside [0, n_variants = 2)")
    assert call(sigma=(0.0, -1.0)) == (ERR_ARG, "gilxm_run: sigma_grid = -1.000000 of variant 1 must be finite and not negative")
    assert call(sigma=()) == (ERR_ARG, "gilxm_run: n_variants = 0 is outside [1, 4096]")
    assert call(order=[1, 1]) == (ERR_ARG, "gilxm_run: order is not a permutation: system 1 appears twice (second time at 1)")
    assert call(n0=np.array([1, 2], np.int32)) == (ERR_ARG, "gilxm_run: n0 = 2 of system 1 is outside [0, n_cap = 1]")
    assert call(pos0=np.array([0, 5000], np.int32)) == (ERR_ARG, "gilxm_run: position outside [0, L)")
    neg = gil.GilParams.from_buffer_copy(par)
    neg.max_events = -1
    assert call(p=neg) == (ERR_ARG, "gilxm_run: max_events = -1 must not be negative")
    huge = gil.GilParams.from_buffer_copy(par)
    huge.L = 2 ** 25 + 1                                                 # the numbers are checked before any array is read
    assert call(p=huge) == (ERR_ARG, "gilxm_run: L = 33554433 is outside [2, 2^25 = 33554432]")
    rc, text = call(order=[1, 0])                                        # acceptable: only the device is missing, or it runs
    assert (rc, text) == (ERR_NODEVICE, "gilxm_run: no HIP device") or rc == 0
    if capi.device_count() == 0:                                         # a good call of the Python entry point fails loudly too
        common = dict(L=5000, K=1, periodic=True, rate_diffusion=0.1, rate_active=1.0, betas=[0.5, 0.5],
                      states=[(np.array([0]), np.array([1])), (np.array([3]), np.array([-1]))], times_obs=[0.0, 0.01], T=0.01, max_events=16)
        with pytest.raises(capi.ApsError) as exc:
            gil.run_mixed_many_raw(sigma_grids=[2.0, 0.0], variant_of_system=[1, 0], seeds=[2 ** 64 - 1, 7], **common)
        assert exc.value.code == ERR_NODEVICE and "gilxm_run: no HIP device" in str(exc.value)


def test_large_keys_are_the_groups_key_plus_the_place(gil, psys):
    kw = dict(L=60, xlim=1.0, site_capacity=1, N=20, init="fixed", scale_rates=False, rate_diffusion=0.5, rate_active=4.0, beta=1.0)
    mk = lambda seed, rs: psys.ParticleSystem(seed=seed, rng=np.random.default_rng(rs), **kw)
    systems = [mk(11, 0), mk(12, 1), mk(13, 2), mk(14, 3), mk(15, 4)]
    assert gil.mixed_keys(systems, [0, 1, 0, 1, 1], large=True) == ([11, 12, 12, 13, 14], [0] * 5)
    assert gil.mixed_keys(systems, large=True) == ([11, 12, 13, 14, 15], [0] * 5)
    assert gil.mixed_keys(systems, [5, 5, 2, 2, 5], large=True) == ([11, 12, 13, 14, 13], [0] * 5)
    assert gil.mixed_keys(systems, [0, 1, 0, 1, 1]) == ([11, 12, 11, 12, 12], [0, 0, 1, 1, 2])      # the batch shape's: unchanged
    # the sum is taken mod 2^64, as gilm_run takes seed + s
    top = 2 ** 64 - 1
    systems = [mk(top - 1, 0), mk(0, 1), mk(0, 2), mk(0, 3), mk(top, 4), mk(0, 5)]
    assert gil.mixed_keys(systems, [0, 0, 0, 0, 1, 1], large=True) == ([top - 1, top, 0, 1, top, 0], [0] * 6)
    # no seed: the group's key is drawn from its first system's rng, after the initial state, as run_batched_exact draws it
    systems, twin = [mk(None, 7), mk(None, 8), mk(None, 9)], [mk(None, 7), mk(None, 8), mk(None, 9)]
    for ps in systems + twin:
        ps.init_particles()
    want = [int(twin[0].rng.random() * 2.0 ** 53), int(twin[1].rng.random() * 2.0 ** 53)]
    assert gil.mixed_keys(systems, [0, 1, 0], large=True) == ([want[0], want[1], want[0] + 1], [0, 0, 0])
    with pytest.raises(ValueError):
        gil.mixed_keys(systems, [0, 1], large=True)


def test_without_allow_large_the_large_shape_is_refused_as_before(capi, gil, ens, psys):
    kw = dict(xlim=1.0, site_capacity=1, init="fixed", scale_rates=False, rate_diffusion=0.5, rate_active=4.0, seed=3)
    big_l = [psys.ParticleSystem(L=5000, N=30, beta=1.0, local_kernel_sigma=s, rng=np.random.default_rng(i), **kw) for i, s in enumerate((0.02, 0.0))]
    big_n = [psys.ParticleSystem(L=3000, N=n, beta=1.0, local_kernel_sigma=0.02, rng=np.random.default_rng(i), **dict(kw, site_capacity=2))
             for i, n in enumerate((30, 2100))]
    text_l = r"L = 5000, N = 30 is a large shape \(beyond L = 4096, N = 2048\); the large-system kernel takes no mixed batches"
    text_n = r"L = 3000, N = 2100 is a large shape \(beyond L = 4096, N = 2048\); the large-system kernel takes no mixed batches"
    for fn in (gil.run_batched_exact_mixed, gil.run_batched_exact_statistics_mixed):
        for more in ({}, dict(allow_large=False)):
            with pytest.raises(ValueError, match=fn.__name__ + ": " + text_l):
                fn(big_l, T=0.1, obs_dt=0.05, **more)
            with pytest.raises(ValueError, match=fn.__name__ + ": " + text_n):
                fn(big_n, T=0.1, obs_dt=0.05, **more)
        with pytest.raises(ValueError, match="cannot resume from a checkpoint"):       # resume stays refused
            fn(big_l, T=0.1, obs_dt=0.05, resume=object(), allow_large=True)
    with pytest.raises(ValueError, match="run_batched_exact_structure_mixed: " + text_l):  # structure sums: out of scope, still refused
        gil.run_batched_exact_structure_mixed(big_l, T=0.1, obs_dt=0.05)
    ps = dict(L=100, xlim=1.0, site_capacity=1, scale_rates=False, rate_diffusion=0.5, rate_active=4.0, seed=3)
    run, seeds = dict(T=1.0, obs_dt=0.1), [[1, 2]]
    with pytest.raises(ValueError, match=r"sweep_over_sigmas: one_launch=True needs the exact dynamics"):
        ens.sweep_over_sigmas([0.02, 0.0], [1.0], 2, ps, dict(N=30, init="fixed"), run, seeds, on_device=True, dynamics="sync", one_launch=True,
                              allow_large=True)
    with pytest.raises(ValueError, match=r"L = 5000, N = 30 is a large shape \(beyond L = 4096, N = 2048\)"):
        ens.sweep_over_sigmas([0.02, 0.0], [1.0], 2, dict(ps, L=5000), dict(N=30, init="fixed"), run, seeds, on_device=True, one_launch=True)
    with pytest.raises(ValueError, match=r"N = 2100 is a large shape \(beyond L = 4096, N = 2048\)"):
        ens.sweep_over_densities([30, 2100], [1.0], 2, dict(ps, L=3000, site_capacity=2), dict(init="fixed"), run, seeds, on_device=False, one_launch=True)
    if capi.device_count() == 0:
        # with allow_large the same calls get as far as the library, which misses only the device: plan, variants and keys went through
        with pytest.raises(capi.ApsError, match="gilxm_run: no HIP device"):
            gil.run_batched_exact_statistics_mixed(big_l, T=0.1, obs_dt=0.05, allow_large=True)
        with pytest.raises(capi.ApsError, match="gilxm_run: no HIP device"):
            ens.sweep_over_densities([30, 2100], [1.0], 2, dict(ps, L=3000, site_capacity=2), dict(init="fixed"), run, seeds, on_device=False,
                                     one_launch=True, allow_large=True)
        small = [psys.ParticleSystem(L=100, N=30, beta=1.0, local_kernel_sigma=s, rng=np.random.default_rng(i), **kw) for i, s in enumerate((0.02, 0.0))]
        with pytest.raises(capi.ApsError, match="gilx_run: no HIP device"):              # no large shape: the batch kernel's launch as before
            gil.run_batched_exact_mixed(small, T=0.1, obs_dt=0.05, allow_large=True)
