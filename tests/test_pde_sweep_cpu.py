"""CPU suite: the kernel-width sweep of the hydrodynamic-limit solver (include/pde_sweep.h, `solve_sweep_raw`, `sweep_plan`,
`IMEXPDE.solve_sweep`, `sweep_over_kernel_sigmas`) as far as it can be checked without a GPU -- the header and its exports,
the plan rule (mode, reach and transform size per system), the refusals, and the loud failure without a device."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"


@pytest.fixture(scope="module")
def capi():
    mod = importlib.import_module(PKG + ".capi")
    if not os.path.exists(mod.LIB_PATH):
        importlib.import_module(PKG + ".build").build()
    return mod


@pytest.fixture(scope="module")
def pde(capi):
    return importlib.import_module(PKG + ".pde")


def header(capi):
    with open(os.path.join(os.path.dirname(capi.HEADER_PATH), "pde_sweep.h")) as fh:
        return fh.read()


def taps_rule(L, sigma, xlim=1.0):
    """kernel_taps() of csrc/pde_common.hpp: the reach in sites of the periodic Gaussian, cut at 1e-17 of the centre tap."""
    dx = xlim / L
    d = np.minimum(np.arange(L), L - np.arange(L)) * dx / sigma
    full = np.exp(-0.5 * d * d)
    return max(i for i in range(L // 2 + 1) if full[i] >= 1e-17 * full[0])


def test_sweep_header_symbols_exported_and_struct_mirrored(capi, pde):
    text = header(capi)
    names = sorted(set(re.findall(r"\b(pdek_[a-z_0-9]+)\s*\(", text)))
    assert names == ["pdek_last_error", "pdek_plan", "pdek_solve"]
    lib = C.CDLL(capi.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/pde_sweep.h but not exported"
    assert '#include "pde.h"' in text and "typedef struct pde_params" not in text      # pde_params is reused, not restated
    body = re.search(r"typedef struct pdek_plan_info \{(.*?)\} pdek_plan_info;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [d.split()[-1] for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in pde.PdekPlanInfo._fields_] == ["ktaps_max", "conv_log2_max", "lds_bytes", "fields_in_lds"]
    assert C.sizeof(pde.PdekPlanInfo) == 4 * 4
    assert int(re.search(r"#define PDEK_MIN_LOG2 (\d+)", text).group(1)) == pde.PDEK_MIN_LOG2 <= 8
    assert int(re.search(r"#define PDEK_MAX_LOG2 (\d+)", text).group(1)) == pde.PDEK_MAX_LOG2


def test_plan_of_the_reference_drivers_widths(pde):
    sig = [0.0005, 0.005, 0.05, 0.1, 1.0, 2e5]
    p = pde.sweep_plan(L=1000, gaussian_kernel=True, kernel_sigmas=sig, convolution="spectral")
    assert p["kernel_mode"] == [1, 1, 1, 1, 1, 2]
    assert p["ktaps"] == [4, 44, 442, 500, 500, 0]
    assert p["conv_log2"] == [10, 11, 11, 11, 11, 0]
    assert p["fields_in_lds"] is True and 0 < p["lds_bytes"] <= 160 * 1024
    assert p["ktaps_max"] == 500 and p["conv_log2_max"] == 11 and p["convolution"] == "spectral"
    for conv in (None, "direct"):
        d = pde.sweep_plan(L=1000, gaussian_kernel=True, kernel_sigmas=sig, convolution=conv)
        assert d["kernel_mode"] == p["kernel_mode"] and d["ktaps"] == p["ktaps"]
        assert d["conv_log2"] == [0] * 6 and d["conv_log2_max"] == 0 and d["convolution"] == "direct"
        assert d["fields_in_lds"] is True and 0 < d["lds_bytes"] < p["lds_bytes"]
    for conv in (None, "spectral"):
        loc = pde.sweep_plan(L=1000, gaussian_kernel=False, kernel_sigmas=sig, convolution=conv)
        assert loc["kernel_mode"] == [0] * 6 and loc["ktaps"] == [0] * 6 and loc["conv_log2"] == [0] * 6


#        L    sigma   kt
RULE = [(333, 0.0005, 1),
        (333, 0.02, 58),
        (333, 0.3, 166),
        (334, 0.3, 167),
        (256, 0.3, 128),
        (257, 0.3, 128),
        (12, 0.3, 6)]
LOG2 = {(333, 0.02): 9, (333, 0.3): 10, (334, 0.3): 10, (256, 0.3): 9, (257, 0.3): 10}


@pytest.mark.parametrize("L,sigma,kt", RULE)
def test_plan_rule_per_system(pde, L, sigma, kt):
    assert taps_rule(L, sigma) == kt
    p = pde.sweep_plan(L=L, gaussian_kernel=True, kernel_sigmas=[sigma], convolution="spectral")
    m = max(pde.PDEK_MIN_LOG2, math.ceil(math.log2(L + 2 * kt)))
    assert p["kernel_mode"] == [1] and p["ktaps"] == [kt] and p["conv_log2"] == [m]
    if (L, sigma) in LOG2:
        assert m == LOG2[(L, sigma)]
    if L == 12:
        assert m == max(pde.PDEK_MIN_LOG2, 5)
    assert 2 ** m >= L + 2 * kt
    d = pde.sweep_plan(L=L, gaussian_kernel=True, kernel_sigmas=[sigma])
    assert d["ktaps"] == [kt] and d["conv_log2"] == [0]


def test_plan_of_a_mixed_launch_is_sized_by_its_largest_system(pde):
    p = pde.sweep_plan(L=333, gaussian_kernel=True, kernel_sigmas=[0.0005, 0.02, 0.3, 1e5 - 10, 2e5], convolution="spectral")
    assert p["kernel_mode"] == [1, 1, 1, 1, 2] and p["ktaps"] == [1, 58, 166, 166, 0] and p["conv_log2"] == [9, 9, 10, 10, 0]
    assert p["ktaps_max"] == 166 and p["conv_log2_max"] == 10
    alone = pde.sweep_plan(L=333, gaussian_kernel=True, kernel_sigmas=[0.02], convolution="spectral")
    assert alone["conv_log2_max"] == 9 and alone["lds_bytes"] < p["lds_bytes"]


def test_refusals_come_with_a_text(capi, pde):
    with pytest.raises(capi.ApsError) as e:
        pde.sweep_plan(L=6000, gaussian_kernel=True, kernel_sigmas=[0.004], convolution="spectral")
    assert "pdek_plan" in str(e.value) and "eligible" in str(e.value)
    with pytest.raises(capi.ApsError) as e:
        pde.sweep_plan(L=6000, gaussian_kernel=True, kernel_sigmas=[0.004])             # fields in global memory: the wide shape's ground
    assert "eligible" in str(e.value)
    with pytest.raises(capi.ApsError) as e:
        pde.sweep_plan(L=1025, gaussian_kernel=True, kernel_sigmas=[1.0], convolution="spectral")   # 1025 + 2 * 512 > 2048
    assert "eligible" in str(e.value)
    assert pde.sweep_plan(L=1024, gaussian_kernel=True, kernel_sigmas=[1.0], convolution="spectral")["conv_log2"] == [11]
    for bad in (0.0, -0.02, float("nan"), float("inf")):
        with pytest.raises(capi.ApsError) as e:
            pde.sweep_plan(L=333, gaussian_kernel=True, kernel_sigmas=[0.02, bad])
        assert "kernel_sigma[1]" in str(e.value)
        assert pde.sweep_plan(L=333, gaussian_kernel=False, kernel_sigmas=[0.02, bad])["kernel_mode"] == [0, 0]   # no kernel asked for
    with pytest.raises(ValueError):
        pde.sweep_plan(L=333, gaussian_kernel=True, kernel_sigmas=[0.02], convolution="fft")


def _raw_kw(L=64, **over):
    rho = np.full(L, 0.5 / L)
    kw = dict(L=L, xlim=1.0, dt=5e-4, nsteps=4, gamma=2.33e-4, lam=0.6, bc="periodic", active_model="bidirectional",
              gaussian_kernel=True, snapshot_interval=2, rho_p0=rho, rho_m0=rho)
    kw.update(over)
    return kw


def test_axes_that_do_not_broadcast_are_refused(pde):
    with pytest.raises(ValueError):
        pde.solve_sweep_raw(betas=[1.0, 2.0, 3.0], kernel_sigmas=[0.02, 0.3], **_raw_kw())
    with pytest.raises(ValueError):
        pde.solve_sweep_raw(betas=[[1.0, 2.0]], kernel_sigmas=[0.02], **_raw_kw())
    s = pde.IMEXPDE(L=64, T=0.01, seed=1, gaussian_kernel=True)
    s.initialize(n_tracers=4)
    with pytest.raises(ValueError):
        s.solve_sweep(betas=[1.0, 2.0], kernel_sigmas=[0.02, 0.3, 1.0])
    with pytest.raises(ValueError):
        s.solve_sweep(convolution="fft")


def test_driver_call_refuses_a_width_given_twice(pde):
    """The result is keyed by the width: a second block of runs of the same width would replace the first."""
    for widths in ([0.02, 0.3, 0.02], [0.05, 0.05], []):
        with pytest.raises(ValueError):
            pde.sweep_over_kernel_sigmas(widths, n_runs=2, L=64, T=0.01, init_kwargs=dict(n_tracers=4))


def test_bad_widths_are_refused_by_the_solve_before_any_device_is_touched(capi, pde):
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(capi.ApsError) as e:
            pde.solve_sweep_raw(betas=[1.0, 2.0], kernel_sigmas=[0.02, bad], **_raw_kw())
        assert "pdek_solve" in str(e.value) and "kernel_sigma[1]" in str(e.value)
    with pytest.raises(capi.ApsError) as e:
        pde.solve_sweep_raw(betas=[1.0], kernel_sigmas=[1.0], convolution="spectral", **_raw_kw(L=1025))
    assert "eligible" in str(e.value)


def test_sweep_solve_fails_loudly_without_gpu(capi, pde):
    if capi.device_count() > 0:
        pytest.skip("GPU present")
    for conv in (None, "spectral"):
        with pytest.raises(capi.ApsError):
            pde.solve_sweep_raw(betas=[1.0, 2.0], kernel_sigmas=[0.02, 0.3], convolution=conv, **_raw_kw())
    s = pde.IMEXPDE(L=64, T=0.01, seed=1, gaussian_kernel=True)
    s.initialize(n_tracers=4)
    with pytest.raises(capi.ApsError):
        s.solve_sweep(kernel_sigmas=[0.02, 0.3], convolution="spectral")
    with pytest.raises(capi.ApsError):
        pde.sweep_over_kernel_sigmas([0.02, 0.3], n_runs=2, L=64, T=0.01, init_kwargs=dict(n_tracers=4))
