"""GPU suite (-m gpu): the spectral convolution of the wide shape (`IMEXPDE(workgroups=..., convolution="spectral")`,
include/pde_spectral.h): the Gaussian-kernel magnetisation by complex binary64 transforms over overlap-save blocks.

Same oracle, same random numbers and the same bars as tests/test_gpu_pde_wide.py holds for the direct sum:
    densities, m_series, var_series, snapshots ........ 1e-11 relative to the field's scale
    fft modes ......................................... 1e-12 absolute
    tracer spin states ................................ equal
    tracer positions, v_eff / D_eff series ............ 1e-9
Blocks on small grids are forced with PDE_SPECTRAL_MAX_LOG2 (the cap of the transform's log2 length).
The yardstick is the binary64 oracle, itself a product of transforms; tests/test_gpu_pde_random.py measures both against the
extended-precision reference of tests/pde_reference.py over random parameters and says where no transform can hold the bar."""
import importlib
import os
import sys

import numpy as np
import pytest

from oracle.pde_numpy import PdeOracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_pde_wide import CASES, deviation, gpu_run, hold_the_bars, oracle_run      # noqa: E402  (helpers and the oracle cache are shared)

pytestmark = pytest.mark.gpu
PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"


@pytest.fixture(scope="module")
def pde():
    mod = importlib.import_module(PKG + ".pde")
    assert importlib.import_module(PKG + ".capi").device_count() >= 1
    return mod


def set_cap(monkeypatch, cap):
    if cap is None:
        monkeypatch.delenv("PDE_SPECTRAL_MAX_LOG2", raising=False)
    else:
        monkeypatch.setenv("PDE_SPECTRAL_MAX_LOG2", str(cap))


SMALL = [(tag, wg, cap) for tag in ("neumann_anchored_kernel", "periodic_anchored_kernel", "periodic_bidirectional_wide_kernel")
         for wg in (1, 7) for cap in ((None,) if tag == "periodic_bidirectional_wide_kernel" else (None, 8))]


@pytest.mark.parametrize("tag,workgroups,cap", SMALL)
def test_spectral_small_grids_match_oracle(pde, monkeypatch, tag, workgroups, cap):
    """L = 333: sigma = 0.02 (58 taps either side; one block of 2^9, or with cap 8 three blocks of 111 sites) and the odd
    ring-wide kernel (166 = floor(L / 2) taps, M = 2^10: the window wraps over itself)."""
    set_cap(monkeypatch, cap)
    case = CASES[tag]
    args, orc, init = oracle_run(case, 257, 321, L=333, xlim=1.0, T=0.2, dt=5e-4, gamma=2.33e-4, lam=0.6, beta=2.0,
                                 kernel_sigma=case.get("kernel_sigma", 0.02), snapshot_interval=100)
    gpu = gpu_run(pde, case, args, orc, init, 257, workgroups=workgroups, convolution="spectral")
    p = gpu.plan()
    kt = 166 if tag == "periodic_bidirectional_wide_kernel" else 58
    assert (p["ktaps"], p["conv_blocks"], p["conv_block_sites"], p["conv_log2"]) == ((kt, 3, 111, 8) if cap else (kt, 1, 333, 9 if kt == 58 else 10))
    hold_the_bars(gpu, orc, (tag, workgroups, cap))


def test_spectral_even_ring_wide_kernel_matches_oracle(pde, monkeypatch):
    """L = 334, sigma = 0.3: the kernel reaches the antipodal site (167 taps, the last one halved), M = 1024; 200 steps."""
    set_cap(monkeypatch, None)
    case = CASES["periodic_bidirectional_wide_kernel"]
    args, orc, init = oracle_run(case, 257, 321, L=334, xlim=1.0, T=0.10001, dt=5e-4, gamma=2.33e-4, lam=0.6, beta=2.0,
                                 kernel_sigma=0.3, snapshot_interval=100)
    assert orc.nsteps == 200
    gpu = gpu_run(pde, case, args, orc, init, 257, workgroups=2, convolution="spectral")
    p = gpu.plan()
    assert (p["ktaps"], p["conv_blocks"], p["conv_log2"]) == (167, 1, 10)
    hold_the_bars(gpu, orc, "L334 ring-wide")


@pytest.mark.parametrize("cap", [None, 10])
def test_spectral_beyond_lds_case_matches_oracle(pde, monkeypatch, cap):
    """L = 6000, sigma = 0.004 (212 taps), 16 slabs: one block of 2^13, or with cap 10 ten blocks of 600 sites."""
    set_cap(monkeypatch, cap)
    case = CASES["neumann_anchored_kernel"]
    args, orc, init = oracle_run(case, 100, 99, L=6000, xlim=1.0, T=0.03, dt=5e-4, gamma=2.33e-4, lam=0.6, beta=2.0,
                                 kernel_sigma=0.004, snapshot_interval=20)
    gpu = gpu_run(pde, case, args, orc, init, 100, workgroups=16, convolution="spectral")
    p = gpu.plan()
    assert (p["ktaps"], p["conv_blocks"], p["conv_block_sites"], p["conv_log2"]) == ((212, 10, 600, 10) if cap else (212, 1, 6000, 13))
    hold_the_bars(gpu, orc, ("L6000", cap))


@pytest.mark.parametrize("cap", [None, 13])
def test_spectral_large_grid_matches_oracle_and_repeats_bit_for_bit(pde, monkeypatch, cap):
    """L = 32 768, "auto", 60 steps, the 8 lowest Fourier modes: one block of 2^16 (five launches per convolution), or with
    cap 13 six blocks.  The same call made twice gives the same bits in every output."""
    set_cap(monkeypatch, cap)
    case = CASES["neumann_anchored_kernel"]
    args, orc, init = oracle_run(case, 100, 99, L=32768, xlim=1.0, T=0.03, dt=5e-4, gamma=2.33e-4, lam=0.6, beta=2.0,
                                 kernel_sigma=0.004, snapshot_interval=20)
    gpu = gpu_run(pde, case, args, orc, init, 100, workgroups="auto", fft_modes=8, convolution="spectral")
    p = gpu.plan()
    assert (p["conv_blocks"], p["conv_log2"]) == ((6, 13) if cap else (1, 16))
    hold_the_bars(gpu, orc, ("L32768", cap), n_modes=8)
    again = gpu_run(pde, case, args, orc, init, 100, workgroups="auto", fft_modes=8, convolution="spectral")
    a, b = gpu.get_output(), again.get_output()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert np.array_equal(gpu.tracers_unwrapped, again.tracers_unwrapped) and np.array_equal(gpu.tracer_state, again.tracer_state)


def test_spectral_batch_equals_single_solves_bit_for_bit(pde, monkeypatch):
    """Three beta values through solve_batch(workgroups=8, convolution="spectral") at L = 4096 with four blocks (cap 11): a
    system's bits do not depend on its index in the batch."""
    set_cap(monkeypatch, 11)
    kw = dict(L=4096, xlim=1.0, T=0.05, dt=5e-4, gamma=2.33e-4, lam=0.6, bc="periodic", active_model="bidirectional",
              gaussian_kernel=True, kernel_sigma=0.01, snapshot_interval=50, seed=5)
    betas = [0.5, 1.5, 2.5]
    base = pde.IMEXPDE(beta=betas[0], record_fft=False, **kw)
    base.initialize(mode="poisson", rho0=1.0, noise=0.2, n_tracers=64)
    rho_p0, rho_m0 = base.rho_p.copy(), base.rho_m.copy()
    batch = base.solve_batch(betas, workgroups=8, convolution="spectral")
    assert base.workgroups is None and base.convolution is None
    for s, beta in enumerate(betas):
        one = pde.IMEXPDE(beta=beta, record_fft=False, workgroups=8, convolution="spectral", **kw)
        p = one.plan()
        assert (p["conv_blocks"], p["conv_block_sites"], p["conv_log2"]) == (4, 1024, 11)
        one.initialize(mode="poisson", rho0=1.0, noise=0.2, n_tracers=64)
        one.rho_p, one.rho_m = rho_p0, rho_m0
        one.solve()
        for k, v in (("rho_p", one.rho_p), ("rho_m", one.rho_m), ("m_series", one.m_series)):
            assert np.array_equal(batch[k][s], v), (beta, k)
    assert not np.array_equal(batch["rho_p"][0], batch["rho_p"][2])
    direct = base.solve_batch(betas, workgroups=8)                  # another path, not another result: each holds 1e-11 against the oracle
    assert deviation(batch["rho_p"], direct["rho_p"]) <= 2e-11 and not np.array_equal(batch["rho_p"], direct["rho_p"])


@pytest.mark.parametrize("tag", ["periodic_bidirectional_local", "neumann_bidirectional_global"])
def test_spectral_changes_nothing_without_a_gaussian_kernel(pde, monkeypatch, tag):
    """gaussian_kernel=False and the global mean: no convolution runs, the outputs are those of convolution="direct", bit for bit."""
    set_cap(monkeypatch, None)
    case = CASES[tag]
    args, orc, init = oracle_run(case, 257, 321, L=333, xlim=1.0, T=0.2, dt=5e-4, gamma=2.33e-4, lam=0.6, beta=2.0,
                                 kernel_sigma=case.get("kernel_sigma", 0.02), snapshot_interval=100)
    runs = [gpu_run(pde, case, args, orc, init, 257, workgroups=7, convolution=c) for c in ("direct", "spectral")]
    assert runs[1].plan()["conv_log2"] == 0
    a, b = runs[0].get_output(), runs[1].get_output()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert np.array_equal(runs[0].tracers_unwrapped, runs[1].tracers_unwrapped) and np.array_equal(runs[0].tracer_state, runs[1].tracer_state)


def test_spectral_refuses_an_ineligible_shape(pde, monkeypatch):
    """L = 333 with the ring-wide kernel under cap 8: 2 kt = 332 is more than half of 256.  No fall-back to the direct sum."""
    set_cap(monkeypatch, 8)
    capi = importlib.import_module(PKG + ".capi")
    s = pde.IMEXPDE(L=333, T=0.01, workgroups=7, gaussian_kernel=True, kernel_sigma=1e5 - 10, convolution="spectral", seed=3)
    s.initialize(n_tracers=8)
    with pytest.raises(capi.ApsError) as e:
        s.solve()
    assert "pdew_solve" in str(e.value) and "eligible" in str(e.value)


def test_spectral_against_the_direct_sum_at_131072_ring_wide(pde, monkeypatch):
    """L = 131 072, sigma = 0.3: the kernel spans the ring (65 536 taps either side, M = 2^18 exactly), neumann_anchored_kernel,
    20 steps, no tracers, no Fourier modes.  As in tests/test_gpu_pde_wide.py at this size, two CPU direct solvers already differ
    by 1e-11, so the yardstick is the direct sum on the same shape: d_spectral <= max(1e-11, 2 d_direct), both against the oracle.
    And the direction of the speed change: the spectral path takes at most a quarter of the direct path's time (a floor: per site
    2 * 131 073 multiply-adds against about 360 operations of the transforms)."""
    set_cap(monkeypatch, None)
    case = CASES["neumann_anchored_kernel"]
    L, nsteps = 131072, 20
    kw = dict(L=L, xlim=1.0, T=(nsteps + 0.5) * 5e-4, dt=5e-4, gamma=2.33e-4, lam=0.6, beta=2.0, kernel_sigma=0.3,
              snapshot_interval=10, bc=case["bc"], active_model=case["active_model"], gaussian_kernel=True, seed=99)
    orc = PdeOracle(**kw)
    assert orc.nsteps == nsteps
    orc.initialize(mode=case["init"], rho0=1.0, noise=0.2, n_tracers=0)
    rho_p0 = orc.rho_p.copy()
    orc.solve()
    runs = {}
    for conv in ("direct", "spectral"):
        s = pde.IMEXPDE(record_fft=False, workgroups="auto", convolution=conv, **kw)
        s.initialize(mode=case["init"], rho0=1.0, noise=0.2, n_tracers=0)
        assert np.array_equal(s.rho_p, rho_p0)                   # same host-side initial condition
        s.solve()
        runs[conv] = s
    p = runs["spectral"].plan()
    assert (p["ktaps"], p["conv_blocks"], p["conv_log2"]) == (65536, 1, 18)
    want = orc.get_output()
    keys = ("rho_p", "rho_m", "m_series", "var_series", "snapshots", "m_snapshots")
    d_direct = max(deviation(runs["direct"].get_output()[k], want[k]) for k in keys)
    d_spectral = max(deviation(runs["spectral"].get_output()[k], want[k]) for k in keys)
    d_pair = max(deviation(runs["spectral"].get_output()[k], runs["direct"].get_output()[k]) for k in keys)
    ms_direct, ms_spectral = runs["direct"].kernel_ms, runs["spectral"].kernel_ms
    print(f"L={L} steps={nsteps} ring-wide: d_direct={d_direct:.3e} d_spectral={d_spectral:.3e} spectral-vs-direct={d_pair:.3e}; "
          f"kernel_ms direct={ms_direct:.3f} spectral={ms_spectral:.3f} ratio={ms_direct / ms_spectral:.1f}; plan={ {k: v for k, v in p.items() if k != 'slab_lengths'} }")
    assert d_spectral <= max(1e-11, 2 * d_direct), (d_spectral, d_direct)
    assert ms_spectral <= 0.25 * ms_direct, (ms_spectral, ms_direct)
