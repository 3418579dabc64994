"""GPU suite (-m gpu): the wide shape of the hydrodynamic-limit solver (include/pde_wide.h, `IMEXPDE(workgroups=...)`):
one system cut into slabs on many workgroups, a time step a chain of kernel launches.

Checked against oracle/pde_numpy.py with the same random numbers, at the tolerances tests/test_gpu_pde.py holds for
the one-workgroup kernel (binary64; Thomas/scan solver instead of SuperLU, direct convolution instead of rfft products,
other summation orders, the device's exp):
    densities, m_series, var_series, snapshots ........ 1e-11 relative to the field's scale
    fft modes ......................................... 1e-12 absolute
    tracer spin states ................................ equal
    tracer positions, v_eff / D_eff series ............ 1e-9
and against the one-workgroup kernel itself where no fixed bar against the oracle can be set (L = 131 072).
The yardstick is the binary64 oracle at one point of the parameter space; tests/test_gpu_pde_random.py holds the same bars on 1,
2 and 7 slabs over random parameters against the extended-precision reference of tests/pde_reference.py."""
import importlib
import time

import numpy as np
import pytest

from oracle.pde_numpy import PdeOracle

pytestmark = pytest.mark.gpu
PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"


@pytest.fixture(scope="module")
def pde():
    mod = importlib.import_module(PKG + ".pde")
    assert importlib.import_module(PKG + ".capi").device_count() >= 1
    return mod


def close(a, b, tol, what):
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    if np.all(np.isnan(b)):                      # a run shorter than the tracers' window: the series is NaN throughout, as the reference leaves it
        return
    scale = max(np.nanmax(np.abs(b)), 1e-300)
    err = np.nanmax(np.abs(np.asarray(a) - np.asarray(b))) / scale
    print(what, f"{err:.3e}")
    assert err <= tol, (what, err)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what


def deviation(a, b):
    return float(np.nanmax(np.abs(np.asarray(a) - np.asarray(b))) / max(np.nanmax(np.abs(b)), 1e-300))


CASES = {c["tag"]: c for c in [
    dict(tag="periodic_bidirectional_local", bc="periodic", active_model="bidirectional", gaussian_kernel=False, init="poisson"),
    dict(tag="neumann_anchored_kernel", bc="neumann", active_model="anchored_minus", gaussian_kernel=True, init="poisson"),
    dict(tag="periodic_anchored_kernel", bc="periodic", active_model="anchored_minus", gaussian_kernel=True, init="homogeneous"),
    dict(tag="neumann_bidirectional_local", bc="neumann", active_model="bidirectional", gaussian_kernel=False, init="homogeneous"),
    dict(tag="periodic_bidirectional_wide_kernel", bc="periodic", active_model="bidirectional", gaussian_kernel=True,
         init="homogeneous", kernel_sigma=1e5 - 10),
    dict(tag="neumann_bidirectional_global", bc="neumann", active_model="bidirectional", gaussian_kernel=True,
         init="poisson", kernel_sigma=2e5),
]}

_oracle_cache = {}


def oracle_run(case, n_tracers, seed, **kw):
    """The oracle's run of a case with its random numbers recorded; one run serves every `workgroups` of that case."""
    key = (case["tag"], n_tracers, seed, tuple(sorted(kw.items())))
    if key not in _oracle_cache:
        args = dict(bc=case["bc"], active_model=case["active_model"], gaussian_kernel=case["gaussian_kernel"], seed=seed, **kw)
        orc = PdeOracle(**args)
        orc.initialize(mode=case["init"], rho0=1.0, noise=0.2, n_tracers=n_tracers)
        init = dict(rho_p=orc.rho_p.copy(), tracers=orc.tracers.copy())
        orc.solve(record_randoms=True)
        _oracle_cache[key] = (args, orc, init)
    return _oracle_cache[key]


def gpu_run(pde, case, args, orc, init, n_tracers, **ext):
    gpu = pde.IMEXPDE(**args, **ext)
    gpu.initialize(mode=case["init"], rho0=1.0, noise=0.2, n_tracers=n_tracers)
    assert np.array_equal(gpu.rho_p, init["rho_p"]) and np.array_equal(gpu.tracers, init["tracers"])   # same host-side initial condition
    gpu.solve(rand_u=np.array(orc.rand_u), rand_n=np.array(orc.rand_n))
    return gpu


def hold_the_bars(gpu, orc, tag, n_modes=None):
    want, got = orc.get_output(), gpu.get_output()
    assert list(got.keys()) == list(want.keys())
    for k in ("rho_p", "rho_m", "m_series", "var_series", "snapshots", "m_snapshots"):
        close(got[k], want[k], 1e-11, (tag, k))
    assert np.array_equal(got["times"], want["times"])
    if n_modes is None:
        n_modes = want["fft_phase"].shape[1]
    assert got["fft_phase"].shape == (want["fft_phase"].shape[0], n_modes) == got["fft_amp"].shape
    assert np.max(np.abs(got["fft_phase"] - want["fft_phase"][:, :n_modes])) <= 1e-12
    assert np.max(np.abs(got["fft_amp"] - want["fft_amp"][:, :n_modes])) <= 1e-12
    assert np.array_equal(gpu.tracer_state, orc.tracer_state)
    close(gpu.tracers_unwrapped, orc.tracers_unwrapped, 1e-9, (tag, "tracers"))
    close(got["v_eff_series"], want["v_eff_series"], 1e-9, (tag, "v_eff"))
    close(got["D_eff_series"], want["D_eff_series"], 1e-9, (tag, "D_eff"))


@pytest.mark.parametrize("workgroups", [1, 2, 7])
@pytest.mark.parametrize("tag", list(CASES))
def test_wide_small_grids_match_oracle(pde, tag, workgroups):
    """L = 333, the six cases of tests/test_gpu_pde.py, on 1, 2 and 7 slabs (7 does not divide 333: slabs of 48 and 47)."""
    case = CASES[tag]
    args, orc, init = oracle_run(case, 257, 321, L=333, xlim=1.0, T=0.2, dt=5e-4, gamma=2.33e-4, lam=0.6, beta=2.0,
                                 kernel_sigma=case.get("kernel_sigma", 0.02), snapshot_interval=100)
    gpu = gpu_run(pde, case, args, orc, init, 257, workgroups=workgroups)
    hold_the_bars(gpu, orc, (tag, workgroups))


@pytest.mark.parametrize("workgroups", [3, 16])
@pytest.mark.parametrize("tag", ["neumann_anchored_kernel", "periodic_bidirectional_local"])
def test_wide_beyond_lds_cases_match_oracle(pde, tag, workgroups):
    """L = 6000, the two beyond-LDS cases of tests/test_gpu_pde.py, on 3 and 16 slabs."""
    case = CASES[tag]
    args, orc, init = oracle_run(case, 100, 99, L=6000, xlim=1.0, T=0.03, dt=5e-4, gamma=2.33e-4, lam=0.6, beta=2.0,
                                 kernel_sigma=0.004, snapshot_interval=20)
    gpu = gpu_run(pde, case, args, orc, init, 100, workgroups=workgroups)
    hold_the_bars(gpu, orc, (tag, workgroups))


LARGE = [("neumann_anchored_kernel", 32768), ("periodic_bidirectional_local", 16384)]


@pytest.mark.parametrize("tag,L", LARGE)
def test_wide_large_grids_match_oracle_and_repeat_bit_for_bit(pde, tag, L):
    """Grids the one-workgroup shape cannot serve well: 60 steps, workgroups="auto", the 8 lowest Fourier modes; the same
    bars.  (The oracle against a banded-LU restatement of the same scheme deviates by at most 2e-14 / 2.5e-13 here, so
    1e-11 leaves a factor 40 or more for the GPU's own summation orders.)  The same call made twice gives the same bits
    in every output."""
    case = CASES[tag]
    args, orc, init = oracle_run(case, 100, 99, L=L, xlim=1.0, T=0.03, dt=5e-4, gamma=2.33e-4, lam=0.6, beta=2.0,
                                 kernel_sigma=0.004, snapshot_interval=20)
    gpu = gpu_run(pde, case, args, orc, init, 100, workgroups="auto", fft_modes=8)
    assert gpu.plan()["workgroups"] >= 2
    hold_the_bars(gpu, orc, (tag, L), n_modes=8)
    again = gpu_run(pde, case, args, orc, init, 100, workgroups="auto", fft_modes=8)
    a, b = gpu.get_output(), again.get_output()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert np.array_equal(gpu.tracers_unwrapped, again.tracers_unwrapped) and np.array_equal(gpu.tracer_state, again.tracer_state)


def test_wide_against_the_one_workgroup_kernel_at_131072(pde):
    """L = 131 072, neumann_anchored_kernel, 20 steps, no tracers, no Fourier modes.  At this size (gamma dt / dx^2 = 2000)
    two CPU direct solvers already differ by 1e-11 .. 1.4e-11, so the yardstick is the one-workgroup kernel, same
    factorisation and taps: d_new <= max(1e-11, 2 d_old), both deviations taken against the oracle, a factor 2 because the
    two shapes differ in rounding order (grouping, fma), not in method.  And the direction of the speed change: the wide
    shape takes at most a quarter of the one-workgroup kernel's time (a floor; one CU against up to 256)."""
    case = CASES["neumann_anchored_kernel"]
    L, nsteps = 131072, 20
    kw = dict(L=L, xlim=1.0, T=(nsteps + 0.5) * 5e-4, dt=5e-4, gamma=2.33e-4, lam=0.6, beta=2.0, kernel_sigma=0.004,
              snapshot_interval=10, bc=case["bc"], active_model=case["active_model"], gaussian_kernel=True, seed=99)
    t0 = time.perf_counter()
    orc = PdeOracle(**kw)
    assert orc.nsteps == nsteps
    orc.initialize(mode=case["init"], rho0=1.0, noise=0.2, n_tracers=0)
    rho_p0 = orc.rho_p.copy()
    orc.solve()
    t_orc = time.perf_counter() - t0
    runs = {}
    for wg in (None, "auto"):
        s = pde.IMEXPDE(record_fft=False, workgroups=wg, **kw)
        s.initialize(mode=case["init"], rho0=1.0, noise=0.2, n_tracers=0)
        assert np.array_equal(s.rho_p, rho_p0)                   # same host-side initial condition
        s.solve()
        runs[wg] = s
    want = orc.get_output()
    keys = ("rho_p", "rho_m", "m_series", "var_series", "snapshots", "m_snapshots")
    d_old = max(deviation(runs[None].get_output()[k], want[k]) for k in keys)
    d_new = max(deviation(runs["auto"].get_output()[k], want[k]) for k in keys)
    d_pair = max(deviation(runs["auto"].get_output()[k], runs[None].get_output()[k]) for k in keys)
    ms_old, ms_new = runs[None].kernel_ms, runs["auto"].kernel_ms
    print(f"L={L} steps={nsteps}: d_old={d_old:.3e} d_new={d_new:.3e} wide-vs-old={d_pair:.3e}; kernel_ms old={ms_old:.2f} "
          f"wide={ms_new:.3f} ratio={ms_old / ms_new:.1f}; plan={runs['auto'].plan()}; oracle {t_orc:.1f} s")
    assert d_new <= max(1e-11, 2 * d_old), (d_new, d_old)
    assert ms_new <= 0.25 * ms_old, (ms_new, ms_old)


def test_wide_batch_equals_single_solves_bit_for_bit(pde):
    """Three beta values through solve_batch(workgroups=8) at L = 4096: the partition and every order of summation are
    those of a single solve, whatever the system index."""
    kw = dict(L=4096, xlim=1.0, T=0.05, dt=5e-4, gamma=2.33e-4, lam=0.6, bc="periodic", active_model="bidirectional",
              gaussian_kernel=True, kernel_sigma=0.01, snapshot_interval=50, seed=5)
    betas = [0.5, 1.5, 2.5]
    base = pde.IMEXPDE(beta=betas[0], record_fft=False, **kw)
    base.initialize(mode="poisson", rho0=1.0, noise=0.2, n_tracers=64)
    rho_p0, rho_m0 = base.rho_p.copy(), base.rho_m.copy()
    batch = base.solve_batch(betas, workgroups=8)
    assert base.workgroups is None
    for s, beta in enumerate(betas):
        one = pde.IMEXPDE(beta=beta, record_fft=False, workgroups=8, **kw)
        one.initialize(mode="poisson", rho0=1.0, noise=0.2, n_tracers=64)
        one.rho_p, one.rho_m = rho_p0, rho_m0
        one.solve()
        for k, v in (("rho_p", one.rho_p), ("rho_m", one.rho_m), ("m_series", one.m_series)):
            assert np.array_equal(batch[k][s], v), (beta, k)
    assert not np.array_equal(batch["rho_p"][0], batch["rho_p"][2])


def test_wide_device_noise_draws_the_same_tracer_stream(pde):
    """Device Philox noise: the counter layout (n, i, sys, 0x7AC3), key = seed is shared by both shapes, so with the same
    seed the tracers flip at the same steps and move alike."""
    kw = dict(L=4096, xlim=1.0, T=0.0252, dt=5e-4, gamma=2.33e-4, lam=0.6, beta=2.0, bc="periodic", active_model="bidirectional",
              gaussian_kernel=False, snapshot_interval=50, seed=77, record_fft=False)
    out = {}
    for wg in (None, 8):
        s = pde.IMEXPDE(workgroups=wg, **kw)
        assert s.nsteps == 50
        s.initialize(mode="poisson", rho0=1.0, noise=0.2, n_tracers=2000)
        s.solve()
        out[wg] = s
    assert np.array_equal(out[8].tracer_state, out[None].tracer_state)
    close(out[8].tracers_unwrapped, out[None].tracers_unwrapped, 1e-9, "device-noise tracers")
    close(out[8].rho_p, out[None].rho_p, 1e-11, "device-noise rho_p")


def test_wide_plan_and_error_paths(pde):
    capi = importlib.import_module(PKG + ".capi")
    p = pde.plan(L=32768, workgroups="auto", gaussian_kernel=True, kernel_sigma=0.004)
    assert p["workgroups"] >= 2 and sum(p["slab_lengths"]) == 32768
    assert pde.plan(L=32768, workgroups=1)["workgroups"] == 1
    s = pde.IMEXPDE(L=64, T=0.01, workgroups=17, record_fft=False)          # floor(64 / 17) < 4 sites per slab
    s.initialize(n_tracers=8)
    with pytest.raises(capi.ApsError):
        s.solve()
    few = pde.IMEXPDE(L=64, T=0.01, workgroups=4, fft_modes=3, seed=3)
    few.initialize(n_tracers=8)
    few.solve()
    full = pde.IMEXPDE(L=64, T=0.01, workgroups=None, seed=3)
    full.initialize(n_tracers=8)
    full.solve()
    assert few.fft_amp.shape == (few.nsteps + 1, 3) and np.max(np.abs(few.fft_phase - full.fft_phase[:, :3])) <= 1e-12
    old_few = pde.IMEXPDE(L=64, T=0.01, fft_modes=3, seed=3)                # fft_modes on the one-workgroup shape too
    old_few.initialize(n_tracers=8)
    old_few.solve()
    assert np.array_equal(old_few.fft_phase, full.fft_phase[:, :3])
