"""Parameter sets for the randomised parity of the hydrodynamic-limit solver against the extended-precision reference of
tests/pde_reference.py (tests/test_pde_cases_cpu.py checks the list itself on the CPU, tests/test_gpu_pde_random.py runs it
through every device path of the solver).  A helper module, not a test.

A draw fixes the model (grid, time step, rates, boundary condition, active model, magnetisation kernel, snapshot interval,
tracer and Fourier-mode counts) and holds two or three systems that differ in beta and in their initial state, so one launch
serves a draw.  `random_draws()` draws 44 from a fixed seed (every L of LS four times), `fixed_draws()` adds the two "poisson"
cases at sigma = 0.0005 that tests/test_gpu_pde_sweep.py leaves out.  THE LIST IS PART OF THIS FILE'S BEHAVIOUR: another seed,
range or order is another set of checks and is reviewed as such.

`runs(draw)` is, computed once per draw and shared (nobody writes into it): the binary64 oracle's run of every system with its
random numbers recorded, the extended-precision reference's run of the batch, and the yardsticks that follow from the two:
    d_oracle[k]   the oracle's deviation from the reference, per field and series, over the scale of the reference's array
                  (pde_reference.scale; "fft": absolute), per system and as the draw's maximum
    m_site        the largest per-site deviation of the oracle's magnetisation field from the reference's, over all steps
    margin        the smallest |u - rate dt| over all tracer flip draws (inf without tracers)
YARDSTICKS holds the committed values of the draws' maxima; tests/test_pde_cases_cpu.py asserts that they are what `runs`
gives, so a change of oracle, reference or generator shows there.  A draw is *tracer-comparable* when m_site <= 1e-10 and
margin >= 1e-9, and *oracle-grade* when 2 max d_oracle <= 1e-11: on the other draws (near-vacuum states, where the round-off of
the oracle's rfft products is divided by den + 1e-12) only a direct sum can be held to the reference.

PATHS names the device paths and `eligible(pde, draw, path)` asks the library's plans, which need no device, whether the
draw's shape runs there; INELIGIBLE is the committed table of the refusals."""
import functools
import os
import warnings

import numpy as np

import pde_reference as R
from oracle.pde_numpy import PdeOracle

RANDOM_SEED = 20261020
N_RANDOM = 44
LS = (4, 5, 7, 63, 64, 65, 255, 256, 257, 300, 333)
XLIMS = (0.5, 1.0, 2.0, 3.7)
DTS = (2e-4, 5e-4, 1e-3, 2.5e-3)
BETAS = (0.0, 0.75, 2.0, 3.0, 8.0, 30.0)
RHO0S = (0.3, 1.0, 5.0)
NOISES = (0.05, 0.2, 0.6)
N_TRACERS = (0, 1, 3, 64, 257)
FIELD_KEYS = R.KEYS
TRACER_M_SITE, TRACER_MARGIN, ORACLE_GRADE = 1e-10, 1e-9, 1e-11


def _sig(x, digits=4):
    return float(f"{x:.{digits}g}")


# random draw -> another stream, where the first one gave an ill-conditioned run: one that amplifies a perturbation of its initial
# state by more than AMPLIFICATION_CAP (`amplification` below measures it on the reference alone, no oracle and no device involved).
# An explicit advection beyond its CFL limit, or a reaction with rate * dt >> 1 at beta = 30, is unstable and held only by the clip at
# zero; two correct binary64 implementations then end far apart, and the run measures nothing.  The cap: binary64 round-off (1e-16
# per operation, some ten operations per site and step) times 1e3 is 1e-12, a tenth of the standing bar.  The four draws replaced
# amplified by 4e3 (7), 9e3 (8), 2e5 (22) and 4e4 (36); every other draw stays below 5e2.  tests/test_pde_cases_cpu.py asserts
# the cap for the whole list.
REDRAW = {7: 1, 8: 1, 22: 1, 36: 1}
AMPLIFICATION_CAP = 1e3


@functools.lru_cache(maxsize=None)
def random_draws(n=N_RANDOM, seed=RANDOM_SEED):
    order_rng = np.random.default_rng(seed)
    order = np.concatenate([order_rng.permutation(len(LS)) for _ in range((n + len(LS) - 1) // len(LS))])
    out = []
    for j in range(n):
        rng = np.random.default_rng([seed, j, REDRAW.get(j, 0)])
        L = LS[int(order[j])]
        xlim = XLIMS[int(rng.integers(len(XLIMS)))]
        dt = DTS[int(rng.integers(len(DTS)))]
        nsteps = int(rng.integers(30, 161))
        every = int(rng.integers(1, 51))
        dx = xlim / L
        r = 0.0 if rng.random() < 0.1 else 10.0 ** rng.uniform(-3.0, np.log10(200.0))        # diffusion number gamma dt / dx^2
        cfl = rng.uniform(1.0, 2.0) if rng.random() < 0.1 else rng.uniform(0.05, 0.8)         # lam dt / dx
        gamma, lam = _sig(r * dx * dx / dt), _sig(cfl * dx / dt)
        bc = ("periodic", "neumann")[int(rng.integers(2))]
        active_model = ("bidirectional", "anchored_minus")[int(rng.integers(2))]
        pick = rng.random()
        kernel = "local" if pick < 0.2 else "global" if pick < 0.35 else "gaussian"
        sigma = _sig(xlim * 10.0 ** rng.uniform(-2.2, 0.3))
        if kernel == "global":
            sigma = 2e5
        elif kernel == "gaussian" and rng.random() < 0.12:
            sigma = 1e5 - 10                                      # the widest width that is still a convolution (ref :159)
        ntr = N_TRACERS[int(rng.integers(len(N_TRACERS)))]
        modes = (0, 1, 8, L // 2 + 1)[int(rng.integers(4))]
        systems = []
        for s in range(int(rng.integers(2, 4))):
            systems.append(dict(beta=BETAS[int(rng.integers(len(BETAS)))], init=("poisson", "homogeneous")[int(rng.integers(2))],
                                rho0=RHO0S[int(rng.integers(3))], noise=NOISES[int(rng.integers(3))], seed=1000 + 10 * j + s))
        out.append(dict(tag=f"random_{j:02d}_{kernel}_L{L}", L=L, xlim=xlim, dt=dt, nsteps=nsteps, snapshot_interval=every,
                        gamma=gamma, lam=lam, bc=bc, active_model=active_model, gaussian_kernel=kernel != "local",
                        kernel_sigma=sigma, n_tracers=ntr, n_fft_modes=min(modes, L // 2 + 1), systems=tuple(systems)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fixed_draws():
    """The "poisson" cases of tests/test_gpu_pde_sweep.py at the narrowest width, which that file leaves out because the oracle
    cannot hold the bar there: same model, seed 321, beta = 0.5 as there, and a second system."""
    base = dict(xlim=1.0, dt=5e-4, nsteps=200, snapshot_interval=100, gamma=2.33e-4, lam=0.6, gaussian_kernel=True,
                kernel_sigma=0.0005, n_tracers=257)
    systems = (dict(beta=0.5, init="poisson", rho0=1.0, noise=0.2, seed=321), dict(beta=2.0, init="poisson", rho0=1.0, noise=0.2, seed=322))
    return (dict(tag="sweep_poisson_narrow_L333", L=333, bc="periodic", active_model="bidirectional", n_fft_modes=167, systems=systems, **base),
            dict(tag="sweep_poisson_narrow_L334", L=334, bc="neumann", active_model="anchored_minus", n_fft_modes=168, systems=systems, **base))


def all_draws():
    return random_draws() + fixed_draws()


def by_tag(tag):
    return next(d for d in all_draws() if d["tag"] == tag)


def model_keywords(draw):
    """The model record of a draw, as the raw entry points and the reference take it (without kernel_sigma for a sweep)."""
    return {k: draw[k] for k in ("L", "xlim", "dt", "nsteps", "gamma", "lam", "bc", "active_model", "gaussian_kernel", "kernel_sigma",
                                 "snapshot_interval")}


class SpyPde(PdeOracle):
    """PdeOracle that keeps the magnetisation field every step's tracers read and, of every flip draw, the spin states before it
    and the two rates it is compared with."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._in_step, self._last_m, self.m_fields, self.flips = False, None, [], []

    def magnetization(self):
        m = super().magnetization()
        if not self._in_step:
            self._last_m = m
        return m

    def cw_rate(self, sigma, m):
        rate = super().cw_rate(sigma, m)
        if not self._in_step:                                      # solve()'s two calls per step: sigma = +1, then -1
            if sigma > 0:
                self.flips.append([self.tracer_state.copy(), rate])
            else:
                self.flips[-1].append(rate)
        return rate

    def step(self):
        self.m_fields.append(np.broadcast_to(self._last_m, (self.L,)).copy())
        self._in_step = True
        try:
            super().step()
        finally:
            self._in_step = False

    def solve(self, record_randoms=False):
        super().solve(record_randoms=record_randoms)
        self.m_fields.append(np.broadcast_to(self._last_m, (self.L,)).copy())


def oracle_system(draw, s):
    """(start, oracle after its run) of system s: the oracle's own seeded initial state, its random numbers recorded."""
    sysd = draw["systems"][s]
    T = (draw["nsteps"] + 0.5) * draw["dt"]
    kw = {k: v for k, v in model_keywords(draw).items() if k != "nsteps"}
    o = SpyPde(T=T, beta=sysd["beta"], seed=sysd["seed"], **kw)
    assert o.nsteps == draw["nsteps"], (draw["tag"], o.nsteps)
    o.initialize(mode=sysd["init"], rho0=sysd["rho0"], noise=sysd["noise"], n_tracers=draw["n_tracers"])
    start = dict(rho_p=o.rho_p.copy(), rho_m=o.rho_m.copy(), tx=o.tracers_unwrapped.copy(), ts=o.tracer_state.astype(np.int8))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)              # without tracers the oracle, like the reference, takes means of nothing
        o.solve(record_randoms=True)
    return start, o


def oracle_deviations(want, ref, s, n_modes):
    """d_oracle of system s: the oracle's output `want` against the reference's batch `ref`."""
    d = {k: R.deviation(want[k], ref[k][s], k) for k in FIELD_KEYS}
    d["fft"] = 0.0
    if n_modes:
        d["fft"] = float(max(np.max(np.abs(want["fft_phase"][:, :n_modes].real.astype(R.LD) - ref["fft_re"][s])),
                             np.max(np.abs(want["fft_phase"][:, :n_modes].imag.astype(R.LD) - ref["fft_im"][s]))))
    return d


@functools.lru_cache(maxsize=None)
def _runs(tag):
    draw = by_tag(tag)
    S, ntr = len(draw["systems"]), draw["n_tracers"]
    pairs = [oracle_system(draw, s) for s in range(S)]
    starts, orcs = [p[0] for p in pairs], [p[1] for p in pairs]
    ref = R.solve(**model_keywords(draw), betas=[sd["beta"] for sd in draw["systems"]], rho_p0=np.array([st["rho_p"] for st in starts]),
                  rho_m0=np.array([st["rho_m"] for st in starts]), n_fft_modes=draw["n_fft_modes"], keep_m=True)
    wants = [o.get_output() for o in orcs]
    d_sys = [oracle_deviations(wants[s], ref, s, draw["n_fft_modes"]) for s in range(S)]
    d_oracle = {k: max(d[k] for d in d_sys) for k in d_sys[0]}
    m_site = max(float(np.max(np.abs(np.array(o.m_fields).astype(R.LD) - ref["m_fields"][s]))) for s, o in enumerate(orcs))
    margin = np.inf
    if ntr:
        for o in orcs:
            for (state, r_plus, r_minus), u in zip(o.flips, o.rand_u):
                margin = min(margin, float(np.min(np.abs(u - np.where(state == 1, r_plus, r_minus) * draw["dt"]))))
    out = dict(draw=draw, starts=starts, oracles=orcs, wants=wants, ref=ref, d_sys=d_sys, d_oracle=d_oracle, m_site=m_site, margin=margin,
               rand_u=np.array([o.rand_u for o in orcs]) if ntr else None, rand_n=np.array([o.rand_n for o in orcs]) if ntr else None,
               tracer_comparable=bool(m_site <= TRACER_M_SITE and margin >= TRACER_MARGIN),
               oracle_grade=bool(2.0 * max(d_oracle[k] for k in FIELD_KEYS) <= ORACLE_GRADE))
    for v in list(ref.values()) + [a for st in starts for a in st.values()] + [a for w in wants for a in w.values()]:
        v.setflags(write=False)
    return out


def runs(draw):
    return _runs(draw["tag"])


# ----------------------------------------------------------------------------- the device paths
# name -> (entry point, its keywords beyond the model and the start, PDE_SPECTRAL_MAX_LOG2 or None, Gaussian-kernel draws only)
PATHS = {
    "one_workgroup": ("solve_batch_raw", {}, None, False),
    "wide_direct_1": ("solve_batch_raw", dict(workgroups=1), None, False),
    "wide_direct_2": ("solve_batch_raw", dict(workgroups=2), None, False),
    "wide_direct_7": ("solve_batch_raw", dict(workgroups=7), None, False),
    "wide_spectral": ("solve_batch_raw", dict(workgroups="auto", convolution="spectral"), None, True),
    "wide_spectral_cap8": ("solve_batch_raw", dict(workgroups=7, convolution="spectral"), 8, True),
    "sweep_direct": ("solve_sweep_raw", {}, None, False),
    "sweep_spectral": ("solve_sweep_raw", dict(convolution="spectral"), None, True),
}
SPECTRAL = tuple(p for p, v in PATHS.items() if v[3])


def is_convolution(draw):
    return R.kernel_mode(draw["gaussian_kernel"], draw["kernel_sigma"]) == 1


def eligible(pde, draw, path):
    """Whether the library's plan (no device) takes the draw's shape on `path`; a spectral path takes only the draws whose
    magnetisation is a convolution (on the others no transform runs: the path is the direct one, bit for bit).  The caller
    has set PDE_SPECTRAL_MAX_LOG2 as PATHS says."""
    entry, ext, cap, conv_only = PATHS[path]
    if conv_only and not is_convolution(draw):
        return False
    kw = {k: v for k, v in model_keywords(draw).items()}
    S = len(draw["systems"])
    assert (os.environ.get("PDE_SPECTRAL_MAX_LOG2") or None) == (None if cap is None else str(cap))
    try:
        if entry == "solve_sweep_raw":
            sigma = kw.pop("kernel_sigma")
            pde.sweep_plan(kernel_sigmas=[sigma] * S, n_tracers=draw["n_tracers"], fft_modes=draw["n_fft_modes"],
                           convolution=ext.get("convolution"), **kw)
        elif "workgroups" in ext:
            pde.plan(n_systems=S, n_tracers=draw["n_tracers"], fft_modes=draw["n_fft_modes"], **ext, **kw)
        return True
    except Exception as e:                                         # capi.ApsError: the plan's refusal
        assert type(e).__name__ == "ApsError", e
        return False


def candidates(path):
    """The draws a path is asked to take: all of them, for a spectral path those whose magnetisation is a convolution."""
    return tuple(d["tag"] for d in all_draws() if not PATHS[path][3] or is_convolution(d))


def eligible_tags(path):
    """The draws of `path` by the committed table (no library is asked: test collection uses this)."""
    return tuple(t for t in candidates(path) if t not in INELIGIBLE[path])


def batching_tags(path):
    """Three draws per path for the batching check: the first, the middle and the last eligible one."""
    t = eligible_tags(path)
    return (t[0], t[len(t) // 2], t[-1])


def amplification(draw):
    """By how much the draw's run amplifies a perturbation of its initial state: the reference run again from states moved by
    up to 2^-55 relative, its deviation from the first run (largest over fields, series and systems) over 2^-55."""
    run, e = runs(draw), R.LD(2.0 ** -55)
    rng = np.random.default_rng(7)
    p0 = np.array([st["rho_p"] for st in run["starts"]]).astype(R.LD)
    m0 = np.array([st["rho_m"] for st in run["starts"]]).astype(R.LD)
    p1, m1 = (a * (1 + e * rng.uniform(-1.0, 1.0, a.shape).astype(R.LD)) for a in (p0, m0))
    again = R.solve(**model_keywords(draw), betas=[sd["beta"] for sd in draw["systems"]], rho_p0=p1, rho_m0=m1)
    return max(R.deviation(again[k][s], run["ref"][k][s], k) for k in FIELD_KEYS for s in range(len(p0))) / float(e)


# ----------------------------------------------------------------------------- committed values (tests/test_pde_cases_cpu.py)
# path -> the candidates its plan refuses: fewer than PDEW_MIN_SLAB = 4 sites per slab, or under PDE_SPECTRAL_MAX_LOG2 = 8 a kernel
# that reaches beyond a quarter of 256 words
INELIGIBLE = {
    "one_workgroup": (),
    "wide_direct_1": (),
    "wide_direct_2": ("random_00_gaussian_L7", "random_01_gaussian_L4", "random_06_gaussian_L5", "random_11_local_L5",
                     "random_12_gaussian_L4", "random_17_global_L7", "random_26_local_L5", "random_27_gaussian_L7",
                     "random_31_gaussian_L4", "random_33_gaussian_L4", "random_39_gaussian_L5", "random_41_gaussian_L7"),
    "wide_direct_7": ("random_00_gaussian_L7", "random_01_gaussian_L4", "random_06_gaussian_L5", "random_11_local_L5",
                     "random_12_gaussian_L4", "random_17_global_L7", "random_26_local_L5", "random_27_gaussian_L7",
                     "random_31_gaussian_L4", "random_33_gaussian_L4", "random_39_gaussian_L5", "random_41_gaussian_L7"),
    "wide_spectral": (),
    "wide_spectral_cap8": ("random_00_gaussian_L7", "random_01_gaussian_L4", "random_02_gaussian_L300", "random_03_gaussian_L257",
                          "random_04_gaussian_L256", "random_06_gaussian_L5", "random_07_gaussian_L255", "random_12_gaussian_L4",
                          "random_24_gaussian_L255", "random_27_gaussian_L7", "random_29_gaussian_L257", "random_30_gaussian_L256",
                          "random_31_gaussian_L4", "random_32_gaussian_L333", "random_33_gaussian_L4", "random_38_gaussian_L256",
                          "random_39_gaussian_L5", "random_41_gaussian_L7", "random_43_gaussian_L333"),
    "sweep_direct": (),
    "sweep_spectral": (),
}

# draw -> the maxima over its systems of d_oracle per key, m_site and margin (None: no tracers), as `runs` gives them
YARDSTICKS = {
    "random_00_gaussian_L7": dict(rho_p=3.48e-10, rho_m=1.52e-10, m_series=1.44e-06, var_series=9.43e-11,
        snapshots=3.63e-11, m_snapshots=1.91e-10, fft=3.26e-11, m_site=9.91e-06, margin=1.13509e-05),
    "random_01_gaussian_L4": dict(rho_p=2.43e-15, rho_m=3.81e-15, m_series=1.27e-14, var_series=7.08e-15,
        snapshots=2.82e-15, m_snapshots=1.15e-14, fft=7.23e-16, m_site=4.42e-14, margin=0.000334486),
    "random_02_gaussian_L300": dict(rho_p=1.77e-14, rho_m=2.58e-14, m_series=3.23e-14, var_series=1.8e-14,
        snapshots=1.17e-14, m_snapshots=1.24e-14, fft=0, m_site=2.09e-14, margin=0.00145586),
    "random_03_gaussian_L257": dict(rho_p=9.9e-15, rho_m=9.26e-15, m_series=1.87e-14, var_series=5.88e-15,
        snapshots=3.02e-15, m_snapshots=7.19e-15, fft=3.6e-17, m_site=3.87e-16, margin=0.000102535),
    "random_04_gaussian_L256": dict(rho_p=9.45e-15, rho_m=1.1e-14, m_series=8.78e-14, var_series=5.52e-15,
        snapshots=6.55e-15, m_snapshots=9.52e-15, fft=4.07e-17, m_site=3.3e-16, margin=1.01239e-06),
    "random_05_local_L333": dict(rho_p=6.24e-13, rho_m=7.16e-13, m_series=2.45e-12, var_series=6.51e-13,
        snapshots=1.1e-12, m_snapshots=1.1e-12, fft=9.94e-16, m_site=9.46e-13, margin=0.00184771),
    "random_06_gaussian_L5": dict(rho_p=5.56e-15, rho_m=4.54e-15, m_series=2.77e-13, var_series=1.11e-13,
        snapshots=5.13e-15, m_snapshots=5.28e-15, fft=1.08e-15, m_site=7.28e-13, margin=3.96933e-05),
    "random_07_gaussian_L255": dict(rho_p=3.16e-14, rho_m=3.16e-14, m_series=3.61e-15, var_series=4.51e-14,
        snapshots=9.99e-15, m_snapshots=2.3e-14, fft=7.97e-17, m_site=1.07e-15, margin=0.00376698),
    "random_08_global_L63": dict(rho_p=2.97e-14, rho_m=3.79e-14, m_series=1.17e-12, var_series=1.04e-14,
        snapshots=1.56e-14, m_snapshots=5.11e-14, fft=2.8e-16, m_site=1.82e-14, margin=1.50982e-07),
    "random_09_local_L64": dict(rho_p=3.62e-15, rho_m=1.9e-15, m_series=1.8e-14, var_series=2.35e-15,
        snapshots=3.03e-15, m_snapshots=3.65e-15, fft=2.58e-17, m_site=2.98e-13, margin=0.00273164),
    "random_10_gaussian_L65": dict(rho_p=1.57e-14, rho_m=1.58e-14, m_series=1.84e-14, var_series=2.26e-14,
        snapshots=1.48e-14, m_snapshots=1.48e-14, fft=1.23e-16, m_site=9.63e-16, margin=6.55222e-05),
    "random_11_local_L5": dict(rho_p=1.93e-14, rho_m=1.59e-14, m_series=3.97e-14, var_series=4.85e-15,
        snapshots=1.71e-14, m_snapshots=1.54e-14, fft=0, m_site=1.77e-15, margin=3.4671e-06),
    "random_12_gaussian_L4": dict(rho_p=1.75e-15, rho_m=5.23e-16, m_series=3.51e-14, var_series=1.2e-15,
        snapshots=9e-16, m_snapshots=3.73e-14, fft=0, m_site=1.16e-15, margin=4.42198e-06),
    "random_13_gaussian_L333": dict(rho_p=1.27e-14, rho_m=1.23e-14, m_series=4.92e-15, var_series=1.22e-14,
        snapshots=5.84e-15, m_snapshots=9.68e-15, fft=3.6e-17, m_site=7.92e-14, margin=6.94751e-05),
    "random_14_gaussian_L65": dict(rho_p=8.62e-07, rho_m=8.63e-07, m_series=1.29e-06, var_series=7e-07,
        snapshots=2.84e-07, m_snapshots=2.85e-07, fft=1.35e-08, m_site=5.72e-05, margin=0.00406029),
    "random_15_local_L255": dict(rho_p=1.79e-14, rho_m=1.79e-14, m_series=2.52e-14, var_series=7.36e-15,
        snapshots=1.26e-14, m_snapshots=5.93e-15, fft=6.74e-17, m_site=1.39e-14, margin=1.32761e-06),
    "random_16_local_L257": dict(rho_p=4.24e-15, rho_m=4.94e-15, m_series=2.84e-16, var_series=3.58e-15,
        snapshots=2.19e-15, m_snapshots=4.54e-15, fft=0, m_site=2.09e-15, margin=5.07256e-06),
    "random_17_global_L7": dict(rho_p=4.83e-15, rho_m=1.06e-14, m_series=5.29e-13, var_series=6.11e-15,
        snapshots=5.51e-15, m_snapshots=9.85e-14, fft=8.58e-16, m_site=4.41e-15, margin=1.03079e-06),
    "random_18_local_L64": dict(rho_p=6.83e-15, rho_m=6.27e-15, m_series=6.42e-14, var_series=1.42e-14,
        snapshots=6.74e-15, m_snapshots=6.88e-15, fft=1.27e-16, m_site=1.04e-12, margin=2.36546e-06),
    "random_19_global_L300": dict(rho_p=4.74e-14, rho_m=5.1e-14, m_series=2.06e-13, var_series=4.57e-14,
        snapshots=3.07e-14, m_snapshots=2.38e-13, fft=1.05e-16, m_site=5.31e-15, margin=0.0349945),
    "random_20_global_L256": dict(rho_p=1.3e-14, rho_m=1.44e-14, m_series=5.89e-14, var_series=1.1e-14,
        snapshots=1.24e-14, m_snapshots=9.61e-14, fft=0, m_site=1.56e-16, margin=0.00409887),
    "random_21_gaussian_L63": dict(rho_p=9e-15, rho_m=1.54e-14, m_series=4.47e-14, var_series=1.26e-14,
        snapshots=1.42e-14, m_snapshots=5.61e-14, fft=2e-16, m_site=4.46e-14, margin=0.00016082),
    "random_22_gaussian_L64": dict(rho_p=6.99e-14, rho_m=6.15e-14, m_series=6.73e-14, var_series=7.79e-16,
        snapshots=3.51e-14, m_snapshots=5.92e-14, fft=9.78e-16, m_site=2.93e-14, margin=0.000124649),
    "random_23_global_L300": dict(rho_p=2.12e-14, rho_m=2.16e-14, m_series=1.41e-14, var_series=5.44e-15,
        snapshots=7.84e-15, m_snapshots=9.14e-15, fft=6.9e-17, m_site=2.28e-16, margin=2.48744e-06),
    "random_24_gaussian_L255": dict(rho_p=6.24e-15, rho_m=7.72e-15, m_series=2.49e-15, var_series=1.15e-14,
        snapshots=6.65e-15, m_snapshots=1.82e-14, fft=0, m_site=3.9e-16, margin=None),
    "random_25_global_L63": dict(rho_p=7.64e-15, rho_m=1.33e-14, m_series=8.25e-14, var_series=1.65e-14,
        snapshots=7.34e-15, m_snapshots=4.04e-14, fft=4.46e-17, m_site=1.29e-16, margin=None),
    "random_26_local_L5": dict(rho_p=9.25e-14, rho_m=9.23e-14, m_series=7.7e-16, var_series=1.23e-13,
        snapshots=5.63e-14, m_snapshots=6.06e-14, fft=1.85e-14, m_site=4.75e-16, margin=None),
    "random_27_gaussian_L7": dict(rho_p=9.66e-07, rho_m=2.2e-15, m_series=4.33e-05, var_series=4.24e-15,
        snapshots=1.53e-15, m_snapshots=1.6e-15, fft=2.88e-16, m_site=0.00024, margin=None),
    "random_28_local_L65": dict(rho_p=4.58e-15, rho_m=4.91e-15, m_series=1.08e-13, var_series=7.13e-15,
        snapshots=3.75e-15, m_snapshots=6.64e-14, fft=5.94e-17, m_site=3.52e-15, margin=0.00236243),
    "random_29_gaussian_L257": dict(rho_p=5.2e-15, rho_m=8.74e-15, m_series=2.99e-14, var_series=7.25e-15,
        snapshots=3.93e-15, m_snapshots=7.57e-15, fft=2.16e-17, m_site=1.79e-14, margin=4.81648e-05),
    "random_30_gaussian_L256": dict(rho_p=1.39e-14, rho_m=1.55e-14, m_series=5.62e-14, var_series=8.44e-15,
        snapshots=1.04e-14, m_snapshots=2.4e-14, fft=5.23e-17, m_site=2.31e-14, margin=0.000248585),
    "random_31_gaussian_L4": dict(rho_p=3.28e-14, rho_m=3.28e-14, m_series=1.18e-13, var_series=4.95e-15,
        snapshots=3.17e-14, m_snapshots=3.24e-14, fft=8.21e-15, m_site=1.19e-13, margin=None),
    "random_32_gaussian_L333": dict(rho_p=7.63e-12, rho_m=7.63e-12, m_series=5.96e-09, var_series=1.51e-11,
        snapshots=2e-10, m_snapshots=2.75e-10, fft=1.93e-15, m_site=8.08e-08, margin=None),
    "random_33_gaussian_L4": dict(rho_p=7.66e-14, rho_m=7.78e-14, m_series=3.8e-15, var_series=9.68e-18,
        snapshots=1.68e-14, m_snapshots=5.78e-14, fft=1.93e-14, m_site=7.83e-16, margin=None),
    "random_34_local_L300": dict(rho_p=1.11e-14, rho_m=1.13e-14, m_series=1.93e-14, var_series=5.36e-16,
        snapshots=5.28e-15, m_snapshots=5.23e-15, fft=3.05e-17, m_site=5.32e-15, margin=0.000855411),
    "random_35_gaussian_L257": dict(rho_p=1.15e-14, rho_m=1.15e-14, m_series=1.86e-13, var_series=8.48e-15,
        snapshots=5.86e-15, m_snapshots=9.01e-15, fft=3.07e-17, m_site=1.07e-14, margin=None),
    "random_36_gaussian_L65": dict(rho_p=1.71e-14, rho_m=2.66e-14, m_series=1.13e-14, var_series=1.91e-15,
        snapshots=9.19e-15, m_snapshots=1.19e-14, fft=3.28e-16, m_site=1.14e-14, margin=0.000356807),
    "random_37_local_L63": dict(rho_p=1.24e-13, rho_m=1.21e-13, m_series=4.38e-13, var_series=4.2e-15,
        snapshots=8.12e-14, m_snapshots=9.63e-14, fft=0, m_site=2.98e-15, margin=None),
    "random_38_gaussian_L256": dict(rho_p=3.96e-15, rho_m=4.28e-15, m_series=3.59e-14, var_series=7.11e-15,
        snapshots=3.54e-15, m_snapshots=2.05e-14, fft=1.26e-17, m_site=5.15e-16, margin=4.46451e-07),
    "random_39_gaussian_L5": dict(rho_p=5.34e-15, rho_m=3.4e-15, m_series=3.61e-15, var_series=3.92e-15,
        snapshots=2.86e-15, m_snapshots=4.21e-15, fft=3.85e-16, m_site=3.98e-15, margin=None),
    "random_40_global_L255": dict(rho_p=6.17e-15, rho_m=6.13e-15, m_series=4.14e-15, var_series=6.27e-15,
        snapshots=5.02e-15, m_snapshots=1.2e-14, fft=1.89e-17, m_site=4.14e-15, margin=1.42095e-05),
    "random_41_gaussian_L7": dict(rho_p=1.52e-13, rho_m=1.47e-13, m_series=3.79e-14, var_series=6.54e-16,
        snapshots=7.19e-14, m_snapshots=1.28e-13, fft=2.21e-14, m_site=3.75e-15, margin=None),
    "random_42_gaussian_L64": dict(rho_p=3.18e-14, rho_m=3.46e-14, m_series=9.75e-15, var_series=3.8e-16,
        snapshots=1.27e-14, m_snapshots=6.37e-15, fft=4e-16, m_site=2.92e-15, margin=7.42606e-06),
    "random_43_gaussian_L333": dict(rho_p=8.49e-15, rho_m=8.65e-15, m_series=1.4e-14, var_series=2.51e-15,
        snapshots=5.02e-15, m_snapshots=6.56e-15, fft=1.99e-17, m_site=5.18e-16, margin=0.00210459),
    "sweep_poisson_narrow_L333": dict(rho_p=3.39e-14, rho_m=3.32e-14, m_series=9.51e-08, var_series=2.77e-14,
        snapshots=1.54e-14, m_snapshots=3.41e-14, fft=9.96e-17, m_site=8.34e-07, margin=4.60246e-06),
    "sweep_poisson_narrow_L334": dict(rho_p=2.23e-14, rho_m=2.01e-14, m_series=8.94e-09, var_series=9.15e-15,
        snapshots=1.24e-14, m_snapshots=4.96e-14, fft=2.21e-17, m_site=1.09e-06, margin=5.7221e-06),
}
