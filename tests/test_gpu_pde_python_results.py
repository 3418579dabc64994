"""GPU suite (-m gpu): what the public functions of the hydrodynamic-limit PDE solver return, end to end and bit for bit.

The other GPU modules of the solver compare with the oracle within tolerances.  Kernels, Philox streams and the library being
fixed, the same call must give the same bits whatever the Python layer and the host drivers do on the way, so every case here is
held to a CRC of each array it returns (NaNs by their bits) and the repr of each scalar; kernel_ms is left out.

The expected values are tests/golden/pde_python_results.json, recorded on an MI355X from the package and library of commit
a987597, the parent of the commit that added this file (there every entry point of pde.py and every host driver wrote its
staging out for itself), by

    python tests/test_gpu_pde_python_results.py --record [out.json]      (run in a checkout of a987597 that holds a copy of this file)

Shapes, chosen so that each branch of the host staging is crossed once.  One-workgroup shape: L = 300 and 333 (two sites per
thread, no multiple of 256), 24 steps with snapshots every 5, two betas, 8 tracers, 3 Fourier modes; periodic and Neumann, both
active models, the three kernel modes; one case without tracers and snapshots; L = 3200 (fields in global memory), 4 steps.
Wide shape: L = 300 on 3 slabs and on "auto", direct and spectral.  Sweep: L = 333, three widths (the last one the global
mean) against two betas, direct and spectral.  The class and both drivers.  Tracer noise from the device's Philox and from
rand_u / rand_n given.  `--record` refuses a spectral case that plan() / sweep_plan() would refuse, and any exception."""
import importlib
import json
import os
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"
FIXTURE = os.path.join(ROOT, "tests", "golden", "pde_python_results.json")
pde = importlib.import_module(PKG + ".pde")

DT, NSTEPS = 4e-3, 24                      # window = int(0.05 / dt) = 12 steps: v_eff / D_eff leave NaN inside the run
T = (NSTEPS + 0.5) * DT                    # int(T / dt) = 24 whatever the last bit of the quotient
BETAS = [1.5, 2.5]
WIDTHS = [0.02, 0.2, 2e5]


def digest(x):
    """A structure of dicts, lists, arrays and scalars as JSON: a CRC (with dtype and shape) per array, repr for scalars."""
    if isinstance(x, dict):
        return {str(k): digest(v) for k, v in x.items() if k != "kernel_ms"}
    if isinstance(x, (list, tuple)):
        return [digest(v) for v in x]
    if isinstance(x, (np.ndarray, np.generic)):
        a = np.ascontiguousarray(x)
        return f"{a.dtype.str}{list(a.shape)}:{zlib.crc32(a.tobytes()):08x}"
    return repr(x)


def start(L, S, ntr, rand=False, nsteps=NSTEPS):
    g = np.random.default_rng(1000 + L)
    rp, rm = g.random((S, L)) + 0.5, g.random((S, L)) + 0.5
    tot = (rp + rm).sum(axis=1, keepdims=True)
    kw = dict(rho_p0=rp / tot, rho_m0=rm / tot)
    if ntr:
        kw.update(tracer_x0=g.random((S, ntr)), tracer_s0=g.choice(np.array([-1, 1], np.int8), (S, ntr)))
    if rand:
        kw.update(rand_u=g.random((S, nsteps + 1, ntr)), rand_n=g.standard_normal((S, nsteps + 1, ntr)))
    return kw


def raw(L=300, betas=BETAS, ntr=8, rand=False, nsteps=NSTEPS, **kw):
    base = dict(L=L, xlim=1.0, dt=DT, nsteps=nsteps, gamma=2.33e-4, lam=0.6, betas=betas, bc="periodic", active_model="bidirectional",
                gaussian_kernel=False, kernel_sigma=0.02, snapshot_interval=5, fft_modes=3, seed=7, **start(L, len(betas), ntr, rand, nsteps))
    base.update(kw)
    return base


GAUSS = dict(gaussian_kernel=True)
MEAN = dict(gaussian_kernel=True, kernel_sigma=2e5)
OTHER = dict(bc="neumann", active_model="anchored_minus")
BARE = dict(ntr=0, want_snapshots=False, fft_modes=0)
SWEEP_AXES = dict(betas=np.repeat(BETAS, len(WIDTHS)), kernel_sigmas=np.tile(WIDTHS, len(BETAS)))
CTOR = dict(L=300, T=T, dt=DT, gaussian_kernel=True, seed=3)


SPECTRAL_PLANS = []        # what plan() / sweep_plan() must accept before a spectral case is recorded (host arithmetic; no GPU)


def plan_keywords(args):
    """The keywords of plan() / sweep_plan() out of those of a raw solve."""
    skip = ("betas", "rho_p0", "rho_m0", "tracer_x0", "tracer_s0", "rand_u", "rand_n", "seed", "want_snapshots")
    return dict({k: v for k, v in args.items() if k not in skip}, n_tracers=np.shape(args["tracer_x0"])[-1] if "tracer_x0" in args else 0)


def batch(**kw):
    if kw.get("convolution") == "spectral":
        SPECTRAL_PLANS.append(lambda: pde.plan(n_systems=len(raw(**kw)["betas"]), **plan_keywords(raw(**kw))))
    return lambda: pde.solve_batch_raw(**raw(**kw))


def sweep(**kw):
    def args():
        a = raw(L=333, betas=SWEEP_AXES["betas"], gaussian_kernel=True, kernel_sigmas=SWEEP_AXES["kernel_sigmas"], **kw)
        del a["kernel_sigma"]
        return a
    if kw.get("convolution") == "spectral":
        SPECTRAL_PLANS.append(lambda: pde.sweep_plan(**plan_keywords(args())))
    return lambda: pde.solve_sweep_raw(**args())


def solver_state(s):
    return dict(output=s.get_output(), tracers=s.tracers, tracers_unwrapped=s.tracers_unwrapped, tracer_state=s.tracer_state)


def class_calls():
    s = pde.IMEXPDE(fft_modes=3, **CTOR)
    s.initialize(n_tracers=8)
    out = [s.solve_batch(BETAS, want_snapshots=True), s.solve_batch(BETAS, workgroups=3, fft_modes=2, convolution="spectral"),
           s.solve_batch(BETAS), s.solve_sweep(betas=BETAS, kernel_sigmas=[0.02, 0.2], convolution="spectral", want_snapshots=True)]
    s.solve()
    return out + [solver_state(s), solver_state(s.solve())]


def class_defaults():
    """record_fft on with no fft_modes: L // 2 + 1 modes; no seed: the seed of the call is drawn, the tracers come from rand_u / rand_n."""
    np.random.seed(12)
    s = pde.IMEXPDE(L=300, T=T, dt=DT, bc="neumann", workgroups="auto")
    s.initialize(mode="homogeneous", n_tracers=8)
    g = np.random.default_rng(5)
    return solver_state(s.solve(rand_u=g.random((NSTEPS + 1, 8)), rand_n=g.standard_normal((NSTEPS + 1, 8))))


CASES = [
    ("batch-L300-local", batch()),
    ("batch-L333-gaussian-neumann-anchored", batch(L=333, **GAUSS, **OTHER)),
    ("batch-L333-mean-anchored", batch(L=333, active_model="anchored_minus", **MEAN)),
    ("batch-L300-gaussian-neumann-rand", batch(rand=True, bc="neumann", **GAUSS)),
    ("batch-L300-bare", batch(**BARE)),
    ("batch-L333-gaussian-bare", batch(L=333, **GAUSS, **BARE)),
    ("batch-L3200-global-memory", batch(L=3200, nsteps=4, snapshot_interval=3, **GAUSS)),
    ("wide-3-direct", batch(workgroups=3, **GAUSS)),
    ("wide-auto-direct-neumann-anchored", batch(workgroups="auto", **GAUSS, **OTHER)),
    ("wide-3-spectral", batch(workgroups=3, convolution="spectral", **GAUSS)),
    ("wide-auto-spectral-neumann-anchored-rand", batch(workgroups="auto", convolution="spectral", rand=True, **GAUSS, **OTHER)),
    ("wide-3-local-bare", batch(workgroups=3, **BARE)),
    ("wide-3-spectral-bare", batch(workgroups=3, convolution="spectral", **GAUSS, **BARE)),
    ("wide-auto-mean-rand", batch(workgroups="auto", rand=True, **MEAN)),
    ("sweep-direct", sweep()),
    ("sweep-spectral-neumann-anchored", sweep(convolution="spectral", **OTHER)),
    ("sweep-spectral-rand", sweep(convolution="spectral", rand=True)),
    ("sweep-direct-bare", sweep(**BARE)),
    ("class", class_calls),
    ("class-defaults-seed-drawn", class_defaults),
    ("sweep_over_betas", lambda: pde.sweep_over_betas(BETAS, n_runs=2, t_min=0.05, t_max=0.09, init_kwargs=dict(n_tracers=8),
                                                      L=300, T=T, dt=DT, gaussian_kernel=True)[:4]),
    ("sweep_over_betas-wide-spectral", lambda: pde.sweep_over_betas(BETAS, n_runs=2, t_min=0.05, t_max=0.09, init_kwargs=dict(n_tracers=8), workgroups=3,
                                                                    fft_modes=2, convolution="spectral", L=300, T=T, dt=DT, gaussian_kernel=True)[:4]),
    ("sweep_over_kernel_sigmas", lambda: pde.sweep_over_kernel_sigmas([0.02, 0.2], n_runs=2, init_kwargs=dict(n_tracers=8), L=333, T=T, dt=DT)),
    ("sweep_over_kernel_sigmas-spectral", lambda: pde.sweep_over_kernel_sigmas([0.02, 2e5], n_runs=2, init_kwargs=dict(n_tracers=8), convolution="spectral",
                                                                               L=333, T=T, dt=DT, bc="neumann")),
]

# the spectral launches of the class and driver cases, restated (the raw cases above add their own)
CLASS = dict(dt=DT, nsteps=NSTEPS, gaussian_kernel=True, n_tracers=8, convolution="spectral")
SPECTRAL_PLANS += [
    lambda: pde.plan(L=300, workgroups=3, n_systems=2, fft_modes=2, **CLASS),                                   # class: solve_batch
    lambda: pde.sweep_plan(L=300, kernel_sigmas=[0.02, 0.2], fft_modes=3, **CLASS),                             # class: solve_sweep
    lambda: pde.plan(L=300, workgroups=3, n_systems=4, fft_modes=2, **CLASS),                                   # sweep_over_betas-wide-spectral
    lambda: pde.sweep_plan(L=333, kernel_sigmas=[0.02, 0.02, 2e5, 2e5], bc="neumann", fft_modes=0, **CLASS),    # sweep_over_kernel_sigmas-spectral
]


def run_case(call):
    return digest(call())


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_and_case_list_agree(recorded):
    assert sorted(recorded) == sorted(name for name, _ in CASES)


def test_spectral_cases_are_eligible():
    for ask in SPECTRAL_PLANS:
        assert ask()["convolution"] == "spectral"


@pytest.mark.parametrize("name,call", CASES, ids=[name for name, _ in CASES])
def test_python_results(recorded, name, call):
    assert run_case(call) == recorded[name]


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_pde_python_results.py --record [out.json]   (on the GPU, in a checkout of the commit to record from)")
    test_spectral_cases_are_eligible()
    out = {name: run_case(call) for name, call in CASES}          # an exception ends the recording
    path = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cases recorded from {pde.__file__} into {path}")
