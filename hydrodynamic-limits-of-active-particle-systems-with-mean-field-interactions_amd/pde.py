"""`IMEXPDE` -- the reference's hydrodynamic-limit solver class (IMEX_PDE_solver_class.py:11) re-hosted on the MI355X.

Same constructor keywords (ref :13-28), `initialize()` (ref :96-131, host NumPy with the reference's legacy
`np.random` call sequence, so a seeded initial condition is the reference's), `solve()`, `get_output()` keys
(ref :293-306).  The time loop (`solve` + `step`, the per-step observables and the Euler-Maruyama tracers) runs in
one persistent HIP kernel per system behind the C ABI of include/pde.h; `solve_batch` runs many beta values at once
(the reference's sweep drivers loop over them serially, IMEX_PDE_solver_run_sweep.py:17-48).

Two execution shapes, one class.  `workgroups=None` (default): one workgroup per system (`pde_solve_batch`), right for
sweeps of small grids.  `workgroups=G` or `"auto"`: the wide shape of include/pde_wide.h (`pdew_solve`), one system cut
into G slabs on G workgroups, a time step a chain of kernel launches; right for one fine grid.  `plan()` tells what
the wide shape would use.  On the wide shape `convolution="spectral"` evaluates the Gaussian-kernel magnetisation by complex
binary64 transforms over overlap-save blocks (include/pde_spectral.h) instead of the direct sum; the default stays direct.

A sweep over the kernel width (the reference's IMEX_PDE_solver_run_sweep_magn*.py) is one launch on the one-workgroup shape:
`sweep_over_kernel_sigmas`, `solve_sweep_raw`, `IMEXPDE.solve_sweep` give every system its own kernel_sigma next to its own beta
(include/pde_sweep.h, `pdek_solve`); there `convolution="spectral"` evaluates the Gaussian-kernel magnetisation by a complex
binary64 transform held in the workgroup's LDS, which is what a kernel that spans the ring wants (eligible while
L + 2 * reach <= 2048; `sweep_plan` tells).

Differences that are part of the design: tracer noise comes from Philox4x32-10 keyed by `seed` on the device (the
reference draws from NumPy's global MT19937 inside the loop); the magnetisation kernel is applied by direct circular
convolution instead of rfft products (unless convolution="spectral" is asked for); no output directory is created; plotting methods are not reproduced.
There is no CPU fallback: without libaps_hip.so or without a GPU `solve()` raises.

Segments (include/pde_resume.h).  `solve_batch_raw` and `solve_sweep_raw` take `resume=` (a `PdeCheckpoint`: the launch runs
`nsteps` FURTHER steps), `return_checkpoint=True` (the result gains "checkpoint") and `steps_per_launch=n` (the call runs as a
chain of launches of at most n steps, merged into the dict of the single launch).  A chain has the single launch's bits as long
as every segment runs the same path (workgroups, convolution); a checkpoint does not depend on the path and may be resumed on
another, to the accuracy by which the two paths agree.  `IMEXPDE.continue_solve(T)` appends to a finished `solve()`.
"""
from __future__ import annotations

import collections
import ctypes as C
import json
import os

import numpy as np

from . import capi


class PdeParams(C.Structure):
    """struct pde_params of include/pde.h, field for field."""
    _fields_ = [("L", C.c_int32), ("nsteps", C.c_int32), ("periodic", C.c_int32), ("anchored_minus", C.c_int32),
                ("kernel_mode", C.c_int32), ("snapshot_interval", C.c_int32), ("n_tracers", C.c_int32),
                ("window", C.c_int32), ("n_fft_modes", C.c_int32), ("device", C.c_int32), ("convolution", C.c_int32),
                ("reserved", C.c_int32),
                ("xlim", C.c_double), ("dt", C.c_double), ("gamma", C.c_double), ("lam", C.c_double),
                ("kernel_sigma", C.c_double), ("seed", C.c_uint64)]


class PdewPlanInfo(C.Structure):
    """struct pdew_plan_info of include/pde_wide.h, field for field."""
    _fields_ = [("workgroups", C.c_int32), ("slab_len", C.c_int32), ("slab_len_min", C.c_int32), ("n_long_slabs", C.c_int32),
                ("ktaps", C.c_int32), ("launches_per_step", C.c_int32), ("lds_bytes", C.c_int32), ("conv_log2", C.c_int32),
                ("work_bytes", C.c_int64)]


class PdekPlanInfo(C.Structure):
    """struct pdek_plan_info of include/pde_sweep.h, field for field."""
    _fields_ = [("ktaps_max", C.c_int32), ("conv_log2_max", C.c_int32), ("lds_bytes", C.c_int32), ("fields_in_lds", C.c_int32)]


class PdeCheckpointStruct(C.Structure):
    """struct pde_checkpoint of include/pde_resume.h, field for field."""
    _fields_ = [("rho_p", C.c_void_p), ("rho_m", C.c_void_p), ("tracer_x", C.c_void_p), ("tracer_s", C.c_void_p),
                ("hist", C.c_void_p), ("step", C.c_int32)]


PDEK_MIN_LOG2, PDEK_MAX_LOG2 = 8, 11     # include/pde_sweep.h
PDE_MAX_L = 1 << 22          # fields in LDS up to L ~ 3000 (PDE_LDS_L of include/pde.h), in global memory beyond

# the launch keywords that describe the equation and the grid: what `_model` picks and `_params` reads
MODEL = ("L", "xlim", "dt", "nsteps", "gamma", "lam", "bc", "active_model", "gaussian_kernel", "kernel_sigma",
         "snapshot_interval", "device")
# the pointers every solve takes (include/pde.h): seven inputs, twelve outputs, in the ABI's order; kernel_ms follows them
SERIES = ("m_series", "var_series", "v_eff_series", "D_eff_series")
COMMON = ("beta", "rho_p0", "rho_m0", "tracer_x0", "tracer_s0", "rand_u", "rand_n", "rho_p", "rho_m") + SERIES + (
    "snapshots", "m_snapshots", "fft_re", "fft_im", "tracer_x", "tracer_s")
_PAR, _PTR, _I32, _MS = C.POINTER(PdeParams), C.c_void_p, C.c_int32, C.POINTER(C.c_double)


# The three solves: the entry's *_last_error, the C types of what it takes of its own next to the common pointers, and its call
# (`own`: that argument's value, workgroups or kernel_sigma[], which stands behind beta; `ptrs`: the common pointers, kernel_ms).
# `fn` is the entry itself or its resumable form, whose two checkpoints stand behind kernel_ms, at the end of `ptrs`.
_Solve = collections.namedtuple("_Solve", "last_error own call")
SOLVES = {
    "pde_solve_batch": _Solve("pde_last_error", [], lambda fn, par, S, own, ptrs: fn(par, S, *ptrs)),
    "pdew_solve": _Solve("pdew_last_error", [_I32], lambda fn, par, S, own, ptrs: fn(par, S, own, *ptrs)),
    "pdek_solve": _Solve("pdek_last_error", [_PTR], lambda fn, par, S, own, ptrs: fn(par, S, ptrs[0], _p(own), *ptrs[1:])),
}
# the resumable form of each solve (include/pde_resume.h): its name and its *_last_error
RESUMABLE = {"pde_solve_batch": ("pder_solve", "pder_last_error"), "pdew_solve": ("pdewr_solve", "pdewr_last_error"),
             "pdek_solve": ("pdekr_solve", "pdekr_last_error")}
_CKP = C.POINTER(PdeCheckpointStruct)
# the plans: name -> (last_error, the C types behind pde_params)
PLANS = {
    "pdew_plan": ("pdew_last_error", [_I32, _I32, C.POINTER(PdewPlanInfo)]),
    "pdek_plan": ("pdek_last_error", [_I32, _PTR, C.POINTER(PdekPlanInfo)] + [_PTR] * 3),
}


def _lib():
    lib = capi.load()
    if not getattr(lib, "_pde_ready", False):
        protos = {name: (e.last_error, [_PAR, _I32] + e.own + [_PTR] * len(COMMON) + [_MS]) for name, e in SOLVES.items()}
        protos.update({name: (last_error, [_PAR] + behind) for name, (last_error, behind) in PLANS.items()})
        protos["pdes_plan"] = ("pdes_last_error", [_I32] * 3 + [C.POINTER(_I32)] * 3)
        protos.update({new: (last_error, protos[old][1] + [_CKP, _CKP]) for old, (new, last_error) in RESUMABLE.items()})
        protos["pder_extents"] = ("pder_last_error", [_PAR, _I32] + [C.POINTER(_I32)] * 4)
        for name, (last_error, argtypes) in protos.items():
            getattr(lib, name).restype, getattr(lib, name).argtypes = C.c_int, argtypes
            getattr(lib, last_error).restype, getattr(lib, last_error).argtypes = C.c_char_p, []
        lib._pde_ready = True
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _check_workgroups(workgroups):
    """None: one workgroup per system; "auto" -> 0 (the library chooses); an integer >= 1: that many slabs per system."""
    if workgroups is None:
        return None
    if isinstance(workgroups, str):
        if workgroups != "auto":
            raise ValueError("workgroups must be None, 'auto' or an integer >= 1")
        return 0
    if isinstance(workgroups, bool) or not isinstance(workgroups, (int, np.integer)) or workgroups < 1:
        raise ValueError("workgroups must be None, 'auto' or an integer >= 1")
    return int(workgroups)


def _check_convolution(convolution, workgroups=0):
    """None or "direct" -> 0, "spectral" -> 1 (the wide shape only: workgroups must not be None)."""
    if convolution is None or (isinstance(convolution, str) and convolution == "direct"):
        return 0
    if not isinstance(convolution, str) or convolution != "spectral":
        raise ValueError("convolution must be None, 'direct' or 'spectral'")
    if workgroups is None:
        raise ValueError("convolution='spectral' belongs to the wide shape: give workgroups ('auto' or an integer >= 1)")
    return 1


def spectral_plan(L, ktaps, max_log2=21):
    """The overlap-save blocks of the spectral convolution (pdes_plan; no GPU is needed): dict with blocks, log2_m,
    block_sites for a ring of L sites and a kernel reaching ktaps sites either side; ApsError when not eligible."""
    lib = _lib()
    b, m, s = C.c_int32(), C.c_int32(), C.c_int32()
    rc = lib.pdes_plan(int(L), int(ktaps), int(max_log2), C.byref(b), C.byref(m), C.byref(s))
    if rc != 0:
        raise capi.ApsError(rc, lib.pdes_last_error().decode())
    return dict(blocks=b.value, log2_m=m.value, block_sites=s.value)


def _check_fft_modes(fft_modes, L):
    if fft_modes is None:
        return None
    if isinstance(fft_modes, bool) or not isinstance(fft_modes, (int, np.integer)) or not 0 <= fft_modes <= L // 2 + 1:
        raise ValueError("fft_modes must be None or an integer in [0, L // 2 + 1]")
    return int(fft_modes)


def _check_bc(bc):
    if bc not in ("periodic", "neumann"):
        raise ValueError("bc must be 'periodic' or 'neumann'")


def _model(kw):
    """The model record: the keywords of MODEL out of `kw`, a raw function's locals() or a solver's attributes."""
    return {k: kw[k] for k in MODEL}


def _params(*, L, xlim, dt, nsteps, gamma, lam, bc, active_model, gaussian_kernel, kernel_sigma, snapshot_interval, n_tracers,
            n_fft_modes, seed, device, convolution=0):
    """struct pde_params from the model record and what a call adds to it."""
    if not gaussian_kernel:
        mode = 0
    elif kernel_sigma > 100000:                                    # ref :161
        mode = 2
    else:
        mode = 1
    window = int(0.05 / dt)                                        # ref :238-239
    return PdeParams(L=L, nsteps=nsteps, periodic=int(bc == "periodic"), anchored_minus=int(active_model != "bidirectional"),
                     kernel_mode=mode, snapshot_interval=snapshot_interval, n_tracers=n_tracers, window=max(window, 1),
                     n_fft_modes=n_fft_modes, device=device, convolution=convolution, xlim=xlim, dt=dt, gamma=gamma, lam=lam,
                     kernel_sigma=kernel_sigma, seed=int(seed) & (2 ** 64 - 1))


def _plan(lib, name, info, kw, conv, front, behind=()):
    """The plan `name` for the keywords `kw` of plan() / sweep_plan(): pde_params without a seed, the call (`front` of and
    `behind` the info structure), the structure's fields as a dict."""
    par = _params(**_model(kw), n_tracers=kw["n_tracers"], n_fft_modes=_check_fft_modes(kw["fft_modes"], kw["L"]) or 0, seed=0,
                  convolution=conv)
    rc = getattr(lib, name)(C.byref(par), *front, C.byref(info), *behind)
    if rc != 0:
        raise capi.ApsError(rc, getattr(lib, PLANS[name][0])().decode())
    return dict({field: getattr(info, field) for field, _ in info._fields_}, convolution="spectral" if conv else "direct")


def plan(*, L, workgroups="auto", n_systems=1, xlim=1.0, dt=5e-4, T=None, nsteps=None, gamma=2.33e-4, lam=0.6, bc="periodic",
         active_model="bidirectional", gaussian_kernel=False, kernel_sigma=0.02, snapshot_interval=50, n_tracers=0,
         fft_modes=0, device=0, convolution=None):
    """What the wide shape would use for these parameters (pdew_plan; nothing is launched, no GPU is needed): dict with
    workgroups, slab_len / slab_len_min / n_long_slabs, slab_lengths (sums to L), ktaps, launches_per_step, lds_bytes,
    work_bytes, and of the convolution: convolution ("direct" | "spectral"), conv_log2 (m; 0 when no transform runs),
    conv_blocks, conv_block_sites (pdes_plan under PDE_SPECTRAL_MAX_LOG2 of the environment; 0 when no transform runs)."""
    lib = _lib()
    wg = _check_workgroups(workgroups)
    conv = _check_convolution(convolution, wg)
    if wg is None:
        raise ValueError("plan() describes the wide shape: workgroups must be 'auto' or an integer >= 1")
    if nsteps is None:
        nsteps = int(T / dt) if T is not None else 0
    info = PdewPlanInfo()
    out = _plan(lib, "pdew_plan", info, locals(), conv, (n_systems, wg))
    out["conv_blocks"] = out["conv_block_sites"] = 0
    if info.conv_log2:
        sp = spectral_plan(L, info.ktaps, int(os.environ.get("PDE_SPECTRAL_MAX_LOG2") or 21))
        assert sp["log2_m"] == info.conv_log2
        out["conv_blocks"], out["conv_block_sites"] = sp["blocks"], sp["block_sites"]
    out["slab_lengths"] = [info.slab_len] * info.n_long_slabs + [info.slab_len_min] * (info.workgroups - info.n_long_slabs)
    return out


CHECKPOINT_ARRAYS = (("rho_p", np.float64), ("rho_m", np.float64), ("tracer_x", np.float64), ("tracer_s", np.int8), ("hist", np.float64))
_FINGERPRINT = ("L", "xlim", "dt", "n_tracers", "n_systems")


class PdeCheckpoint:
    """The state of a batch of systems between two launches of the PDE solver (struct pde_checkpoint of include/pde_resume.h),
    at step `step`: after row `step` was recorded and the tracers made that row's move, before step().  Per system the fields
    `rho_p`, `rho_m` [n_systems, L], the unwrapped tracers `tracer_x` and their states `tracer_s` [n_systems, n_tracers], and
    `hist` [n_systems, window, n_tracers], the ring of the last `window` tracer positions (slot n % window: after the move of
    row n; slots no row has filled are 0); the three are None without tracers.

    With it travel the model record of the launch that left it (`model`: the keywords of MODEL), its `seed`, its `betas` and, for
    a sweep, its `kernel_sigmas` (else None).  What sizes the arrays or places the random numbers must not change on a resume:
    L, xlim, dt (the window), n_tracers and the number of systems; another value raises ValueError naming the field.  Betas,
    kernel widths and every other parameter are the resuming launch's: other values mean the same scheme with the parameter
    switched at the checkpoint's step."""

    def __init__(self, *, rho_p, rho_m, tracer_x=None, tracer_s=None, hist=None, step, model, seed, betas, kernel_sigmas=None):
        for k, dt in CHECKPOINT_ARRAYS:
            v = locals()[k]
            setattr(self, k, None if v is None else np.ascontiguousarray(v, dtype=dt))
        if self.rho_p.ndim != 2 or self.rho_m.shape != self.rho_p.shape:
            raise ValueError("PdeCheckpoint: rho_p and rho_m must be [systems][L]")
        if (self.tracer_x is None) != (self.tracer_s is None) or (self.tracer_x is None) != (self.hist is None):
            raise ValueError("PdeCheckpoint: tracer_x, tracer_s and hist come together")
        if self.tracer_x is not None and (self.tracer_x.shape != self.tracer_s.shape or self.tracer_x.shape[:1] != self.rho_p.shape[:1]
                                          or self.hist.ndim != 3 or self.hist.shape[::2] != self.tracer_x.shape):
            raise ValueError("PdeCheckpoint: tracer_x, tracer_s must be [systems][tracers], hist [systems][window][tracers]")
        self.step, self.seed, self.model = int(step), int(seed), dict(model)
        self.betas = np.ascontiguousarray(np.atleast_1d(betas), dtype=np.float64)
        self.kernel_sigmas = None if kernel_sigmas is None else np.ascontiguousarray(np.atleast_1d(kernel_sigmas), dtype=np.float64)

    n_systems = property(lambda self: self.rho_p.shape[0])
    n_tracers = property(lambda self: 0 if self.tracer_x is None else self.tracer_x.shape[1])
    L = property(lambda self: self.rho_p.shape[1])
    xlim = property(lambda self: self.model["xlim"])
    dt = property(lambda self: self.model["dt"])

    def arrays(self):
        return {k: getattr(self, k) for k, _ in CHECKPOINT_ARRAYS if getattr(self, k) is not None}

    def require(self, **expected):
        """ValueError naming the first of L, xlim, dt, n_tracers, n_systems whose value differs from `expected[field]`."""
        for k in _FINGERPRINT:
            if k in expected and getattr(self, k) != expected[k]:
                raise ValueError(f"PdeCheckpoint: the resuming run differs from the checkpoint in {k}: the checkpoint has "
                                 f"{getattr(self, k)!r}, the resuming run {expected[k]!r}")

    def struct(self):
        """struct pde_checkpoint pointing into this object's arrays (keep the object alive while the struct is in use)."""
        return PdeCheckpointStruct(step=self.step, **{k: _p(getattr(self, k)).value if getattr(self, k) is not None else None
                                                      for k, _ in CHECKPOINT_ARRAYS})

    def save(self, path):
        """One .npz: the arrays, betas, kernel widths and, as JSON, the model record, seed and step."""
        meta = dict(step=self.step, seed=self.seed, model={k: v.item() if isinstance(v, np.generic) else v for k, v in self.model.items()})
        more = {} if self.kernel_sigmas is None else dict(kernel_sigmas=self.kernel_sigmas)
        with open(path, "wb") as fh:
            np.savez(fh, meta=np.array(json.dumps(meta)), betas=self.betas, **self.arrays(), **more)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(betas=z["betas"], kernel_sigmas=z["kernel_sigmas"] if "kernel_sigmas" in z else None,
                       **{k: z[k] for k, _ in CHECKPOINT_ARRAYS if k in z}, **json.loads(str(z["meta"])))


def extents(par, from_step=-1):
    """pder_extents (host arithmetic, no GPU): (first_row, n_rows, n_snap, first_snap) of a launch of par.nsteps steps, fresh
    (from_step = -1) or resumed from a checkpoint at from_step."""
    lib = _lib()
    v = [C.c_int32() for _ in range(4)]
    rc = lib.pder_extents(C.byref(par), int(from_step), *[C.byref(x) for x in v])
    if rc != 0:
        raise capi.ApsError(rc, lib.pder_last_error().decode())
    return tuple(x.value for x in v)


def _launch(lib, name, own, model, *, betas, rho_p0, rho_m0, tracer_x0, tracer_s0, rand_u, rand_n, n_fft_modes, seed,
            want_snapshots, convolution, resume=None, return_checkpoint=False):
    """One launch of SOLVES[name], `own` its own argument: broadcasts the start fields, tracers and random numbers over the
    systems and pins them as the ABI's types, allocates the outputs, calls, raises the entry's error, returns the result dict.
    With `resume` (a PdeCheckpoint) or `return_checkpoint` the launch goes through the entry's resumable form: the start is the
    checkpoint's, model["nsteps"] counts further steps, the outputs hold this launch's rows and the result gains "first_row"
    and, when asked for, "checkpoint"."""
    L, nsteps, every = model["L"], model["nsteps"], model["snapshot_interval"]
    betas = np.ascontiguousarray(np.atleast_1d(betas), dtype=np.float64)
    S = len(betas)
    segment = resume is not None or return_checkpoint

    def pin(a, *shape, dtype=np.float64):
        return np.ascontiguousarray(np.broadcast_to(a, shape), dtype=dtype)

    if resume is not None:
        ntr = resume.n_tracers
        given = {k: np.shape(v)[-1] for k, v in (("tracer_x0", tracer_x0), ("rand_u", rand_u)) if v is not None}
        resume.require(L=L, xlim=model["xlim"], dt=model["dt"], n_systems=S, **({"n_tracers": min(given.values())} if given else {}))
        arg = dict(beta=betas)                                     # the start is the checkpoint's: rho_p0 .. tracer_s0 stay NULL
    else:
        arg = dict(beta=betas, rho_p0=pin(rho_p0, S, L), rho_m0=pin(rho_m0, S, L))   # what the C call takes, by COMMON's names
        ntr = 0 if tracer_x0 is None else np.shape(tracer_x0)[-1]
        if ntr:
            arg.update(tracer_x0=pin(tracer_x0, S, ntr), tracer_s0=pin(tracer_s0, S, ntr, dtype=np.int8))
    if rand_u is not None and not segment:
        arg.update(rand_u=pin(rand_u, S, nsteps + 1, ntr), rand_n=pin(rand_n, S, nsteps + 1, ntr))
    par = _params(**model, n_tracers=ntr, n_fft_modes=n_fft_modes, seed=seed, convolution=convolution)
    _check_bc(model["bc"])           # where solve_batch_raw has always refused a bad bc (solve_sweep_raw does before it comes here)
    first_row, n_rows, n_snap, first_snap = extents(par, -1 if resume is None else resume.step) if segment else (0, nsteps + 1, nsteps // every + 1, 0)
    if rand_u is not None and segment:
        arg.update(rand_u=pin(rand_u, S, n_rows, ntr), rand_n=pin(rand_n, S, n_rows, ntr))
    out = dict(rho_p=np.zeros((S, L)), rho_m=np.zeros((S, L)), m_series=np.zeros((S, n_rows)),
               var_series=np.zeros((S, n_rows)), v_eff_series=np.full((S, n_rows), np.nan),
               D_eff_series=np.full((S, n_rows), np.nan),
               snapshots=np.zeros((S, n_snap, L)) if want_snapshots else None,
               m_snapshots=np.zeros((S, n_snap, L)) if want_snapshots else None,
               fft_re=np.zeros((S, n_rows, n_fft_modes)) if n_fft_modes else None,
               fft_im=np.zeros((S, n_rows, n_fft_modes)) if n_fft_modes else None,
               tracers_unwrapped=np.zeros((S, ntr)) if ntr else None, tracer_state=np.zeros((S, ntr), np.int8) if ntr else None)
    arg.update(out, tracer_x=out["tracers_unwrapped"], tracer_s=out["tracer_state"])
    if not ntr:
        arg.update(v_eff_series=None, D_eff_series=None)           # without tracers the caller's two series stay NaN
    ms = C.c_double()
    ptrs = [_p(arg.get(k)) for k in COMMON] + [C.byref(ms)]
    entry, last_error = name, SOLVES[name].last_error
    if segment:
        entry, last_error = RESUMABLE[name]
        left = None
        if return_checkpoint:
            window = par.window
            left = PdeCheckpoint(rho_p=np.zeros((S, L)), rho_m=np.zeros((S, L)), tracer_x=np.zeros((S, ntr)) if ntr else None,
                                 tracer_s=np.zeros((S, ntr), np.int8) if ntr else None, hist=np.zeros((S, window, ntr)) if ntr else None,
                                 step=-1, model=model, seed=par.seed, betas=betas, kernel_sigmas=own if name == "pdek_solve" else None)
        c_from, c_to = (None if c is None else c.struct() for c in (resume, left))
        ptrs += [None if c is None else C.byref(c) for c in (c_from, c_to)]
    rc = SOLVES[name].call(getattr(lib, entry), C.byref(par), S, own, ptrs)
    if rc != 0:
        raise capi.ApsError(rc, getattr(lib, last_error)().decode())
    out.update(times=(first_snap + np.arange(n_snap)) * every * model["dt"] if segment else np.arange(n_snap) * every * model["dt"], kernel_ms=ms.value)
    if segment:
        out["first_row"] = first_row
        if left is not None:
            left.step = c_to.step
            out["checkpoint"] = left
    return out


def _check_steps_per_launch(steps_per_launch):
    if steps_per_launch is not None and (isinstance(steps_per_launch, bool) or not isinstance(steps_per_launch, (int, np.integer)) or steps_per_launch < 1):
        raise ValueError("steps_per_launch must be None or an integer >= 1")


def _check_resume(resume):
    if resume is not None and not isinstance(resume, PdeCheckpoint):
        raise ValueError("resume must be None or a PdeCheckpoint")


_PER_ROW = SERIES + ("fft_re", "fft_im", "snapshots", "m_snapshots", "times")


def _segments(launch, nsteps, resume, return_checkpoint, steps_per_launch, rand_u, rand_n, seed):
    """`launch(nsteps=, resume=, return_checkpoint=, rand_u=, rand_n=, seed=)` as one launch, or with steps_per_launch as a
    chain of launches of at most that many steps, each resumed from the checkpoint of the one before and merged into the dict
    of the single launch: rows and snapshots one after another, the final state of the last, kernel_ms their sum and
    kernel_ms_segments the parts.  rand_u / rand_n are cut along their row axis (the last but one)."""
    if seed is None:
        seed = resume.seed if resume is not None else 0
    if steps_per_launch is None:
        return launch(nsteps=nsteps, resume=resume, return_checkpoint=return_checkpoint, rand_u=rand_u, rand_n=rand_n, seed=seed)
    if nsteps <= steps_per_launch:                                 # a chain of one: the same keys as a longer one
        r = launch(nsteps=nsteps, resume=resume, return_checkpoint=True, rand_u=rand_u, rand_n=rand_n, seed=seed)
        r["kernel_ms_segments"] = [r["kernel_ms"]]
        if not return_checkpoint:
            del r["checkpoint"]
        return r
    parts, done, row = [], 0, 0
    while done < nsteps:
        n = min(int(steps_per_launch), nsteps - done)
        rows = n + (1 if resume is None else 0)                    # a fresh start records row 0 as well
        cut = (lambda a: None if a is None else np.asarray(a)[..., row:row + rows, :])
        parts.append(launch(nsteps=n, resume=resume, return_checkpoint=True, rand_u=cut(rand_u), rand_n=cut(rand_n), seed=seed))
        resume = parts[-1]["checkpoint"]
        done, row = done + n, row + rows
    out = dict(parts[-1])
    for k in _PER_ROW:
        if parts[0][k] is not None:
            out[k] = np.concatenate([r[k] for r in parts], axis=0 if k == "times" else 1)
    out["kernel_ms_segments"] = [r["kernel_ms"] for r in parts]
    out["kernel_ms"] = float(sum(out["kernel_ms_segments"]))
    out["first_row"] = parts[0]["first_row"]
    if not return_checkpoint:
        del out["checkpoint"]
    return out


def solve_batch_raw(*, L, xlim, dt, nsteps, gamma, lam, betas, bc, active_model, gaussian_kernel, kernel_sigma,
                    snapshot_interval, rho_p0, rho_m0, tracer_x0=None, tracer_s0=None, rand_u=None, rand_n=None,
                    n_fft_modes=0, seed=None, device=0, want_snapshots=True, workgroups=None, fft_modes=None,
                    convolution=None, resume=None, return_checkpoint=False, steps_per_launch=None):
    """All systems of `betas` from their initial states to step nsteps on the GPU; dict of arrays with a leading
    system axis.  rand_u / rand_n [n_systems, nsteps+1, n_tracers] replace the device's Philox draws (tests).
    workgroups: None = one workgroup per system (pde_solve_batch); "auto" or an integer >= 1 = the wide shape with that
    many slabs per system (pdew_solve).  fft_modes: when given, the number of lowest Fourier modes (replaces n_fft_modes).
    convolution: None / "direct" = the direct sum, "spectral" = transforms over overlap-save blocks (wide shape only).
    seed: the Philox key of the tracer noise; None = 0, or the checkpoint's on a resume.

    Segments (include/pde_resume.h).  resume: a `PdeCheckpoint`; the run goes on from it for `nsteps` FURTHER steps, rho_p0 ..
    tracer_s0 are not read (pass None), the series hold rows resume.step + 1 .. resume.step + nsteps (rand_u / rand_n: those
    rows), the snapshots those of them whose absolute number is a multiple of snapshot_interval (maybe none), `times` stays
    absolute and the result gains "first_row".  Other betas (kernel_sigma, ...) than the checkpoint's switch the parameter at
    its step; another L, xlim, dt, n_tracers or number of systems raises ValueError naming the field.
    return_checkpoint: the result gains "checkpoint", the state at the last row.  steps_per_launch=n: the call runs as a chain
    of launches of at most n steps; the merged dict equals the single launch's in every key of it, kernel_ms is the sum over
    the segments and "kernel_ms_segments" lists the parts.
    A chain, or a resumed run, has the bits of the single launch when every segment runs the same path (workgroups,
    convolution).  A checkpoint does not depend on the path: it may be resumed on another one, and the run then agrees with
    the single launch as closely as the two paths agree with each other."""
    lib = _lib()
    wg = _check_workgroups(workgroups)
    conv = _check_convolution(convolution, wg)
    fm = _check_fft_modes(fft_modes, L)
    _check_resume(resume)
    _check_steps_per_launch(steps_per_launch)
    model = _model(locals())

    def launch(nsteps, **segment):
        return _launch(lib, "pde_solve_batch" if wg is None else "pdew_solve", wg, dict(model, nsteps=nsteps), betas=betas, rho_p0=rho_p0,
                       rho_m0=rho_m0, tracer_x0=tracer_x0, tracer_s0=tracer_s0, n_fft_modes=n_fft_modes if fm is None else fm,
                       want_snapshots=want_snapshots, convolution=conv, **segment)
    return _segments(launch, nsteps, resume, return_checkpoint, steps_per_launch, rand_u, rand_n, seed)


def _sweep_axes(betas, kernel_sigmas):
    """betas and kernel_sigmas broadcast against each other -> two contiguous float64 vectors of one length."""
    b = np.atleast_1d(np.asarray(betas, dtype=np.float64))
    k = np.atleast_1d(np.asarray(kernel_sigmas, dtype=np.float64))
    if b.ndim != 1 or k.ndim != 1:
        raise ValueError("betas and kernel_sigmas must be scalars or one-dimensional")
    try:
        b, k = np.broadcast_arrays(b, k)
    except ValueError:
        raise ValueError(f"betas ({len(b)}) and kernel_sigmas ({len(k)}) do not broadcast against each other") from None
    return np.ascontiguousarray(b), np.ascontiguousarray(k)


def sweep_plan(*, L, kernel_sigmas, convolution=None, xlim=1.0, dt=5e-4, T=None, nsteps=None, gamma=2.33e-4, lam=0.6, bc="periodic",
               active_model="bidirectional", gaussian_kernel=False, snapshot_interval=50, n_tracers=0, fft_modes=0, device=0):
    """What `solve_sweep_raw` would use for these kernel widths (pdek_plan of include/pde_sweep.h; nothing is launched, no GPU
    is needed): dict with the lists kernel_mode, ktaps, conv_log2 (one entry per width; conv_log2 0 where no transform runs),
    ktaps_max, conv_log2_max, lds_bytes, fields_in_lds and convolution ("direct" | "spectral").  ApsError when a width is not
    finite and > 0 under a Gaussian kernel, or the shape is not eligible."""
    lib = _lib()
    conv = _check_convolution(convolution)
    if nsteps is None:
        nsteps = int(T / dt) if T is not None else 0
    ks = np.ascontiguousarray(np.atleast_1d(np.asarray(kernel_sigmas, dtype=np.float64)))
    if ks.ndim != 1:
        raise ValueError("kernel_sigmas must be a scalar or one-dimensional")
    mode, kt, lg = (np.zeros(len(ks), np.int32) for _ in range(3))
    info = _plan(lib, "pdek_plan", PdekPlanInfo(), dict(locals(), kernel_sigma=0.0), conv, (len(ks), _p(ks)),
                 (_p(mode), _p(kt), _p(lg)))
    info["fields_in_lds"] = bool(info["fields_in_lds"])
    return dict(kernel_mode=mode.tolist(), ktaps=kt.tolist(), conv_log2=lg.tolist(), **info)


def solve_sweep_raw(*, L, xlim, dt, nsteps, gamma, lam, betas, kernel_sigmas, bc, active_model, gaussian_kernel,
                    snapshot_interval, rho_p0, rho_m0, tracer_x0=None, tracer_s0=None, rand_u=None, rand_n=None,
                    n_fft_modes=0, seed=None, device=0, want_snapshots=True, fft_modes=None, convolution=None,
                    resume=None, return_checkpoint=False, steps_per_launch=None):
    """`solve_batch_raw` with a kernel width per system (pdek_solve of include/pde_sweep.h): `betas` and `kernel_sigmas` are
    broadcast against each other, system s runs (betas[s], kernel_sigmas[s]) on its own workgroup, all in ONE launch; the same
    dict of arrays with a leading system axis.  convolution: None / "direct" = the direct sum of `solve_batch_raw`,
    "spectral" = the Gaussian-kernel magnetisation by a transform in the workgroup's LDS (see `sweep_plan` for what is eligible).
    resume / return_checkpoint / steps_per_launch: as in `solve_batch_raw`; a resume may bring other kernel_sigmas as well as
    other betas (the checkpoint remembers the widths it was taken with)."""
    lib = _lib()
    conv = _check_convolution(convolution)
    fm = _check_fft_modes(fft_modes, L)
    betas, ks = _sweep_axes(betas, kernel_sigmas)
    _check_bc(bc)
    _check_resume(resume)
    _check_steps_per_launch(steps_per_launch)
    model = _model(dict(locals(), kernel_sigma=0.0))

    def launch(nsteps, **segment):
        return _launch(lib, "pdek_solve", ks, dict(model, nsteps=nsteps), betas=betas, rho_p0=rho_p0, rho_m0=rho_m0,
                       tracer_x0=tracer_x0, tracer_s0=tracer_s0, n_fft_modes=n_fft_modes if fm is None else fm,
                       want_snapshots=want_snapshots, convolution=conv, **segment)
    return _segments(launch, nsteps, resume, return_checkpoint, steps_per_launch, rand_u, rand_n, seed)


class IMEXPDE:
    def __init__(self, L=1000, xlim=1.0, T=10.0, dt=5e-4, gamma=2.33e-4, lam=0.6, beta=2.0, bc="periodic",
                 active_model="bidirectional", gaussian_kernel=False, kernel_sigma=0.02, snapshot_interval=50,
                 outdir="IMEX_output", seed=None,
                 # extensions (optional, after the reference's keywords)
                 device=0, record_fft=True, workgroups=None, fft_modes=None, convolution=None):
        self.L, self.xlim, self.dx = L, xlim, xlim / L
        self.x = np.linspace(0, xlim, L, endpoint=False)
        self.T, self.dt, self.nsteps = T, dt, int(T / dt)
        self.gamma, self.lam, self.beta = gamma, lam, beta
        self.bc, self.active_model = bc, active_model
        self.gaussian_kernel, self.kernel_sigma = gaussian_kernel, kernel_sigma
        self.snapshot_interval, self.seed = snapshot_interval, seed
        self.outdir = outdir                                       # kept as an attribute; nothing is written
        self.device, self.record_fft = int(device), bool(record_fft)
        if L > PDE_MAX_L:
            raise ValueError(f"L <= {PDE_MAX_L}")
        _check_workgroups(workgroups)
        _check_fft_modes(fft_modes, L)
        _check_convolution(convolution, workgroups)
        self.workgroups, self.fft_modes = workgroups, fft_modes    # None: one workgroup per system; record_fft decides the modes
        self.convolution = convolution                             # None: the direct sum
        if seed is not None:
            np.random.seed(seed)                                   # ref :55-56
        self.rho_mean = 1.0 / self.xlim
        self._out = None

    def cw_rate(self, sigma, m):                                   # ref :64-66
        return np.clip(np.exp(-self.beta * sigma * m), 1e-8, 1e8)

    def initialize(self, mode="poisson", rho0=1.0, noise=0.2, n_tracers=1000):   # ref :96-131, host side
        L = self.L
        if mode == "homogeneous":
            rho_p = rho0 + noise * np.random.randn(L)
            rho_m = rho0 + noise * np.random.randn(L)
        elif mode == "poisson":
            rho_p = np.exp(-np.abs(self.x - 0.5) / 0.05)
            rho_m = np.exp(-np.abs(self.x - 0.5) / 0.05)
            rho_p += noise * np.random.randn(L)
            rho_m += noise * np.random.randn(L)
        else:
            raise ValueError("Unknown init mode.")
        rho_p, rho_m = np.clip(rho_p, 0, None), np.clip(rho_m, 0, None)
        tot = (rho_p + rho_m).sum()
        self.rho_p, self.rho_m = rho_p / tot, rho_m / tot
        self.n_tracers = n_tracers
        self.tracers = np.random.choice(L, size=n_tracers) * self.dx
        self.tracers_unwrapped = self.tracers.copy()
        self.tracer_state = np.random.choice([-1, 1], size=n_tracers)
        self._out = None

    def _model(self, sweep=False):
        """The model record of this solver (MODEL above), as the raw solves and plan() take it; a sweep has a width per system
        in place of kernel_sigma."""
        model = _model(vars(self))
        if sweep:
            del model["kernel_sigma"]
        return model

    def _modes(self, fft_modes=None):
        """The Fourier modes of a call: given with it, else the constructor's fft_modes, else all of them under record_fft."""
        for n in (fft_modes, self.fft_modes):
            if n is not None:
                return n
        return self.L // 2 + 1 if self.record_fft else 0

    def _start(self):
        """This solver's state as the start of a launch."""
        return dict(rho_p0=self.rho_p, rho_m0=self.rho_m, tracer_x0=self.tracers_unwrapped if self.n_tracers else None,
                    tracer_s0=self.tracer_state if self.n_tracers else None)

    def _seed(self):
        """The seed of a call: the solver's, else drawn from NumPy's global generator."""
        return self.seed if self.seed is not None else int(np.random.randint(0, 2 ** 31 - 1))

    def _run(self, betas, rand_u=None, rand_n=None, want_snapshots=True, workgroups=None, fft_modes=None, convolution=None,
             note=None, **segments):
        """solve_batch_raw from this solver's state; workgroups / fft_modes / convolution override the constructor's, `segments`
        are resume / return_checkpoint / steps_per_launch.  `note`: a dict that receives what the call started from and its seed."""
        model, start = self._model(), self._start()
        seed = self._seed()
        if note is not None:
            note.update(start, seed=seed)
        return solve_batch_raw(**model, **start, seed=seed, betas=betas, rand_u=rand_u, rand_n=rand_n,
                               want_snapshots=want_snapshots, fft_modes=self._modes(fft_modes),
                               workgroups=workgroups if workgroups is not None else self.workgroups,
                               convolution=convolution if convolution is not None else self.convolution, **segments)

    def solve(self, rand_u=None, rand_n=None, keep_checkpoint=False, steps_per_launch=None):   # ref :236-290, on the GPU
        """The run to T.  A solved instance can be continued (`continue_solve`).  By default the run is the one launch of
        pde_solve_batch / pdew_solve it has always been and remembers what it started from; the first continuation then
        obtains the checkpoint by running these steps once more through the resumable entry point (no series, no snapshots).
        keep_checkpoint=True takes the checkpoint in this run itself (pder_solve / pdewr_solve), so that continuing costs the
        further steps only; steps_per_launch=n runs it as a chain of launches of at most n steps (and keeps the checkpoint)."""
        _check_steps_per_launch(steps_per_launch)
        began = {}
        keep = bool(keep_checkpoint) or steps_per_launch is not None
        r = self._run([self.beta], rand_u, rand_n, note=began, **(dict(return_checkpoint=True, steps_per_launch=steps_per_launch) if keep else {}))
        self._adopt(r, 0)
        # what continue_solve goes on from: the checkpoint, or else how to obtain it (kept in _out, with the random numbers given)
        self._out = dict(checkpoint=r.get("checkpoint"), began=began, steps=self.nsteps, rand_u=rand_u, rand_n=rand_n)
        return self

    def continue_solve(self, T, rand_u=None, rand_n=None, steps_per_launch=None):
        """Appends int(T / dt) steps to a finished `solve()` (or to an earlier continuation), bit for bit the run that was never
        cut: afterwards T, nsteps, every series, the snapshots, times, Fourier modes, fields and tracers are those of a solver
        constructed with the total T (T1 and T2 such that int(T1 / dt) + int(T2 / dt) == int((T1 + T2) / dt)); kernel_ms is
        the sum.  rand_u / rand_n [int(T / dt), n_tracers]: the rows of the further steps, needed iff solve() was given them.
        The tracer noise continues under the seed of solve().  The instance keeps the new checkpoint (`checkpoint()`)."""
        _check_steps_per_launch(steps_per_launch)
        kept = self._out
        if not isinstance(kept, dict) or "began" not in kept:
            raise RuntimeError("continue_solve: nothing to continue; call solve() first")
        more = int(T / self.dt)
        if more < 1:
            raise ValueError("continue_solve: T must cover at least one step")
        if (rand_u is None) != (kept["rand_u"] is None):
            raise ValueError("continue_solve: rand_u / rand_n must be given iff solve() was given them")
        ck, seed = self.checkpoint(), kept["began"]["seed"]
        r = solve_batch_raw(**dict(self._model(), nsteps=more), rho_p0=None, rho_m0=None, betas=[self.beta], seed=seed, rand_u=rand_u,
                            rand_n=rand_n, fft_modes=self._modes(), workgroups=self.workgroups, convolution=self.convolution,
                            resume=ck, return_checkpoint=True, steps_per_launch=steps_per_launch)
        before = {k: getattr(self, k) for k in SERIES + ("snapshots", "m_snapshots", "times", "fft_phase", "kernel_ms")}
        self._adopt(r, 0)
        for k in SERIES:
            setattr(self, k, np.concatenate([before[k], getattr(self, k)]))
        for k in ("snapshots", "m_snapshots", "times"):
            setattr(self, k, before[k] + getattr(self, k))
        if self.fft_phase is not None:
            self.fft_phase = np.concatenate([before["fft_phase"], self.fft_phase])
            self.fft_amp = np.abs(self.fft_phase)
        self.kernel_ms += before["kernel_ms"]
        self.T, self.nsteps = self.T + T, self.nsteps + more
        self._out = dict(kept, checkpoint=r["checkpoint"], steps=self.nsteps)
        return self

    def checkpoint(self):
        """The `PdeCheckpoint` (one system) at the end of the run so far; see `solve` for what it costs when solve() kept none."""
        kept = self._out
        if not isinstance(kept, dict) or "began" not in kept:
            raise RuntimeError("checkpoint: call solve() first")
        if kept["checkpoint"] is None:                             # the run once more, for its checkpoint alone
            began = kept["began"]
            r = solve_batch_raw(**dict(self._model(), nsteps=kept["steps"]), **{k: v for k, v in began.items() if k != "seed"},
                                betas=[self.beta], seed=began["seed"], rand_u=kept["rand_u"], rand_n=kept["rand_n"], fft_modes=0,
                                want_snapshots=False, workgroups=self.workgroups, convolution=self.convolution, return_checkpoint=True)
            if not (np.array_equal(r["rho_p"][0], self.rho_p) and np.array_equal(r["rho_m"][0], self.rho_m)):
                raise RuntimeError("checkpoint: the repeated run does not reproduce the solved state (was the instance changed since solve()?)")
            kept["checkpoint"] = r["checkpoint"]
        return kept["checkpoint"]

    def resume_from(self, checkpoint, steps=None):
        """Makes `checkpoint` (a one-system PdeCheckpoint, e.g. loaded from a file) the state this instance continues from, as
        if its solve() had just left it; `steps`: the steps the run has taken (default: checkpoint.step).  The series held so
        far are kept as they are."""
        _check_resume(checkpoint)
        kept = self._out if isinstance(self._out, dict) and "began" in self._out else dict(began=dict(seed=checkpoint.seed), rand_u=None, rand_n=None)
        self._out = dict(kept, checkpoint=checkpoint, steps=checkpoint.step if steps is None else steps)
        return self

    def _adopt(self, r, s):
        for name in ("rho_p", "rho_m") + SERIES:
            setattr(self, name, r[name][s])
        self.snapshots = list(r["snapshots"][s]) if r["snapshots"] is not None else []
        self.m_snapshots = list(r["m_snapshots"][s]) if r["m_snapshots"] is not None else []
        self.times = list(r["times"])
        if r["fft_re"] is not None:
            self.fft_phase = r["fft_re"][s] + 1j * r["fft_im"][s]
            self.fft_amp = np.abs(self.fft_phase)
        else:
            self.fft_phase = self.fft_amp = None
        if r["tracers_unwrapped"] is not None:
            self.tracers_unwrapped = r["tracers_unwrapped"][s]
            self.tracers = self.tracers_unwrapped % self.xlim
            self.tracer_state = r["tracer_state"][s].astype(int)
        self.kernel_ms = r["kernel_ms"]

    def plan(self, n_systems=1, convolution=None):
        """What the wide shape would use for this solver (see `plan`); with workgroups=None, what "auto" would.
        convolution given here overrides the constructor's."""
        return plan(**self._model(), workgroups=self.workgroups if self.workgroups is not None else "auto", n_systems=n_systems,
                    n_tracers=getattr(self, "n_tracers", 0), fft_modes=self._modes(),
                    convolution=convolution if convolution is not None else self.convolution)

    def solve_batch(self, betas, want_snapshots=False, workgroups=None, fft_modes=None, convolution=None, resume=None,
                    return_checkpoint=False, steps_per_launch=None):
        """The same initial condition evolved for every beta of `betas` in ONE launch (one workgroup per beta, or
        `workgroups` slabs per beta on the wide shape; independent tracer noise per system).  workgroups / fft_modes /
        convolution given here override the constructor's.  Returns the raw dict of arrays with a leading system axis.
        resume / return_checkpoint / steps_per_launch: as in `solve_batch_raw` (with resume, nsteps further steps from the
        checkpoint instead of this instance's state)."""
        _check_workgroups(workgroups)                              # what is given here is checked before the seed is drawn
        _check_fft_modes(fft_modes, self.L)
        _check_convolution(convolution, workgroups if workgroups is not None else self.workgroups)
        segments = {k: v for k, v in dict(resume=resume, return_checkpoint=return_checkpoint, steps_per_launch=steps_per_launch).items() if v}
        return self._run(betas, want_snapshots=want_snapshots, workgroups=workgroups, fft_modes=fft_modes,
                         convolution=convolution, **segments)

    def solve_sweep(self, betas=None, kernel_sigmas=None, convolution=None, want_snapshots=False, resume=None, return_checkpoint=False,
                    steps_per_launch=None):
        """This instance's initial condition evolved for every (beta, kernel_sigma) pair in ONE launch on the one-workgroup
        shape (`solve_sweep_raw`): betas and kernel_sigmas are broadcast against each other, each defaults to the instance's
        own value.  convolution: None / "direct" or "spectral" (the transform in LDS).  Returns the raw dict of arrays.
        resume / return_checkpoint / steps_per_launch: as in `solve_sweep_raw`."""
        return solve_sweep_raw(seed=self._seed(), **self._model(sweep=True), **self._start(),
                               betas=self.beta if betas is None else betas,
                               kernel_sigmas=self.kernel_sigma if kernel_sigmas is None else kernel_sigmas,
                               n_fft_modes=self._modes(), want_snapshots=want_snapshots, convolution=convolution,
                               resume=resume, return_checkpoint=return_checkpoint, steps_per_launch=steps_per_launch)

    def get_output(self):                                          # ref :293-306
        return dict(rho_p=self.rho_p, rho_m=self.rho_m, m_series=self.m_series, var_series=self.var_series,
                    fft_amp=self.fft_amp, fft_phase=self.fft_phase, snapshots=np.array(self.snapshots),
                    m_snapshots=np.array(self.m_snapshots), times=np.array(self.times),
                    v_eff_series=self.v_eff_series, D_eff_series=self.D_eff_series)

    def plot_all(self, *args, **kwargs):
        raise NotImplementedError("plot_all (matplotlib figures, reference :309-346) is presentation code outside the "
                                  "accelerated path; plot get_output() yourself")

    def plot_individual(self, *args, **kwargs):
        raise NotImplementedError("plot_individual (matplotlib figures, reference :348-461) is presentation code "
                                  "outside the accelerated path")


def sweep_over_betas(beta_values, n_runs=3, t_min=20.0, t_max=40.0, seeds=None, init_kwargs=None, workgroups=None, fft_modes=None,
                     convolution=None, steps_per_launch=None, **ctor_kwargs):
    """The reference's PDE tracer sweep (IMEX_PDE_solver_run_sweep.py:7-75) as ONE launch: every (beta, run) pair is a
    system with its own seeded initial condition.  Returns (v_mean, v_err, D_mean, D_err) per beta exactly as the
    driver forms them: v = |nanmean(v_eff_series[t_min <= t <= t_max])|, D = nanmean(D_eff_series[...]), mean over runs,
    err = std(ddof=1) / sqrt(n_runs).  workgroups selects the execution shape as in `IMEXPDE`; fft_modes > 0 adds the
    Fourier modes of every system to the work (the sweep itself does not use them); convolution as in `IMEXPDE`.
    steps_per_launch=n: the run as a chain of launches of at most n steps (`solve_batch_raw`), the same numbers."""
    init_kwargs = dict(init_kwargs or {})
    betas, rp, rm, tx, ts = [], [], [], [], []
    proto = None
    for bi, beta in enumerate(beta_values):
        for run in range(n_runs):
            seed = run if seeds is None else seeds[bi][run]         # the reference seeds each run with its run index
            s = IMEXPDE(beta=beta, seed=seed, record_fft=False, workgroups=workgroups, fft_modes=fft_modes, convolution=convolution,
                        **ctor_kwargs)
            s.initialize(**init_kwargs)
            proto = proto or s
            betas.append(float(beta)); rp.append(s.rho_p); rm.append(s.rho_m); tx.append(s.tracers_unwrapped); ts.append(s.tracer_state)
    r = solve_batch_raw(**proto._model(), betas=betas, rho_p0=np.array(rp), rho_m0=np.array(rm), tracer_x0=np.array(tx),
                        tracer_s0=np.array(ts), seed=proto.seed or 0, want_snapshots=False, workgroups=workgroups,
                        fft_modes=fft_modes, convolution=convolution, steps_per_launch=steps_per_launch)
    t = np.linspace(0, proto.T, proto.nsteps + 1)
    mask = (t >= t_min) & (t <= t_max)
    v = np.abs(np.nanmean(r["v_eff_series"][:, mask], axis=1)).reshape(len(beta_values), n_runs)
    D = np.nanmean(r["D_eff_series"][:, mask], axis=1).reshape(len(beta_values), n_runs)
    root = np.sqrt(n_runs)
    return (v.mean(axis=1), v.std(axis=1, ddof=1) / root, D.mean(axis=1), D.std(axis=1, ddof=1) / root, r["kernel_ms"])


def sweep_over_kernel_sigmas(kernel_sigma_values, n_runs=5, base_seed=100, init_kwargs=None, convolution=None, steps_per_launch=None,
                             **ctor_kwargs):
    """The reference's kernel-width sweep (IMEX_PDE_solver_run_sweep_magn.py:55-85) as ONE launch: system (k, r) is the solver
    of kernel_sigma_values[k] constructed with seed = base_seed + 1000 k + r and initialised on the host like the driver does.
    Returns a dict: each sigma -> dict of arrays [n_runs, nsteps + 1] with the four quantities the driver collects,
    m_series = |m_series|, v_eff_series = |v_eff_series|, D_eff_series, var_series; and "kernel_ms".
    The result is keyed by the sigma values themselves (the driver's `results[kernel_sigma]`) next to the one string key
    "kernel_ms", so a width given twice is refused (ValueError): its second block of runs would replace the first.
    convolution: None / "direct" or "spectral" as in `solve_sweep_raw`; steps_per_launch=n: the run as a chain of launches of at
    most n steps, the same numbers."""
    init_kwargs = dict(init_kwargs or {})
    kernel_sigma_values = list(kernel_sigma_values)
    if len(set(float(v) for v in kernel_sigma_values)) != len(kernel_sigma_values):
        raise ValueError(f"kernel_sigma_values holds a width twice ({kernel_sigma_values}): the result is keyed by the width")
    if not kernel_sigma_values or n_runs < 1:
        raise ValueError("sweep_over_kernel_sigmas needs at least one width and n_runs >= 1")
    ctor_kwargs.setdefault("gaussian_kernel", True)                # ref :68
    sig, rp, rm, tx, ts = [], [], [], [], []
    proto = None
    for k, sigma in enumerate(kernel_sigma_values):
        for run in range(n_runs):
            s = IMEXPDE(kernel_sigma=sigma, seed=base_seed + 1000 * k + run, record_fft=False, **ctor_kwargs)
            s.initialize(**init_kwargs)
            if proto is None:
                proto = s
            sig.append(float(sigma)); rp.append(s.rho_p); rm.append(s.rho_m); tx.append(s.tracers_unwrapped); ts.append(s.tracer_state)
    ntr = proto.n_tracers
    r = solve_sweep_raw(**proto._model(sweep=True), betas=proto.beta, kernel_sigmas=sig, rho_p0=np.array(rp), rho_m0=np.array(rm),
                        tracer_x0=np.array(tx) if ntr else None, tracer_s0=np.array(ts) if ntr else None, seed=proto.seed or 0,
                        want_snapshots=False, convolution=convolution, steps_per_launch=steps_per_launch)
    out = {}
    for k, sigma in enumerate(kernel_sigma_values):
        rows = slice(k * n_runs, (k + 1) * n_runs)
        m, var, v, D = (r[name][rows] for name in SERIES)
        out[sigma] = dict(m_series=np.abs(m), v_eff_series=np.abs(v), D_eff_series=D, var_series=var)
    out["kernel_ms"] = r["kernel_ms"]
    return out
