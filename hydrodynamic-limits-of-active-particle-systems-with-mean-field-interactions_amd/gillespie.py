"""Device-resident exact Gillespie loop for batches of systems (include/gillespie.h; systems beyond one workgroup's LDS:
include/gillespie_many.h): the reference's `ParticleSystem.run` as written (one event per iteration,
PARTICLE_solver_CLASS.py:450-558), one persistent workgroup per system.  `run_batched_exact` returns the reference's
result dictionaries; `sweep` statistics can be taken from the scalar sums without the M x L arrays (`scalars_only=True`),
and the structure observables from sums the loop takes at every observation (`run_batched_exact_structure`,
include/gillespie_structure.h); the anchor-capture study's cluster, lifetime and exit statistics likewise
(`run_batched_exact_capture`, include/gillespie_capture.h); the ensemble density and field profiles of many runs
(`run_batched_exact_profiles`, include/gillespie_profile.h) are summed over the runs on the device.  Systems that differ in
the interaction range or in the blocking threshold of their particle number share ONE launch as a mixed batch
(`run_batched_exact_mixed`, `run_batched_exact_statistics_mixed`, include/gillespie_mixed.h; with `allow_large=True` also systems
beyond one workgroup's LDS, include/gillespie_mixed_many.h); the structure observables of such a batch come from sums the
mixed launch takes and reduces over the window on the device (`run_batched_exact_structure_mixed`,
include/gillespie_mixed_structure.h), and its ensemble profiles from sums the mixed launch adds per group, in either shape
(`run_batched_exact_profiles_mixed`, include/gillespie_mixed_profile.h).  A run may be cut into segments and resumed bit for bit (`Checkpoint`,
include/gillespie_resume.h), a mixed batch too (`MixedCheckpoint`, include/gillespie_mixed_resume.h).

Differences to the reference: randomness is Philox4x32-10 keyed by `seed` (the reference consumes a NumPy Generator), so
trajectories agree in distribution, not draw for draw; `m_local_list[k]` is the field of the observed state (the
reference stores the field from before the last event).  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import json
import types

import numpy as np

from . import capi

GIL_MAX_L, GIL_MAX_N, NSCALARS = 4096, 2048, 12
SCALARS = ("n", "sum_sigma", "sum_pos", "n_wall", "max_pos", "n_front", "attempts", "blocked", "sum_d", "sum_d2", "n_d", "events")


class GilParams(C.Structure):
    """struct gil_params of include/gillespie.h, field for field."""
    _fields_ = [("L", C.c_int32), ("K", C.c_int32), ("periodic", C.c_int32), ("minus_anchor", C.c_int32),
                ("immobilize", C.c_int32), ("suppress_flip", C.c_int32), ("crowding", C.c_int32), ("n_systems", C.c_int32),
                ("n_cap", C.c_int32), ("n_obs", C.c_int32), ("device", C.c_int32), ("x_wall", C.c_int32),
                ("ref_obs", C.c_int32), ("flip_n", C.c_int32), ("sigma_grid", C.c_double), ("rate_diffusion", C.c_double),
                ("rate_active", C.c_double), ("k_on", C.c_double), ("k_off", C.c_double), ("k_exit", C.c_double),
                ("T", C.c_double), ("seed", C.c_uint64), ("max_events", C.c_int64), ("beta", C.c_void_p),
                ("anchor_mask", C.c_void_p), ("times_obs", C.c_void_p), ("front_lo", C.c_void_p), ("block_table", C.c_void_p),
                ("flip_table", C.c_void_p)]


class GilmPlanInfo(C.Structure):
    """struct gilm_plan_info of include/gillespie_many.h, field for field."""
    _fields_ = [("n_systems", C.c_int32), ("n_blocks", C.c_int32), ("table_len", C.c_int32), ("table_in_lds", C.c_int32),
                ("lds_bytes", C.c_int32), ("reserved", C.c_int32), ("work_bytes_per_system", C.c_int64), ("output_bytes", C.c_int64)]


class GilsPlanInfo(C.Structure):
    """struct gils_plan_info of include/gillespie_structure.h, field for field."""
    _fields_ = [("shape", C.c_int32), ("threads", C.c_int32), ("lds_bytes", C.c_int32), ("row_len", C.c_int32),
                ("phase_in_lds", C.c_int32), ("reserved", C.c_int32), ("work_bytes", C.c_int64), ("output_bytes", C.c_int64)]


class GilcPlanInfo(C.Structure):
    """struct gilc_plan_info of include/gillespie_capture.h, field for field."""
    _fields_ = [("shape", C.c_int32), ("threads", C.c_int32), ("lds_bytes", C.c_int32), ("row_len", C.c_int32),
                ("work_bytes", C.c_int64), ("output_bytes", C.c_int64)]


class GilpPlanInfo(C.Structure):
    """struct gilp_plan_info of include/gillespie_profile.h, field for field."""
    _fields_ = [("shape", C.c_int32), ("threads", C.c_int32), ("lds_bytes", C.c_int32), ("bin_width", C.c_int32),
                ("n_bins_used", C.c_int32), ("reserved", C.c_int32), ("work_bytes", C.c_int64), ("output_bytes", C.c_int64)]


class GilxVariants(C.Structure):
    """struct gilx_variants of include/gillespie_mixed.h, field for field."""
    _fields_ = [("n_variants", C.c_int32), ("reserved", C.c_int32), ("sigma_grid", C.c_void_p), ("block_table", C.c_void_p),
                ("variant_of_system", C.c_void_p), ("seed", C.c_void_p), ("stream", C.c_void_p), ("order", C.c_void_p)]


class GilxPlanInfo(C.Structure):
    """struct gilx_plan_info of include/gillespie_mixed.h, field for field."""
    _fields_ = [("threads", C.c_int32), ("lds_bytes", C.c_int32), ("max_tlen", C.c_int32), ("systems_per_cu", C.c_int32),
                ("table_doubles", C.c_int64), ("output_bytes", C.c_int64)]


class GilxmPlanInfo(C.Structure):
    """struct gilxm_plan_info of include/gillespie_mixed_many.h, field for field."""
    _fields_ = [("n_systems", C.c_int32), ("n_blocks", C.c_int32), ("max_tlen", C.c_int32), ("max_tlen_lds", C.c_int32),
                ("n_global", C.c_int32), ("lds_bytes", C.c_int32), ("table_doubles", C.c_int64), ("work_bytes_per_system", C.c_int64),
                ("output_bytes", C.c_int64)]


class GilxpPlanInfo(C.Structure):
    """struct gilxp_plan_info of include/gillespie_mixed_profile.h, field for field."""
    _fields_ = [("shape", C.c_int32), ("threads", C.c_int32), ("lds_bytes", C.c_int32), ("max_tlen", C.c_int32),
                ("bin_width", C.c_int32), ("n_bins_used", C.c_int32), ("table_doubles", C.c_int64), ("work_bytes", C.c_int64),
                ("output_bytes", C.c_int64)]


class GilCheckpoint(C.Structure):
    """struct gil_checkpoint of include/gillespie_resume.h, field for field."""
    _fields_ = [("pos", C.c_void_p), ("flags", C.c_void_p), ("ref", C.c_void_p), ("t", C.c_void_p), ("n_events", C.c_void_p),
                ("next_obs", C.c_void_p)]


class GilxCheckpoint(C.Structure):
    """struct gilx_checkpoint of include/gillespie_mixed_resume.h, field for field."""
    _fields_ = [("base", GilCheckpoint), ("n_slots", C.c_void_p), ("window", C.c_void_p), ("n_window", C.c_void_p), ("n_empty", C.c_void_p)]


GILR_PLUS, GILR_BOUND, GILR_ALIVE = 1, 2, 4     # bits of a checkpoint's flags
GILX_MAX_VARIANTS = 4096
GILX_LDS_LIMIT = 160 * 1024     # bytes of LDS a workgroup can have: what a mixed launch must fit
GILP_NCOLS, GILP_MAX_BINS, GILP_MAX_GROUPS = 7, 1024, 4096
PROFILE_COLUMNS = ("n_plus", "n_minus", "n_bound", "n_plus2", "n_minus2", "n_plus_minus", "field")
GILC_NFIXED = 9
CAPTURE_COLUMNS = ("n", "n_bound", "binds", "unbinds", "exits", "occupied_sites", "n_clusters", "largest_cluster", "sum_size2")


_I32, _DBL, _PTR, _MS = C.c_int32, C.c_double, C.c_void_p, C.POINTER(C.c_double)
_PAR, _VAR, _CKP, _XCKP = C.POINTER(GilParams), C.POINTER(GilxVariants), C.POINTER(GilCheckpoint), C.POINTER(GilxCheckpoint)
N_COMMON = 14       # n0, pos0, sigma0, bound0, uniforms; pos, sigma, flags, scalars, n_recorded, n_events, t_final, exits, n_exits
CHECKPOINT_ARRAYS = (("pos", np.int32, 2), ("flags", np.uint8, 2), ("ref", np.int32, 2), ("t", np.float64, 1), ("n_events", np.int64, 1),
                     ("next_obs", np.int32, 1))
_WINDOW_ARRAYS = (("window", np.float64), ("n_window", np.int32), ("n_empty", np.int32))       # of a mixed structure run


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- the entry points.  One launch is  entry(gil_params *, front..., the 14 common pointers, behind..., double *kernel_ms, tail...);
# a row of ENTRIES says what an entry point puts around the common part, and its stage function makes those arguments for a call
# `c` (the numbers of _run_batch_entry: S, M, ncap, L, K, the checkpoint's arrays `ck_in`, the common output arrays `results`)
# from the keywords it names, out of all the extra keywords of _run_batch_entry, and names the outputs it adds to the dictionary.
# An array whose bare address goes into a structure is appended to c.keep: c outlives the call.

def _stage_plain(c, **_):
    return [], [], [], {}


def _stage_checkpoints(c, obs_first, kk=None):
    """The tail of a segment -- obs_first, the checkpoint to start from (NULL: a fresh start) and the one to fill -- and what it adds
    to the dictionary: the latter's arrays and the first row of every system.  `kk=None`: a gil_checkpoint; otherwise a
    gilx_checkpoint, with n_slots and, for kk > 0, the window sums of kk modes.  c.ck_in holds the six arrays of the caller's
    checkpoint, c.ck_more what it has beyond them."""
    more = {}
    if kk is not None:
        more = dict(n_slots=(np.int32, (c.S,)))
        if kk > 0:
            more.update({k: (dt, (c.S, kk, 3) if k == "window" else (c.S,)) for k, dt in _WINDOW_ARRAYS})
    ck_out = {k: np.zeros((c.S, c.ncap)[:nd], dt) for k, dt, nd in CHECKPOINT_ARRAYS}
    ck_out.update({k: np.zeros(shape, dt) for k, (dt, shape) in more.items()})
    arrays, first_row = None, np.zeros(c.S, np.int32)
    if c.ck_in is not None:
        arrays = dict(c.ck_in)
        for k, (dt, shape) in more.items():
            if c.ck_more.get(k) is None:
                continue                                       # a missing array is the library's to refuse
            arrays[k] = np.ascontiguousarray(c.ck_more[k], dtype=dt)
            if arrays[k].shape != shape:
                raise ValueError(f"checkpoint: {k} must have the shape {shape}")
        c.keep.append(arrays)
        # a system that ended before this segment starts at row 0, and its n_recorded is 0 too.  This reads the checkpoint to start
        # from only, which the library does not write (const in gillespie_resume.h)
        first_row = np.clip(c.ck_in["next_obs"] - int(obs_first), 0, None).astype(np.int32)

    def struct(a):
        base = GilCheckpoint(**{k: _p(a[k]).value for k, _, _ in CHECKPOINT_ARRAYS})
        return base if kk is None else GilxCheckpoint(base=base, **{k: _p(a[k]).value for k in more if a.get(k) is not None})

    c_in, c_out = None if arrays is None else struct(arrays), struct(ck_out)
    n0 = np.full(c.S, c.ncap, np.int32) if kk is None else ck_out["n_slots"]     # a plain checkpoint: any slot may be alive
    return [int(obs_first), None if c_in is None else C.byref(c_in), C.byref(c_out)], dict(checkpoint=ck_out, first_row=first_row,
                                                                                          obs_first=int(obs_first), n0=n0)


def _stage_resumable(c, *, obs_first, **_):
    """obs_first, the checkpoint to start from and the one to fill, behind kernel_ms"""
    return ([], [], *_stage_checkpoints(c, obs_first))


def _stage_structure(c, *, k_max, first_obs, **_):
    rows = np.zeros((c.S, c.M, 4 + 2 * max(int(k_max), 0)))
    return [int(k_max), int(first_obs)], [_p(rows)], [], dict(structure=rows)


def _stage_capture(c, *, group_of_site, n_groups, c_bins, h_bins, h_dt, first_obs, **_):
    groups = None if group_of_site is None else np.ascontiguousarray(group_of_site, dtype=np.int32)
    if groups is not None and groups.shape != (c.L,):
        raise ValueError("group_of_site must have one entry per site")
    capture = np.zeros((c.S, c.M, GILC_NFIXED + max(int(n_groups), 0) + max(int(c_bins), 0)), np.int64)
    life_hist, life_sums = np.zeros((c.S, 2, max(int(h_bins), 1)), np.int64), np.zeros((c.S, 2, 2))
    return ([_p(groups), int(n_groups), int(c_bins), int(h_bins), float(h_dt), int(first_obs)], [_p(capture), _p(life_hist), _p(life_sums)],
            [], dict(capture=capture, life_hist=life_hist, life_sums=life_sums))


def _stage_profiles(c, *, n_bins, first_obs, want_field, group_of_system, n_groups, per_system, **_):
    groups = None if group_of_system is None else np.ascontiguousarray(group_of_system, dtype=np.int32)
    if groups is not None and groups.shape != (c.S,):
        raise ValueError("group_of_system must have one entry per system")
    G, B = max(int(n_groups), 1), max(int(n_bins), 1)                     # a number below 1 is the library's to refuse
    sums, members = np.zeros((G, c.M, GILP_NCOLS, B), np.int64), np.zeros((G, c.M), np.int32)
    prof = np.zeros((c.S, c.M, 3, B), np.int32) if per_system else None
    return ([int(n_bins), int(first_obs), int(want_field), _p(groups), int(n_groups)], [_p(sums), _p(members), _p(prof)], [],
            dict(ensemble_sums=sums, members=members, profile_obs=prof))


def _profile_bins(c, *, n_bins, **_):
    """What a finished gilp_run adds behind its outputs (the library has accepted n_bins by then)."""
    width = -(-int(c.L) // int(n_bins))
    return dict(bin_width=width, n_bins_used=-(-int(c.L) // width))


def _stage_mixed(c, *, mixed, **_):
    desc, keep = _mixed_descriptor(c.S, int(c.K), **mixed)
    if desc.variant_of_system is None:
        raise ValueError("variant_of_system must have one entry per system")
    c.keep.append(keep)
    return [C.byref(desc)], [], [], {}


def _stage_mixed_profiles(c, *, mixed, n_bins, first_obs, want_field, group_of_system, n_groups, per_system, **_):
    """the variants in front of gilp_run's five numbers; its three outputs behind the common ones"""
    front = _stage_mixed(c, mixed=mixed)[0]
    numbers, behind, tail, extra = _stage_profiles(c, n_bins=n_bins, first_obs=first_obs, want_field=want_field, group_of_system=group_of_system,
                                                   n_groups=n_groups, per_system=per_system)
    return front + numbers, behind, tail, extra


def _stage_rows_and_head(c, k_max, first_obs, want_rows, sums):
    """What gilxs_run and gilxsr_run share: k_max and first_obs behind the variants, the rows (`want_rows`) and the head behind the
    common outputs; `sums` = the arrays of the window sums, which the two hand over differently."""
    rows = np.zeros((c.S, c.M, 4 + 2 * max(int(k_max), 0))) if want_rows else None
    head = np.zeros((c.S, c.M, 4))
    back = c.results + [rows, head] + list(sums.values())
    return ([int(k_max), int(first_obs)], [_p(rows), _p(head)],
            dict(sums, structure=rows, head=head, bytes_back=int(sum(x.nbytes for x in back if x is not None))))


def _stage_mixed_structure(c, *, mixed, k_max, first_obs, want_rows, **_):
    """the window sums are three more outputs behind the head"""
    front = _stage_mixed(c, mixed=mixed)[0]
    kk = max(int(k_max), 0)                                    # gilxs_run refuses k_max < 1
    sums = {k: np.zeros((c.S, kk, 3) if k == "window" else c.S, dt) for k, dt in _WINDOW_ARRAYS}
    numbers, behind, extra = _stage_rows_and_head(c, k_max, first_obs, want_rows, sums)
    return front + numbers, behind + [_p(a) for a in sums.values()], [], extra


def _stage_mixed_resumable(c, *, mixed, obs_first, **_):
    """the variants in front; obs_first, the checkpoint to start from and the one to fill behind kernel_ms"""
    front = _stage_mixed(c, mixed=mixed)[0]
    return (front, [], *_stage_checkpoints(c, obs_first, 0))


def _stage_mixed_structure_resumable(c, *, mixed, k_max, first_obs, want_rows, obs_first, **_):
    """_stage_mixed_structure where the window sums travel in the checkpoints"""
    front = _stage_mixed(c, mixed=mixed)[0]
    tail, extra = _stage_checkpoints(c, obs_first, max(int(k_max), 0))
    numbers, behind, more = _stage_rows_and_head(c, k_max, first_obs, want_rows, {k: extra["checkpoint"].get(k) for k, _ in _WINDOW_ARRAYS})
    return front + numbers, behind, tail, dict(more, **extra)


def _stage_profiles_resumable(c, *, obs_first, **profile):
    """_stage_profiles (first_obs ABSOLUTE on the run's grid) with a segment's tail and a gil_checkpoint"""
    numbers, behind, _, extra = _stage_profiles(c, **profile)
    tail, more = _stage_checkpoints(c, obs_first)
    return numbers, behind, tail, dict(extra, **more)


def _stage_mixed_profiles_resumable(c, *, obs_first, **profile):
    """_stage_mixed_profiles likewise, with a gilx_checkpoint that has n_slots and no window sums"""
    front, behind, _, extra = _stage_mixed_profiles(c, **profile)
    tail, more = _stage_checkpoints(c, obs_first, 0)
    return front, behind, tail, dict(extra, **more)


class _Entry:
    """last_error; the C types in `front` of the common pointers, `behind` them and, after kernel_ms, in the `tail`; `stage`;
    `header`: named by the error of a call that finds the entry point missing in the loaded library; `finish`: like `stage`, what a
    call that returned 0 adds to the dictionary last."""

    def __init__(self, last_error, stage=_stage_plain, front=(), behind=(), tail=(), header=None, finish=None):
        self.last_error, self.stage, self.front, self.behind, self.tail = last_error, stage, list(front), list(behind), list(tail)
        self.header, self.finish = header, finish


_RESUMABLE = dict(stage=_stage_resumable, tail=[_I32, _CKP, _CKP], header="include/gillespie_resume.h")
ENTRIES = {
    "gil_run_batch": _Entry("gil_last_error"),                     # systems in LDS
    "gilm_run": _Entry("gilm_last_error"),                         # large systems
    "gilr_run": _Entry("gilr_last_error", **_RESUMABLE),           # one segment of a run, systems in LDS
    "gilrm_run": _Entry("gilr_last_error", **_RESUMABLE),          # the same, large systems
    "gils_run": _Entry("gils_last_error", _stage_structure, [_I32, _I32], [_PTR]),
    "gilc_run": _Entry("gilc_last_error", _stage_capture, [_PTR, _I32, _I32, _I32, _DBL, _I32], [_PTR] * 3),
    "gilp_run": _Entry("gilp_last_error", _stage_profiles, [_I32, _I32, _I32, _PTR, _I32], [_PTR] * 3, finish=_profile_bins),
    "gilx_run": _Entry("gilx_last_error", _stage_mixed, [_VAR]),   # a variant per system
    "gilxs_run": _Entry("gilxs_last_error", _stage_mixed_structure, [_VAR, _I32, _I32], [_PTR] * 5),
    "gilxm_run": _Entry("gilxm_last_error", _stage_mixed, [_VAR], header="include/gillespie_mixed_many.h"),   # the same, large systems
    "gilxp_run": _Entry("gilxp_last_error", _stage_mixed_profiles, [_VAR, _I32, _I32, _I32, _PTR, _I32], [_PTR] * 3,
                        header="include/gillespie_mixed_profile.h", finish=_profile_bins),   # a variant per system and the profiles, either shape
    # one segment of a mixed run: systems in LDS, large systems, systems in LDS with the structure sums
    "gilxr_run": _Entry("gilxr_last_error", _stage_mixed_resumable, [_VAR], tail=[_I32, _XCKP, _XCKP], header="include/gillespie_mixed_resume.h"),
    "gilxmr_run": _Entry("gilxr_last_error", _stage_mixed_resumable, [_VAR], tail=[_I32, _XCKP, _XCKP], header="include/gillespie_mixed_resume.h"),
    "gilxsr_run": _Entry("gilxr_last_error", _stage_mixed_structure_resumable, [_VAR, _I32, _I32], [_PTR] * 2, [_I32, _XCKP, _XCKP],
                         header="include/gillespie_mixed_resume.h"),
    # one segment of a profile run, unmixed and mixed, either shape (the library picks it as for the one launch)
    "gilpr_run": _Entry("gilpr_last_error", _stage_profiles_resumable, [_I32, _I32, _I32, _PTR, _I32], [_PTR] * 3, [_I32, _CKP, _CKP],
                        header="include/gillespie_profile_resume.h", finish=_profile_bins),
    "gilxpr_run": _Entry("gilpr_last_error", _stage_mixed_profiles_resumable, [_VAR, _I32, _I32, _I32, _PTR, _I32], [_PTR] * 3,
                         [_I32, _XCKP, _XCKP], header="include/gillespie_profile_resume.h", finish=_profile_bins),
}
# the plans: name -> (last_error, the C types between gil_params and the info structure, the info structure)
PLANS = {
    "gilm_plan": ("gilm_last_error", [_I32, _I32], GilmPlanInfo),
    "gils_plan": ("gils_last_error", [_I32, _I32, _I32], GilsPlanInfo),
    "gilc_plan": ("gilc_last_error", [_I32] * 5, GilcPlanInfo),
    "gilp_plan": ("gilp_last_error", [_I32] * 6, GilpPlanInfo),
    "gilx_plan": ("gilx_last_error", [_VAR, _I32], GilxPlanInfo),
    "gilxs_plan": ("gilxs_last_error", [_VAR, _I32, _I32, _I32, _I32], capi.GilxsPlanInfo),
    "gilxm_plan": ("gilxm_last_error", [_VAR, _I32], GilxmPlanInfo),
    "gilxp_plan": ("gilxp_last_error", [_VAR] + [_I32] * 6, GilxpPlanInfo),
}
# an older build named by APS_LIB (a timing yardstick) may lack any entry point but these
EVERY_BUILD = ("gil_run_batch", "gil_run_large", "gilm_run", "gilm_plan", "gils_run", "gils_plan")


def _lib():
    lib = capi.load()
    if not getattr(lib, "_gil_ready", False):
        protos = {"gil_run_large": ("gil_large_last_error", [_PAR, _I32] + [_PTR] * 12 + [_MS])}
        for name, e in ENTRIES.items():
            protos[name] = (e.last_error, [_PAR] + e.front + [_PTR] * N_COMMON + e.behind + [_MS] + e.tail)
        for name, (last_error, middle, info) in PLANS.items():
            protos[name] = (last_error, [_PAR] + middle + [C.POINTER(info)])
        for name, (last_error, argtypes) in protos.items():
            if name not in EVERY_BUILD and not hasattr(lib, name):
                continue
            getattr(lib, name).restype, getattr(lib, name).argtypes = C.c_int, argtypes
            getattr(lib, last_error).restype, getattr(lib, last_error).argtypes = C.c_char_p, []
        lib._gil_ready = True
    return lib


def _params(*, L, K, periodic, n_systems, n_cap, n_obs, sigma_grid=0.0, minus_anchor=False, immobilize=False, suppress_flip=False,
            crowding=False, device=0, x_wall=0, ref_obs=0, rate_diffusion=0.0, rate_active=0.0, k_on=0.0, k_off=0.0, k_exit=0.0, T=0.0,
            seed=0, max_events=0, beta=None, times_obs=None, anchor_mask=None, front_lo=None, block_table=None, flip_table=None):
    """struct gil_params for a launch or a plan (a plan reads the shape alone), and the arrays it points to (keep them alive for the
    call).  `beta` and `times_obs` are float64 arrays already; the tables are converted here."""
    mask = None if anchor_mask is None or not np.any(anchor_mask) else np.ascontiguousarray(anchor_mask, dtype=np.uint8)
    flo = None if front_lo is None else np.ascontiguousarray(front_lo, dtype=np.int32)
    btab = None if block_table is None else np.ascontiguousarray(block_table, dtype=np.uint8)
    ftab = None if flip_table is None else np.ascontiguousarray(flip_table, dtype=np.float64)      # [2][n + 1] (aps_set_flip_table)
    keep = [beta, times_obs, mask, flo, btab, ftab]
    address = [None if a is None else _p(a).value for a in keep]
    par = GilParams(flip_n=0 if ftab is None else ftab.shape[1] - 1, L=L, K=K, periodic=int(bool(periodic)), minus_anchor=int(bool(minus_anchor)),
                    immobilize=int(bool(immobilize)), suppress_flip=int(bool(suppress_flip)), crowding=int(bool(crowding)), n_systems=n_systems,
                    n_cap=n_cap, n_obs=n_obs, device=device, x_wall=int(x_wall), ref_obs=int(ref_obs), sigma_grid=float(sigma_grid),
                    rate_diffusion=float(rate_diffusion), rate_active=float(rate_active), k_on=float(k_on), k_off=float(k_off),
                    k_exit=float(k_exit), T=float(T), seed=int(seed) & (2 ** 64 - 1), max_events=int(max_events), beta=address[0],
                    times_obs=address[1], anchor_mask=address[2], front_lo=address[3], block_table=address[4], flip_table=address[5])
    return par, keep


def _plan(name, shape, numbers, variants=None):
    """The one body of the plan_* functions: `shape` = the keywords of _params, `numbers` = the integers behind gil_params,
    `variants` = the keywords of _mixed_descriptor for the plans of a mixed launch."""
    lib = _lib()
    last_error, _, info_type = PLANS[name]
    par, keep = _params(**shape)                               # both `keep` lists live until this function returns
    front = []
    if variants is not None:
        desc, keep_variants = _mixed_descriptor(int(shape["n_systems"]), int(shape["K"]), **variants)
        front = [C.byref(desc)]
    info = info_type()
    rc = getattr(lib, name)(C.byref(par), *front, *numbers, C.byref(info))
    if rc != 0:
        raise capi.ApsError(rc, getattr(lib, last_error)().decode())
    return {k: int(getattr(info, k)) for k, _ in info_type._fields_ if k != "reserved"}


def run_raw(*, L, K, periodic, sigma_grid, rate_diffusion, rate_active, betas, states, times_obs, T, seed=0,
            minus_anchor=True, immobilize=True, suppress_flip=True, crowding=False, k_on=0.0, k_off=0.0, k_exit=0.0,
            anchor_mask=None, uniforms=None, max_events=None, want_states=True, x_wall=0, ref_obs=-1, front_lo=None,
            block_table=None, device=0, flip_table=None, n_cap=None):
    """`states` = list of (pos, sigma[, bound]) per system.  Returns a dict of arrays with a leading system axis.  `n_cap`:
    particle slots per system, where more than the largest initial state are wanted (the spare ones stay empty; more than 1024
    put a system on four wavefronts)."""
    return _run_batch_entry("gil_run_batch", **locals())       # first statement: locals() are the keywords


def run_many_large_raw(*, L, K, periodic, sigma_grid, rate_diffusion, rate_active, betas, states, times_obs, T, seed=0,
                       minus_anchor=True, immobilize=True, suppress_flip=True, crowding=False, k_on=0.0, k_off=0.0, k_exit=0.0,
                       anchor_mask=None, uniforms=None, max_events=None, want_states=True, x_wall=0, ref_obs=-1, front_lo=None,
                       block_table=None, device=0, flip_table=None, n_cap=None):
    """`run_raw` for systems beyond one workgroup's LDS (gilm_run of include/gillespie_many.h): the large-system kernel, one
    workgroup per system, all systems in one launch.  Same keywords, same dictionary, scalars included.  System s draws
    with Philox key seed + s: it is the `run_large_raw` run with that seed.  `n_cap`: particle slots per system, where more
    than the largest initial state are wanted (the spare ones stay empty)."""
    return _run_batch_entry("gilm_run", **locals())


def run_resumable_raw(*, L, K, periodic, sigma_grid, rate_diffusion, rate_active, betas, states, times_obs, T, seed=0,
                      minus_anchor=True, immobilize=True, suppress_flip=True, crowding=False, k_on=0.0, k_off=0.0, k_exit=0.0,
                      anchor_mask=None, uniforms=None, max_events=None, want_states=True, x_wall=0, ref_obs=-1, front_lo=None,
                      block_table=None, device=0, flip_table=None, n_cap=None, large=False, obs_first=0, checkpoint=None):
    """`run_raw` (large=True: `run_many_large_raw`) as one SEGMENT of a run (gilr_run / gilrm_run of include/gillespie_resume.h).
    `times_obs` holds the absolute times of the observations obs_first, obs_first + 1, ... of the run's grid; `checkpoint` is
    the dictionary of arrays (pos, flags, ref, t, n_events, next_obs) a previous segment returned under "checkpoint", or None
    for a fresh start from `states` (which is not read otherwise).  `uniforms` and `max_events` count events from the run's
    start; `ref_obs` counts within this segment; `T` is the run's.  The result also has "checkpoint" (the end state) and
    "first_row" (per system: the first row of this segment that is its own)."""
    kw = dict(locals())                                        # first statement: locals() are the keywords
    return _run_batch_entry("gilrm_run" if kw.pop("large") else "gilr_run", **kw)


def plan_many_large(*, L, K, periodic, sigma_grid, n_systems, n_cap, n_obs, want_states=True, want_scalars=True):
    """gilm_plan: what a batch of large systems would use (blocks, table, LDS, bytes), by host arithmetic; no device needed."""
    return _plan("gilm_plan", dict(L=L, K=K, periodic=periodic, sigma_grid=sigma_grid, n_systems=n_systems, n_cap=n_cap, n_obs=n_obs),
                 [int(bool(want_states)), int(bool(want_scalars))])


def run_structure_raw(*, L, K, periodic, sigma_grid, rate_diffusion, rate_active, betas, states, times_obs, T, seed=0,
                      minus_anchor=True, immobilize=True, suppress_flip=True, crowding=False, k_on=0.0, k_off=0.0, k_exit=0.0,
                      anchor_mask=None, uniforms=None, max_events=None, want_states=True, x_wall=0, ref_obs=-1, front_lo=None,
                      block_table=None, device=0, flip_table=None, k_max=None, first_obs=0, n_cap=None):
    """`run_raw` with the structure sums of every observation from `first_obs` on taken inside the event loop (gils_run of
    include/gillespie_structure.h).  The library picks the kernel: systems that fit a workgroup's LDS run as in `run_raw`,
    larger ones as in `run_many_large_raw` (system s: Philox key seed + s).  The dictionary of `run_raw` plus
    `structure` [systems][observations][4 + 2 k_max]: n, sum occ^2, sum m, sum m^2, then Re, Im of the first k_max Fourier sums
    of the site histogram -- the arguments of observables.DeviceStructure.add.  `k_max=None`: all L modes (at most 4096).
    `n_cap`: particle slots per system, as in `run_capture_raw`."""
    k_max = min(int(L), 4096) if k_max is None else int(k_max)
    return _run_batch_entry("gils_run", **locals())


def plan_structure(*, L, K, periodic, sigma_grid, n_systems, n_cap, n_obs, k_max, first_obs=0, want_states=True):
    """gils_plan: which kernel `run_structure_raw` would use (shape 0: systems in LDS, 1: large systems), its threads per system,
    LDS, work and output bytes, by host arithmetic; no device needed.  Refuses what the run would refuse on these numbers."""
    return _plan("gils_plan", dict(L=L, K=K, periodic=periodic, sigma_grid=sigma_grid, n_systems=n_systems, n_cap=n_cap, n_obs=n_obs),
                 [int(k_max), int(first_obs), int(bool(want_states))])


def run_capture_raw(*, L, K, periodic, sigma_grid, rate_diffusion, rate_active, betas, states, times_obs, T, seed=0,
                    minus_anchor=True, immobilize=True, suppress_flip=True, crowding=False, k_on=0.0, k_off=0.0, k_exit=0.0,
                    anchor_mask=None, uniforms=None, max_events=None, want_states=True, x_wall=0, ref_obs=-1, front_lo=None,
                    block_table=None, device=0, flip_table=None, group_of_site=None, c_bins=16, h_bins=40, h_dt=None, first_obs=0,
                    n_groups=None, n_cap=None):
    """`run_raw` with the anchor-capture and cluster statistics taken inside the event loop (gilc_run of
    include/gillespie_capture.h); the library picks the kernel as for `run_structure_raw`.  `group_of_site` [L]: the anchor group
    of a site or -1 (observables.anchor_groups), None: no groups; `n_groups=None`: the largest id + 1.  `h_dt=None`: T / h_bins.
    `n_cap`: particle slots per system, where more than the largest initial state are wanted (more than 2048 select the
    large-system kernel).
    The dictionary of `run_raw` plus
      `capture`   [systems][observations][9 + n_groups + c_bins] int64: CAPTURE_COLUMNS, exits per group, clusters per size;
      `life_hist` [systems][2][h_bins] int64 and `life_sums` [systems][2][2] (sum, sum of squares): lifetimes of bound states
                  ended by unbinding (0) and by exit (1), resolved to the event."""
    if n_groups is None:
        n_groups = 0 if group_of_site is None else int(max(-1, np.max(group_of_site))) + 1
    h_dt = float(T) / int(h_bins) if h_dt is None else float(h_dt)
    return _run_batch_entry("gilc_run", **locals())


def plan_capture(*, L, K, periodic, sigma_grid, n_systems, n_cap, n_obs, n_groups=0, c_bins=16, h_bins=40, first_obs=0,
                 want_states=True):
    """gilc_plan: which kernel `run_capture_raw` would use (shape 0: systems in LDS, 1: large systems), its threads per system,
    LDS, row length, work and output bytes, by host arithmetic; no device needed.  Refuses what the run would refuse on these
    numbers."""
    return _plan("gilc_plan", dict(L=L, K=K, periodic=periodic, sigma_grid=sigma_grid, n_systems=n_systems, n_cap=n_cap, n_obs=n_obs),
                 [int(n_groups), int(c_bins), int(h_bins), int(first_obs), int(bool(want_states))])


def run_profiles_raw(*, L, K, periodic, sigma_grid, rate_diffusion, rate_active, betas, states, times_obs, T, seed=0,
                     minus_anchor=True, immobilize=True, suppress_flip=True, crowding=False, k_on=0.0, k_off=0.0, k_exit=0.0,
                     anchor_mask=None, uniforms=None, max_events=None, want_states=True, x_wall=0, ref_obs=-1, front_lo=None,
                     block_table=None, device=0, flip_table=None, n_bins=None, first_obs=0, want_field=False, group_of_system=None,
                     n_groups=None, per_system=False, n_cap=None):
    """`run_raw` with the bin counts of every observation from `first_obs` on summed over the systems of a group inside the
    event loop (gilp_run of include/gillespie_profile.h); the library picks the kernel as for `run_structure_raw`.
    `n_bins=None`: min(L, 1024).  `group_of_system` [systems]: the group a system adds to, None: all to group 0;
    `n_groups=None`: the largest id + 1.  The dictionary of `run_raw` plus
      `ensemble_sums` [groups][observations][7][n_bins] int64: PROFILE_COLUMNS (sums over the group's members of n+, n-, n_bound,
                      n+^2, n-^2, n+ n- per bin, and of the bin's field sum in 2^-32 fixed point when `want_field`);
      `members`       [groups][observations] int32: the systems of the group that recorded the observation;
      `profile_obs`   [systems][observations][3][n_bins] int32 when `per_system`: one system's own n+, n-, n_bound;
      `bin_width`, `n_bins_used`: the sites of a bin (the last used one may hold fewer) and the bins that hold sites."""
    n_bins = min(int(L), GILP_MAX_BINS) if n_bins is None else int(n_bins)
    if n_groups is None:
        n_groups = 1 if group_of_system is None else int(max(0, np.max(group_of_system))) + 1
    return _run_batch_entry("gilp_run", **locals())


def plan_profiles(*, L, K, periodic, sigma_grid, n_systems, n_cap, n_obs, n_bins, n_groups=1, first_obs=0, want_field=False,
                  want_states=True, per_system=False):
    """gilp_plan: which kernel `run_profiles_raw` would use (shape 0: systems in LDS, 1: large systems), its threads per system,
    LDS, the bin width and the bins that hold sites, work and output bytes, by host arithmetic; no device needed.  Refuses what
    the run would refuse on these numbers."""
    return _plan("gilp_plan", dict(L=L, K=K, periodic=periodic, sigma_grid=sigma_grid, n_systems=n_systems, n_cap=n_cap, n_obs=n_obs),
                 [int(n_bins), int(n_groups), int(first_obs), int(want_field), int(bool(want_states)), int(bool(per_system))])


def run_profiles_resumable_raw(*, L, K, periodic, sigma_grid, rate_diffusion, rate_active, betas, states, times_obs, T, seed=0,
                               minus_anchor=True, immobilize=True, suppress_flip=True, crowding=False, k_on=0.0, k_off=0.0, k_exit=0.0,
                               anchor_mask=None, uniforms=None, max_events=None, want_states=True, x_wall=0, ref_obs=-1, front_lo=None,
                               block_table=None, device=0, flip_table=None, n_bins=None, first_obs=0, want_field=False,
                               group_of_system=None, n_groups=None, per_system=False, n_cap=None, obs_first=0, checkpoint=None):
    """`run_profiles_raw` as one SEGMENT of a run (gilpr_run of include/gillespie_profile_resume.h), with the slices and the
    checkpoint of `run_resumable_raw`: `times_obs` holds the absolute times of the observations obs_first, obs_first + 1, ...;
    `checkpoint` is the dictionary a previous segment returned under "checkpoint", or None for a fresh start from `states`.
    `first_obs` is an ABSOLUTE index on the run's grid; `n_bins`, `want_field`, the groups and `per_system` are the run's in every
    segment.  The library picks the kernel as for `run_profiles_raw` (`plan_profiles`, which does not depend on the number of
    observations), so every segment has the same shape and keys.  `ensemble_sums`, `members` and `profile_obs` cover this
    segment's rows; laid one after the other along the observation axis they are the one launch's.  The result also has
    "checkpoint" and "first_row"."""
    n_bins = min(int(L), GILP_MAX_BINS) if n_bins is None else int(n_bins)
    if n_groups is None:
        n_groups = 1 if group_of_system is None else int(max(0, np.max(group_of_system))) + 1
    return _run_batch_entry("gilpr_run", **locals())


def _mixed_descriptor(S, K, sigma_grids, variant_of_system, block_tables=None, seeds=None, streams=None, order=None):
    """struct gilx_variants for S systems, and the arrays it points to (keep them alive for the call)."""
    sg = np.ascontiguousarray(sigma_grids, dtype=np.float64).reshape(-1)
    V = len(sg)
    keep = [sg]

    def per_system(a, dtype, name):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.shape != (S,):
            raise ValueError(f"{name} must have one entry per system")
        keep.append(a)
        return _p(a).value

    bt = None
    if block_tables is not None:
        bt = np.ascontiguousarray(block_tables, dtype=np.uint8)
        if bt.shape != (V, K + 1, K + 1):
            raise ValueError("block_tables must be [variants][K + 1][K + 1]")
        keep.append(bt)
    if seeds is not None:
        seeds = [int(x) & (2 ** 64 - 1) for x in seeds]
    desc = GilxVariants(n_variants=V, sigma_grid=_p(sg).value, block_table=None if bt is None else _p(bt).value,
                        variant_of_system=per_system(variant_of_system, np.int32, "variant_of_system"),
                        seed=per_system(seeds, np.uint64, "seeds"), stream=per_system(streams, np.int32, "streams"),
                        order=per_system(order, np.int32, "order"))
    return desc, keep


def plan_mixed(*, L, K, periodic, sigma_grids, n_systems, n_cap, n_obs, variant_of_system=None, order=None, want_states=True):
    """gilx_plan: what a mixed launch (`run_mixed_raw`) would use -- threads per system, LDS of a workgroup (the longest table of
    the batch), that table's length, the doubles of all tables, systems per CU by LDS and the output bytes -- by host arithmetic;
    no device needed.  Refuses what the run would refuse on these numbers."""
    return _plan("gilx_plan", dict(L=L, K=K, periodic=periodic, n_systems=n_systems, n_cap=n_cap, n_obs=n_obs), [int(bool(want_states))],
                 dict(sigma_grids=sigma_grids, variant_of_system=variant_of_system, order=order))


def run_mixed_raw(*, L, K, periodic, sigma_grids, variant_of_system, rate_diffusion, rate_active, betas, states, times_obs, T, seed=0,
                  minus_anchor=True, immobilize=True, suppress_flip=True, crowding=False, k_on=0.0, k_off=0.0, k_exit=0.0,
                  anchor_mask=None, uniforms=None, max_events=None, want_states=True, x_wall=0, ref_obs=-1, front_lo=None,
                  block_tables=None, device=0, flip_table=None, seeds=None, streams=None, order=None, n_cap=None):
    """`run_raw` for a MIXED batch (gilx_run of include/gillespie_mixed.h): system s runs with the interaction range
    `sigma_grids[variant_of_system[s]]` and the blocking table `block_tables[variant_of_system[s]]` ([variants][K + 1][K + 1], or
    None), all systems in one launch.  `seeds[s]`, `streams[s]`: Philox key and system index of system s (None: `seed` and s), so
    that a system can draw what it would draw in a `run_raw` launch of its own group.  `order`: the system each workgroup takes,
    a permutation (None: falling particle number).  Same dictionary as `run_raw`; the slots at and beyond a system's own particle
    number are zero in `pos`, `sigma` and `flags`."""
    return _run_mixed_entry("gilx_run", locals())              # first statement: locals() are the keywords


def plan_mixed_many(*, L, K, periodic, sigma_grids, n_systems, n_cap, n_obs, variant_of_system=None, order=None, want_states=True):
    """gilxm_plan: what a mixed launch of large systems (`run_mixed_many_raw`) would use -- rate blocks, the longest table, the
    longest one kept in LDS (-1: none), the variants read from global memory, LDS of a workgroup, the doubles of all tables, work
    bytes per system and output bytes -- by host arithmetic; no device needed.  Refuses what the run would refuse on these numbers."""
    return _plan("gilxm_plan", dict(L=L, K=K, periodic=periodic, n_systems=n_systems, n_cap=n_cap, n_obs=n_obs), [int(bool(want_states))],
                 dict(sigma_grids=sigma_grids, variant_of_system=variant_of_system, order=order))


def run_mixed_many_raw(*, L, K, periodic, sigma_grids, variant_of_system, rate_diffusion, rate_active, betas, states, times_obs, T, seed=0,
                       minus_anchor=True, immobilize=True, suppress_flip=True, crowding=False, k_on=0.0, k_off=0.0, k_exit=0.0,
                       anchor_mask=None, uniforms=None, max_events=None, want_states=True, x_wall=0, ref_obs=-1, front_lo=None,
                       block_tables=None, device=0, flip_table=None, seeds=None, streams=None, order=None, n_cap=None):
    """`run_mixed_raw` for systems beyond one workgroup's LDS (gilxm_run of include/gillespie_mixed_many.h): the large-system
    kernel of `run_many_large_raw`, one workgroup per system, with a variant per system.  Same keywords, same dictionary.  The
    defaults of the keys are the large shape's: `seeds=None` is `seed` + s, `streams=None` is 0, so one variant with the defaults
    is `run_many_large_raw`.  Any L >= 2 is accepted; system s is, bit for bit, the `run_many_large_raw` system with its
    variant's range and blocking table under key `seeds[s]` (include/gillespie_mixed_many.h states the condition on n_cap)."""
    return _run_mixed_entry("gilxm_run", locals())


def plan_mixed_profiles(*, L, K, periodic, sigma_grids, n_systems, n_cap, n_obs, n_bins, n_groups=1, first_obs=0, want_field=False,
                        variant_of_system=None, order=None, want_states=True, per_system=False):
    """gilxp_plan: what a mixed launch with the ensemble profiles (`run_mixed_profiles_raw`) would use -- the shape (0: systems in
    LDS, gilx_run's kernel; 1: large systems, gilxm_run's), threads per system, LDS of a workgroup (the mixed launch's for the
    longest table plus the profile slots), that table's length, the bin width and the bins that hold sites, the doubles of all
    tables, work and output bytes -- by host arithmetic; no device needed.  Refuses what the run would refuse on these numbers."""
    return _plan("gilxp_plan", dict(L=L, K=K, periodic=periodic, n_systems=n_systems, n_cap=n_cap, n_obs=n_obs),
                 [int(n_bins), int(n_groups), int(first_obs), int(want_field), int(bool(want_states)), int(bool(per_system))],
                 dict(sigma_grids=sigma_grids, variant_of_system=variant_of_system, order=order))


def run_mixed_profiles_raw(*, L, K, periodic, sigma_grids, variant_of_system, rate_diffusion, rate_active, betas, states, times_obs, T, seed=0,
                           minus_anchor=True, immobilize=True, suppress_flip=True, crowding=False, k_on=0.0, k_off=0.0, k_exit=0.0,
                           anchor_mask=None, uniforms=None, max_events=None, want_states=True, x_wall=0, ref_obs=-1, front_lo=None,
                           block_tables=None, device=0, flip_table=None, seeds=None, streams=None, order=None, n_cap=None, n_bins=None,
                           first_obs=0, want_field=False, group_of_system=None, n_groups=None, per_system=False):
    """`run_mixed_raw` with the bin counts of `run_profiles_raw` summed over the systems of a group in the same launch, every
    system with its own variant's field (gilxp_run of include/gillespie_mixed_profile.h).  The library picks the kernel as
    `plan_mixed_profiles` tells: `run_mixed_raw`'s or `run_mixed_many_raw`'s, and the defaults of `seeds` and `streams` are that
    shape's.  A group may hold systems of different variants.  The dictionary of `run_mixed_raw` plus `ensemble_sums`, `members`,
    `profile_obs` (when `per_system`), `bin_width` and `n_bins_used` of `run_profiles_raw`."""
    n_bins = min(int(L), GILP_MAX_BINS) if n_bins is None else int(n_bins)
    if n_groups is None:
        n_groups = 1 if group_of_system is None else int(max(0, np.max(group_of_system))) + 1
    return _run_mixed_entry("gilxp_run", locals())


def run_mixed_profiles_resumable_raw(*, L, K, periodic, sigma_grids, variant_of_system, rate_diffusion, rate_active, betas, states, times_obs,
                                     T, seed=0, minus_anchor=True, immobilize=True, suppress_flip=True, crowding=False, k_on=0.0, k_off=0.0,
                                     k_exit=0.0, anchor_mask=None, uniforms=None, max_events=None, want_states=True, x_wall=0, ref_obs=-1,
                                     front_lo=None, block_tables=None, device=0, flip_table=None, seeds=None, streams=None, order=None,
                                     n_cap=None, n_bins=None, first_obs=0, want_field=False, group_of_system=None, n_groups=None,
                                     per_system=False, obs_first=0, checkpoint=None):
    """`run_mixed_profiles_raw` as one SEGMENT of a run (gilxpr_run of include/gillespie_profile_resume.h), with the slices and the
    checkpoint of `run_mixed_resumable_raw` (the six arrays and `n_slots`; no window sums).  `first_obs` is an ABSOLUTE index on
    the run's grid.  The library picks the kernel as `plan_mixed_profiles` tells, for every segment alike; the keys (`seeds`,
    `streams`) and the variants are the resuming launch's.  The three profile arrays cover this segment's rows."""
    n_bins = min(int(L), GILP_MAX_BINS) if n_bins is None else int(n_bins)
    if n_groups is None:
        n_groups = 1 if group_of_system is None else int(max(0, np.max(group_of_system))) + 1
    return _run_mixed_entry("gilxpr_run", locals())


def plan_mixed_structure(*, L, K, periodic, sigma_grids, n_systems, n_cap, n_obs, k_max, first_obs=0, variant_of_system=None,
                         order=None, want_states=True, want_rows=True):
    """gilxs_plan: what a mixed launch with the structure sums (`run_mixed_structure_raw`) would use -- threads per system, LDS of
    a workgroup (with the sums' slots and, where it fits, the phase table), the longest table's length, systems per CU by LDS, the
    row length, work and output bytes -- by host arithmetic; no device needed.  Refuses what the run would refuse on these
    numbers.  Without rows and states the output bytes do not grow with n_obs * k_max."""
    return _plan("gilxs_plan", dict(L=L, K=K, periodic=periodic, n_systems=n_systems, n_cap=n_cap, n_obs=n_obs),
                 [int(k_max), int(first_obs), int(bool(want_states)), int(bool(want_rows))],
                 dict(sigma_grids=sigma_grids, variant_of_system=variant_of_system, order=order))


def run_mixed_structure_raw(*, L, K, periodic, sigma_grids, variant_of_system, rate_diffusion, rate_active, betas, states, times_obs, T,
                            seed=0, minus_anchor=True, immobilize=True, suppress_flip=True, crowding=False, k_on=0.0, k_off=0.0,
                            k_exit=0.0, anchor_mask=None, uniforms=None, max_events=None, want_states=True, x_wall=0, ref_obs=-1,
                            front_lo=None, block_tables=None, device=0, flip_table=None, seeds=None, streams=None, order=None,
                            n_cap=None, k_max=None, first_obs=0, want_rows=True):
    """`run_mixed_raw` with the structure sums of `run_structure_raw` taken in the same launch, every system with its own table
    and field mode, and reduced over the window of observations on the device (gilxs_run of
    include/gillespie_mixed_structure.h).  The dictionary of `run_mixed_raw` plus
      `head`      [systems][observations][4]: n, sum occ^2, sum m, sum m^2 of every recorded observation (row entries 0..3);
      `window`    [systems][k_max][3]: per mode a0, sum d, sum d^2 over the recorded observations from `first_obs` on that had a
                  live particle, d = a - a0, a = sqrt(re^2 + im^2) / n (observables.DeviceStructureWindow);
      `n_window`, `n_empty` [systems]: observations accumulated, and window observations without a live particle;
      `structure` [systems][observations][4 + 2 k_max] when `want_rows`, as `run_structure_raw` (None otherwise: no row is stored);
      `bytes_back`: the bytes of the output arrays the call copied back.
    One variant is the uniform batch.  `k_max=None`: all L modes (at most 4096)."""
    k_max = min(int(L), 4096) if k_max is None else int(k_max)
    return _run_mixed_entry("gilxs_run", locals())


def run_mixed_resumable_raw(*, L, K, periodic, sigma_grids, variant_of_system, rate_diffusion, rate_active, betas, states, times_obs, T, seed=0,
                            minus_anchor=True, immobilize=True, suppress_flip=True, crowding=False, k_on=0.0, k_off=0.0, k_exit=0.0,
                            anchor_mask=None, uniforms=None, max_events=None, want_states=True, x_wall=0, ref_obs=-1, front_lo=None,
                            block_tables=None, device=0, flip_table=None, seeds=None, streams=None, order=None, n_cap=None, large=False,
                            obs_first=0, checkpoint=None):
    """`run_mixed_raw` (large=True: `run_mixed_many_raw`) as one SEGMENT of a run (gilxr_run / gilxmr_run of
    include/gillespie_mixed_resume.h), the counterpart of `run_resumable_raw`: `times_obs` holds the absolute times of the
    observations obs_first, obs_first + 1, ... of the run's grid; `checkpoint` is the dictionary a previous segment returned under
    "checkpoint" (the six arrays of `run_resumable_raw` and `n_slots`, every system's slot count of the run's start), or None for
    a fresh start from `states`.  The keys (`seeds`, `streams`) and the variants are the resuming launch's: pass the same for the
    same trajectory.  The result also has "checkpoint", "first_row", and "n0" = the slot counts."""
    return _run_mixed_entry("gilxmr_run" if large else "gilxr_run", locals())


def run_mixed_structure_resumable_raw(*, L, K, periodic, sigma_grids, variant_of_system, rate_diffusion, rate_active, betas, states, times_obs,
                                      T, seed=0, minus_anchor=True, immobilize=True, suppress_flip=True, crowding=False, k_on=0.0, k_off=0.0,
                                      k_exit=0.0, anchor_mask=None, uniforms=None, max_events=None, want_states=True, x_wall=0, ref_obs=-1,
                                      front_lo=None, block_tables=None, device=0, flip_table=None, seeds=None, streams=None, order=None,
                                      n_cap=None, k_max=None, first_obs=0, want_rows=True, obs_first=0, checkpoint=None):
    """`run_mixed_structure_raw` as one SEGMENT of a run (gilxsr_run of include/gillespie_mixed_resume.h).  `first_obs` is an
    ABSOLUTE index on the run's grid, `k_max` the run's in every segment.  `checkpoint` also holds `window`, `n_window` and
    `n_empty`, which the segment continues; the dictionary's `window`, `n_window`, `n_empty` are those of the checkpoint it
    leaves (the sums over all segments so far), `head` and `structure` cover this segment's rows."""
    k_max = min(int(L), 4096) if k_max is None else int(k_max)
    return _run_mixed_entry("gilxsr_run", locals())


def _run_mixed_entry(entry, keywords):
    """_run_batch_entry for the mixed raw functions: `keywords` = their locals(), of which the six of _mixed_descriptor travel as
    `mixed`; a mixed launch has no range or blocking table of its own."""
    kw = {k: v for k, v in keywords.items() if k != "large"}
    mixed = {k: kw.pop(k) for k in ("sigma_grids", "variant_of_system", "block_tables", "seeds", "streams", "order")}
    return _run_batch_entry(entry, sigma_grid=0.0, block_table=None, mixed=mixed, **kw)


def _run_batch_entry(entry, *, L, K, periodic, sigma_grid, rate_diffusion, rate_active, betas, states, times_obs, T, seed,
                     minus_anchor, immobilize, suppress_flip, crowding, k_on, k_off, k_exit, anchor_mask, uniforms, max_events,
                     want_states, x_wall, ref_obs, front_lo, block_table, device, flip_table, k_max=None, first_obs=0,
                     group_of_site=None, n_groups=0, c_bins=0, h_bins=0, h_dt=0.0, n_cap=None, n_bins=0, want_field=False,
                     group_of_system=None, per_system=False, mixed=None, want_rows=True, obs_first=0, checkpoint=None):
    """One launch of the entry point `entry` of ENTRIES.  The batch entry points take the same arguments: gil_run_batch (systems in
    LDS), gilm_run (large systems), gils_run (either, with the structure sums: k_max, first_obs) and gilc_run (either, with the
    capture statistics: group_of_site, n_groups, c_bins, h_bins, h_dt, first_obs); gilp_run (either, with the ensemble profiles:
    n_bins, first_obs, want_field, group_of_system, n_groups, per_system); gilx_run (systems in LDS, a variant per system: `mixed`,
    the keywords of _mixed_descriptor), gilxm_run (the same, large systems), gilxs_run (the same with the structure sums: k_max,
    first_obs, want_rows) and gilxp_run (`mixed` with gilp_run's keywords, either shape); gilr_run and gilrm_run (one segment of a
    run: obs_first, checkpoint); gilxr_run, gilxmr_run and
    gilxsr_run (one segment of a mixed run: `mixed`, obs_first, and a checkpoint that also has n_slots and, for gilxsr_run, the
    window sums); gilpr_run and gilxpr_run (one segment of a profile run: gilp_run's / gilxp_run's keywords with first_obs absolute,
    obs_first, and the checkpoint of gilr_run / gilxr_run)."""
    lib, row = _lib(), ENTRIES[entry]
    if row.header is not None and not hasattr(lib, entry):
        raise capi.ApsError(-1, f"the loaded library has no {entry} ({row.header})")
    call, last_error = getattr(lib, entry), getattr(lib, row.last_error)
    ck_in = None
    if checkpoint is not None:                                 # a resumed segment: the systems and their slots are the checkpoint's
        ck_in = _checkpoint_arrays(checkpoint, "checkpoint")
        if n_cap is not None and int(n_cap) != ck_in["pos"].shape[1]:
            raise ValueError("n_cap differs from the checkpoint's")
        n_cap = ck_in["pos"].shape[1]
        states = [((), ())] * ck_in["pos"].shape[0]
    S = len(states)
    betas = np.ascontiguousarray(np.broadcast_to(np.asarray(betas, dtype=np.float64), (S,)))
    ncap = max(1, max(len(st[0]) for st in states))
    if n_cap is not None:
        if int(n_cap) < ncap:
            raise ValueError("n_cap is smaller than an initial state")
        ncap = int(n_cap)
    n0 = np.array([len(st[0]) for st in states], np.int32)
    pos0, sg0, bd0 = np.zeros((S, ncap), np.int32), np.ones((S, ncap), np.int8), np.zeros((S, ncap), np.uint8)
    for s, st in enumerate(states):
        pos0[s, :n0[s]], sg0[s, :n0[s]] = st[0], st[1]
        if len(st) > 2 and st[2] is not None:
            bd0[s, :n0[s]] = st[2]
    times = np.ascontiguousarray(times_obs, dtype=np.float64)
    M = len(times)
    if uniforms is not None:
        uniforms = np.ascontiguousarray(uniforms, dtype=np.float64)
        assert uniforms.shape[0] == S and uniforms.shape[2] == 4
        max_events = uniforms.shape[1]
    elif max_events is None:
        max_events = 2 ** 40
    par, keep = _params(L=L, K=K, periodic=periodic, n_systems=S, n_cap=ncap, n_obs=M, sigma_grid=sigma_grid, minus_anchor=minus_anchor,
                        immobilize=immobilize, suppress_flip=suppress_flip, crowding=crowding, device=device, x_wall=x_wall, ref_obs=ref_obs,
                        rate_diffusion=rate_diffusion, rate_active=rate_active, k_on=k_on, k_off=k_off, k_exit=k_exit, T=T, seed=seed,
                        max_events=max_events, beta=betas, times_obs=times, anchor_mask=anchor_mask, front_lo=front_lo, block_table=block_table,
                        flip_table=flip_table)
    pos_obs = np.zeros((S, M, ncap), np.int32) if want_states else None
    sg_obs = np.zeros((S, M, ncap), np.int8) if want_states else None
    fl_obs = np.zeros((S, M, ncap), np.uint8) if want_states else None
    scal = np.zeros((S, M, NSCALARS), np.int64)
    n_rec, n_ev, t_fin = np.zeros(S, np.int32), np.zeros(S, np.int64), np.zeros(S)
    exits, n_exit = np.zeros((S, ncap, 3)), np.zeros(S, np.int32)
    ms = C.c_double()
    results = [pos_obs, sg_obs, fl_obs, scal, n_rec, n_ev, t_fin, exits, n_exit]
    c = types.SimpleNamespace(S=S, M=M, ncap=ncap, L=L, K=K, ck_in=ck_in, ck_more=checkpoint, results=results, keep=[keep])
    own = dict(k_max=k_max, first_obs=first_obs, group_of_site=group_of_site, n_groups=n_groups, c_bins=c_bins, h_bins=h_bins, h_dt=h_dt,
               n_bins=n_bins, want_field=want_field, group_of_system=group_of_system, per_system=per_system, mixed=mixed, want_rows=want_rows,
               obs_first=obs_first)
    front, behind, tail, extra = row.stage(c, **own)
    rc = call(C.byref(par), *front, _p(n0), _p(pos0), _p(sg0), _p(bd0), _p(uniforms), *[_p(a) for a in results], *behind, C.byref(ms), *tail)
    if rc != 0:
        raise capi.ApsError(rc, last_error().decode())
    out = dict(pos=pos_obs, sigma=sg_obs, flags=fl_obs, scalars=scal, n_recorded=n_rec, n_events=n_ev, t_final=t_fin,
               exits=exits, n_exits=n_exit, n0=n0, kernel_ms=ms.value)
    out.update(extra)
    if row.finish is not None:
        out.update(row.finish(c, **own))
    return out


def _large_shape(L, n):
    """Beyond one workgroup's LDS: the large-system kernel, one workgroup per system in one launch (system s: key seed + s)."""
    return L > GIL_MAX_L or n > GIL_MAX_N


def _open_batch(who, systems, *, resume=None, no_exit=False, seed=True, **variants):
    """Opens a batch: the systems may differ in beta, rng / initial condition and particle number only (`variants`: the options of
    particle_system.require_same_shape), `no_exit` asks for k_exit = 0.  Then ALL initial states are drawn, in the order of the
    list, and only then the Philox key (`seed=False`: the caller takes keys per group, mixed_keys).  A resumed run consumes no
    generator.  Returns (first system, initial states, key)."""
    from .particle_system import batch_seed, require_same_shape
    first = require_same_shape(who, systems, **variants)
    if no_exit and first.k_exit:
        raise ValueError(f"{who} needs k_exit = 0")
    if resume is not None:
        return first, None, None
    inits = [ps.init_particles() for ps in systems]
    return first, inits, batch_seed(first) if seed else None


def _model(first, systems, **more):
    """The launch keywords every entry point shares, from the batch's first system (and beta from all of them); `more` adds to
    them or replaces them."""
    kw = dict(L=first.L, K=first.K, periodic=first.periodic, sigma_grid=first._sigma_grid, rate_diffusion=first.rate_diffusion,
              rate_active=first.rate_active, betas=[float(ps.beta) for ps in systems], minus_anchor=first.minus_anchor,
              immobilize=first.immobilize_when_anchored, suppress_flip=first.suppress_flip_when_bound,
              crowding=first.crowding_suppresses_rates, k_on=first.k_on, k_off=first.k_off, k_exit=first.k_exit,
              anchor_mask=first.is_anchor_site, device=first.device, flip_table=first.flip_table())
    kw.update(more)
    return kw


def _statistics_keywords(who, first, times_obs, n_live, one_table=True):
    """The keywords of a launch that takes the sums of observables.DeviceObservables over `times_obs`, and the blocking table of
    every system (the threshold depends on the particle number).  `one_table`: the launch has one table for all, so they must agree."""
    from . import observables
    acc0 = observables.DeviceObservables(times_obs, first.L, first.dx, first.K)
    tables = [acc0.block_table(n) for n in n_live]
    kw = dict(want_states=False, x_wall=acc0.x_wall, ref_obs=acc0.start, front_lo=np.array([acc0.front_range(s)[0] for s in range(first.L)], np.int32))
    if one_table:
        if any(not np.array_equal(t, tables[0]) for t in tables[1:]):
            raise ValueError(f"{who}: the systems' particle numbers give different blocking thresholds; run them in separate batches")
        kw.update(k_exit=0.0, block_table=tables[0])
    return kw, tables


def _require_recorded(r, s, M):
    if int(r["n_recorded"][s]) < M:
        raise RuntimeError("a system passed T before its last observation time (choose T beyond the last observation)")


def _reduce_structure_rows(rows, M, L, dx, start_fraction, kk, first_obs, return_series):
    """observables.DeviceStructure over the rows [M][4 + 2 kk] of one system from `first_obs` on: (its result over the window, the
    accumulator over all observations or None)."""
    from . import observables
    acc = observables.DeviceStructure(M, L, dx, start_fraction, kk)
    series = observables.DeviceStructure(M, L, dx, 0.0, kk) if return_series else None
    for k in range(first_obs, M):
        row = rows[k]
        acc.add(k, row[0], row[1], row[2], row[3], row[4:])
        if series is not None:
            series.add(k, row[0], row[1], row[2], row[3], row[4:])
    return acc.result(), series


def run_batched_exact(systems, T=10.0, obs_dt=0.01, record_fft=False, record_var=False, uniforms=None, want_m_local=True,
                      resume=None, obs_range=None, return_checkpoint=False, obs_per_launch=None):
    """`run()` of several ParticleSystem objects with the reference's exact event-by-event dynamics, all systems at
    once on the GPU.  They may differ in beta, rng / initial condition and particle number only.  Returns the list of
    result dictionaries (reference :542-557).  Observations the loop never reached (t passed T first, ref :515-516)
    keep the reference's pre-allocated zeros / None.  want_m_local=False leaves m_local_list zero (saves one field
    evaluation per observation and system).

    A run may be cut into segments (include/gillespie_resume.h); the segments together are, bit for bit, the run in one launch.
    The observation grid np.arange(0, T, obs_dt) and `T` are the whole run's in every segment; a segment is a range of
    observations.  `obs_range=(k0, k1)`: record the observations k0 .. k1 - 1 only (default: from the start state's next
    observation to the grid's end); the result dictionaries then cover those observations, and an observation the checkpoint
    had already recorded for a system keeps the zeros / None.  `return_checkpoint=True`: return (results, Checkpoint).
    `resume=checkpoint`: start from that state instead of `init_particles()` -- no generator is consumed, and the Philox key is
    the checkpoint's.  The systems passed on resume supply beta, the rate constants and flip_rate_fn, which may differ from the
    values the checkpoint was made with: that is the exact process with the parameter switched at the checkpoint's time (a
    stopping time; the next event draws fresh numbers, so the switched process is exact).  A longer `T` extends a finished run.
    `obs_per_launch=n`: run the range as a chain of launches of at most n observations each and return what one launch returns.
    With none of the four keywords the run is one launch of the entry points that have no checkpoint."""
    who = "run_batched_exact"
    first, inits, seed = _open_batch(who, systems, resume=resume)
    r, times_obs, ck = _launch(who, systems, T, obs_dt, inits, seed, uniforms=uniforms, resume=resume, obs_range=obs_range,
                               return_checkpoint=return_checkpoint, obs_per_launch=obs_per_launch)
    outs = _exact_outputs(systems, r, times_obs, record_fft, record_var, want_m_local)
    first.kernel_ms = r["kernel_ms"]
    return (outs, ck) if return_checkpoint else outs


def _exact_outputs(systems, r, times_obs, record_fft, record_var, want_m_local):
    """The reference's result dictionaries (:542-557) from the raw outputs `r` of a launch with states."""
    from .particle_system import ParticleSystem
    M, L, dx = len(times_obs), systems[0].L, systems[0].dx
    outs = []
    for s, ps in enumerate(systems):
        n0 = int(r["n0"][s])
        pos_list, count, bound_list = [None] * M, [None] * M, [None] * M
        rho_p, rho_m, total, m_loc, m_glob = np.zeros((M, L)), np.zeros((M, L)), np.zeros((M, L)), np.zeros((M, L)), np.zeros(M)
        hat = np.zeros((M, L), dtype=complex) if record_fft else None
        amp = np.zeros((M, L)) if record_fft else None
        var = np.zeros(M) if record_var else None
        for k in range(int(r["first_row"][s]) if "first_row" in r else 0, int(r["n_recorded"][s])):
            fl = r["flags"][s, k, :n0]
            live = (fl & 2) != 0
            p, sg = r["pos"][s, k, :n0][live].astype(np.int64), r["sigma"][s, k, :n0][live]
            pos_list[k], count[k], bound_list[k] = p, p.size, (fl[live] & 1).astype(bool)
            a, b = ParticleSystem.empirical_densities_from_particles(p, sg, L, dx)
            rho_p[k], rho_m[k], total[k] = a, b, a + b
            if want_m_local:                                       # field of the observed state, on the GPU (aps_field_from_counts)
                m_loc[k] = ps.compute_local_m_field(np.bincount(p[sg == 1], minlength=L), np.bincount(p[sg == -1], minlength=L))
            m_glob[k] = np.mean(sg) if sg.size else np.nan
            if record_fft:
                spec = np.fft.fft(total[k])
                hat[k], amp[k] = spec, np.abs(spec)
                if record_var:
                    var[k] = float(np.var(total[k]))
        ex = r["exits"][s, :int(r["n_exits"][s])]
        ps.n_events = int(r["n_events"][s])
        outs.append({"times_obs": times_obs.copy(), "pos_list": pos_list, "rho_p_list": rho_p, "rho_m_list": rho_m,
                     "total_list": total, "particle_count_list": count, "bound_list": bound_list, "m_local_list": m_loc,
                     "m_global": m_glob, "rho_hat_complex": hat, "fft_amp_list": amp, "var_list": var,
                     "exit_times": [float(t) for t in ex[:, 0]], "exit_positions": [int(x) for x in ex[:, 1]]})
    return outs


def run_batched_exact_statistics(systems, T=10.0, obs_dt=0.01, resume=None, obs_range=None, return_checkpoint=False, obs_per_launch=None):
    """The sweep drivers' per-run observables (observables.DeviceObservables: v_eff, D_eff, mean magnetisation, front
    density, blocking probability) for many systems under the exact dynamics, from the integer sums the event-loop
    kernel records at every observation -- no state arrays leave the GPU.  Needs k_exit = 0 like every reference sweep.
    `resume`, `obs_range`, `return_checkpoint`, `obs_per_launch`: as in run_batched_exact.  The observables are those of the
    observations of `obs_range` (the windows of DeviceObservables lie within them); `obs_per_launch` chains the launches and
    evaluates the concatenated sums, which are the single launch's."""
    who = "run_batched_exact_statistics"
    first, inits, seed = _open_batch(who, systems, resume=resume, no_exit=True)
    r, times_obs, ck = _launch(who, systems, T, obs_dt, inits, seed, statistics=True, resume=resume, obs_range=obs_range,
                               return_checkpoint=return_checkpoint, obs_per_launch=obs_per_launch)
    rows = _statistics_rows(who, systems, r, times_obs)
    first.kernel_ms = r["kernel_ms"]
    return (rows, ck) if return_checkpoint else rows


def _statistics_rows(who, systems, r, times_obs):
    """The DeviceObservables rows from the scalar sums of the raw outputs `r` (of one launch, or of a chain: with `first_row`)."""
    from . import observables
    first = systems[0]
    if np.any(r.get("first_row", 0) > 0):
        raise ValueError(f"{who}: the checkpoint's systems stand at different observations; the sums need a common first observation")
    rows = []
    for s, ps in enumerate(systems):
        _require_recorded(r, s, len(times_obs))
        acc = observables.DeviceObservables(times_obs, first.L, first.dx, first.K)
        for k in range(len(times_obs)):
            sums = dict(zip(SCALARS, (int(v) for v in r["scalars"][s, k])))
            acc.add(k, sums, sums["n_front"] if k >= acc.start and sums["max_pos"] >= 0 else None)
        rows.append(acc.result())
        ps.n_events = int(r["n_events"][s])
    return rows


def _refuse_resume(who, resume, mixed=False, own=None):
    """The structure, capture, profile and mixed launches carry sums of their own across a run (window sums, bind times, group
    rows) or values per system (slot counts, keys), which a Checkpoint does not hold: they cannot start from one.  `mixed`: the
    mixed launches resume from a MixedCheckpoint, which is not refused here.  `own`: the profile functions resume from the class
    of their own alone (ProfileCheckpoint, MixedProfileCheckpoint), whose fingerprint holds what keeps the rows of a chain together."""
    if own is not None and isinstance(resume, own):
        return
    if resume is not None and not (own is None and mixed and isinstance(resume, MixedCheckpoint)):
        raise ValueError(f"{who} cannot resume from a checkpoint: its launch carries sums across the run that a Checkpoint does not hold "
                         "(include/gillespie_resume.h); run_batched_exact and run_batched_exact_statistics can")


CHECKPOINT_STREAMS = {"batch": "key = seed, stream = system index (gil_run_batch)", "large": "key = seed + system index, stream = 0 (gilm_run)"}


def _anchor_mask(mask, L):
    """An anchor mask as the checkpoints hold and compare it: uint8 [L], all zero for a system without anchors."""
    return np.zeros(int(L), np.uint8) if mask is None else (np.asarray(mask).reshape(-1) != 0).astype(np.uint8)


def _checkpoint_arrays(given, who):
    """The six arrays of CHECKPOINT_ARRAYS out of the mapping `given`, converted; ValueError in the name of `who` unless their
    shapes agree."""
    a = {k: np.ascontiguousarray(given[k], dtype=dt) for k, dt, _ in CHECKPOINT_ARRAYS}
    if a["pos"].ndim != 2 or any(a[k].shape != a["pos"].shape[:nd] for k, _, nd in CHECKPOINT_ARRAYS):
        raise ValueError(f"{who}: pos, flags, ref must be [systems][slots], t, n_events, next_obs [systems]")
    return a


class _SavedState:
    """What Checkpoint and MixedCheckpoint share: the six arrays, L and the anchor mask, and a fingerprint that `require` compares
    and `save` / `load` carry.  A subclass states FINGERPRINT (the fields, in the order `require` names them), OPTIONAL (those a
    checkpoint may lack), META (the scalars of the file's `meta`) and SAVED (its arrays in the file beyond `arrays()`)."""
    FINGERPRINT = OPTIONAL = META = SAVED = ()

    def _take(self, given, L, anchor_mask):
        vars(self).update(_checkpoint_arrays(given, type(self).__name__))
        self.L = int(L)
        self.anchor_mask = _anchor_mask(anchor_mask, self.L)

    n_systems = property(lambda self: self.pos.shape[0])
    n_cap = property(lambda self: self.pos.shape[1])

    def arrays(self):
        """The dictionary of arrays `run_resumable_raw(checkpoint=...)` takes."""
        return {k: getattr(self, k) for k, _, _ in CHECKPOINT_ARRAYS}

    def fingerprint(self):
        return {k: getattr(self, k) for k in self.FINGERPRINT}

    def require(self, **expected):
        """ValueError naming the first fingerprint field whose value differs from `expected[field]`."""
        mine, name = self.fingerprint(), type(self).__name__
        for k in self.FINGERPRINT + self.OPTIONAL:
            if k not in expected:
                continue
            if k not in mine:
                raise ValueError(f"{name}: the resuming run differs from the checkpoint in {k}: the checkpoint is of a run without structure sums")
            want = expected[k]
            if k == "anchor_mask":
                same = np.array_equal(mine[k], _anchor_mask(want, self.L))
            elif k == "seeds":
                same = np.array_equal(mine[k], np.array([int(x) & (2 ** 64 - 1) for x in want], dtype=np.uint64))
            elif isinstance(mine[k], np.ndarray):
                same = np.array_equal(mine[k], np.asarray(want, dtype=mine[k].dtype))
            else:
                same = mine[k] == want
            if not same:
                shown = "" if isinstance(mine[k], np.ndarray) and mine[k].size > 16 else f": the checkpoint has {mine[k]!r}, the resuming run {want!r}"
                raise ValueError(f"{name}: the resuming run differs from the checkpoint in {k}{shown}")

    def save(self, path):
        """One .npz without pickles: the arrays, the anchor mask and, as `meta`, the scalar fields."""
        more = {k: getattr(self, k) for k in self.SAVED if getattr(self, k) is not None}
        with open(path, "wb") as fh:
            np.savez(fh, anchor_mask=self.anchor_mask, meta=np.array(json.dumps({k: getattr(self, k) for k in self.META})), **self.arrays(), **more)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(**{k: z[k] for k in z.files if k != "meta"}, **json.loads(str(z["meta"])))


class Checkpoint(_SavedState):
    """The state of a batch of systems between two launches of the exact event loop (struct gil_checkpoint of
    include/gillespie_resume.h): per system and slot the site (`pos`), the flags (`flags`: GILR_PLUS | GILR_BOUND | GILR_ALIVE)
    and the origin of the displacement sums (`ref`, -1: none); per system the time after the last applied event (`t`; it may
    exceed T, and is +inf once the total rate fell to zero), the events fired since the run's start (`n_events` = index of the
    next event's random numbers) and the first observation not yet recorded (`next_obs`).

    With it travels a fingerprint of what must not change between segments, because the layout or the random numbers depend
    on it: L, K, periodic, local_kernel_sigma, the anchor mask, the numbers of systems and slots, the Philox key `seed`, the
    stream convention `streams` ("batch": the kernel of systems in LDS, "large": the large-system kernel; CHECKPOINT_STREAMS)
    and obs_dt (the observation grid).  Resuming against another value raises ValueError naming the field.  Beta, the rate
    constants and flip_rate_fn are deliberately NOT part of it: the systems passed on resume supply them, and other values than
    before mean the exact process with the parameter switched at the checkpoint's time."""

    FINGERPRINT = ("L", "K", "periodic", "local_kernel_sigma", "anchor_mask", "n_systems", "n_cap", "seed", "streams", "obs_dt")
    META = ("L", "K", "periodic", "local_kernel_sigma", "seed", "streams", "obs_dt")

    def __init__(self, *, pos, flags, ref, t, n_events, next_obs, L, K, periodic, local_kernel_sigma, anchor_mask, seed, streams, obs_dt):
        self._take(locals(), L, anchor_mask)
        if streams not in CHECKPOINT_STREAMS:
            raise ValueError("Checkpoint: streams must be 'batch' or 'large'")
        self.K, self.periodic, self.local_kernel_sigma = int(K), bool(periodic), float(local_kernel_sigma)
        self.seed, self.streams, self.obs_dt = int(seed), str(streams), float(obs_dt)


_PROFILE_FIELDS = ("n_bins", "want_field", "first_obs", "groups", "per_system")


def _take_profile_fields(self, n_bins, want_field, first_obs, groups, per_system):
    """What the two profile checkpoints add to their base: the numbers that must not change between the segments of a profile
    chain, because their rows would no longer belong together."""
    self.n_bins, self.want_field, self.first_obs, self.per_system = int(n_bins), bool(want_field), int(first_obs), bool(per_system)
    self.groups = np.ascontiguousarray(groups, dtype=np.int32)
    if self.groups.shape != (self.n_systems,):
        raise ValueError(f"{type(self).__name__}: groups must have one entry per system")


class ProfileCheckpoint(Checkpoint):
    """The state of a batch between two launches of a PROFILE run (include/gillespie_profile_resume.h): the arrays and the
    fingerprint of `Checkpoint` -- a row of the profile sums belongs to one observation, so the loop state is all a cut hands over
    -- and, in the fingerprint as well, `n_bins`, `want_field`, `first_obs` (absolute on the run's grid), `groups` [systems] and
    `per_system`.  `streams` is the shape the PROFILE plan gives (`plan_profiles`): it can be "large" for a batch-sized system
    whose profile slots do not fit beside the loop, which is why a plain Checkpoint, made elsewhere, is not taken over."""

    FINGERPRINT = Checkpoint.FINGERPRINT + _PROFILE_FIELDS
    META = Checkpoint.META + ("n_bins", "want_field", "first_obs", "per_system")
    SAVED = ("groups",)

    def __init__(self, *, n_bins, want_field, first_obs, groups, per_system, **checkpoint):
        super().__init__(**checkpoint)
        _take_profile_fields(self, n_bins, want_field, first_obs, groups, per_system)


def _merge_segments(parts, k0):
    """The raw outputs of a chain of segments as those of one launch over all their observations (row 0 = observation k0).  Of a
    mixed structure chain also `head` and `structure`, the bytes copied back, and the window sums: those of the last checkpoint.
    Of a profile chain also `ensemble_sums`, `members` and `profile_obs`, whose second axis is the observation's too."""
    last = parts[-1]
    out = {k: (None if parts[0][k] is None else np.concatenate([r[k] for r in parts], axis=1))
           for k in ("pos", "sigma", "flags", "scalars", "head", "structure", "ensemble_sums", "members", "profile_obs") if k in last}
    out.update({k: last[k] for k in ("bin_width", "n_bins_used") if k in last})
    S, ncap = last["exits"].shape[:2]
    exits, n_exits = np.zeros((S, ncap, 3)), np.zeros(S, np.int32)
    for r in parts:                                            # the exit log of a segment holds that segment's exits
        for s in range(S):
            n = int(r["n_exits"][s])
            exits[s, n_exits[s]:n_exits[s] + n] = r["exits"][s, :n]
            n_exits[s] += n
    n_rec = np.clip(last["checkpoint"]["next_obs"] - k0, 0, None).astype(np.int32)
    out.update(exits=exits, n_exits=n_exits, n_recorded=n_rec, first_row=np.minimum(parts[0]["first_row"], n_rec),
               n_events=last["n_events"], t_final=last["t_final"], n0=last["n0"], kernel_ms=float(sum(r["kernel_ms"] for r in parts)),
               checkpoint=last["checkpoint"], launches=len(parts))
    out.update({k: last["checkpoint"][k] for k, _ in _WINDOW_ARRAYS if k in last["checkpoint"]})
    if "bytes_back" in last:
        out["bytes_back"] = int(sum(r["bytes_back"] for r in parts))
    return out


def _chained(resume, obs_range, return_checkpoint, obs_per_launch):
    """Any of the four keywords makes a run a chain of resumable launches; none: the one launch of an entry point without checkpoint."""
    return resume is not None or obs_range is not None or return_checkpoint or obs_per_launch is not None


def _segment_chain(who, run_fn, T, obs_dt, inits, ck, obs_range, obs_per_launch, keywords):
    """The observations `obs_range` of the run (T, obs_dt), from the arrays `ck` of a checkpoint (None: from the fresh initial states
    `inits`), in launches of `run_fn` of at most `obs_per_launch` observations each.  `keywords(times_obs, n_obs)` makes the launch
    keywords once the range (its times, the observations of the longest launch) is known; their `ref_obs` counts within the range
    and is placed in the launch that holds it.  Returns (merged raw outputs with `obs_range`, the observation times)."""
    times_all = np.arange(0.0, T, obs_dt)
    M = len(times_all)
    k0, k1 = (0 if ck is None else int(ck["next_obs"].min()), M) if obs_range is None else (int(obs_range[0]), int(obs_range[1]))
    if not 0 <= k0 < k1 <= M:
        raise ValueError(f"{who}: obs_range must be a non-empty range within the {M} observations of the run (got [{k0}, {k1}))")
    if ck is None and k0 != 0:
        raise ValueError(f"{who}: a run without `resume` starts at observation 0")
    step = k1 - k0 if obs_per_launch is None else int(obs_per_launch)
    if step < 1:
        raise ValueError(f"{who}: obs_per_launch must be at least 1")
    kw = keywords(times_all[k0:k1], min(step, k1 - k0))
    ref_abs = k0 + kw.pop("ref_obs") if "ref_obs" in kw else -1
    parts = []
    for a in range(k0, k1, step):
        b = min(a + step, k1)
        parts.append(run_fn(states=inits, times_obs=times_all[a:b], obs_first=a, checkpoint=ck, ref_obs=ref_abs - a if a <= ref_abs < b else -1, **kw))
        ck = parts[-1]["checkpoint"]
    return dict(_merge_segments(parts, k0), obs_range=(k0, k1)), times_all[k0:k1]


def _launch(who, systems, T, obs_dt, inits, seed, *, uniforms=None, statistics=False, resume=None, obs_range=None, return_checkpoint=False,
            obs_per_launch=None):
    """The launch behind run_batched_exact and (`statistics`) run_batched_exact_statistics, from what _open_batch returned: one
    launch of gil_run_batch / gilm_run or, with any of the four keywords, a chain of gilr_run / gilrm_run.  Returns (raw outputs,
    their observation times, the Checkpoint at the end of a chain or None)."""
    first = systems[0]

    def keywords(times_obs, n_live, **more):                   # the statistics: those of run_batched_exact_statistics' launch
        kw = _model(first, systems, T=T, seed=seed, uniforms=uniforms, **more)
        return dict(kw, **_statistics_keywords(who, first, times_obs, n_live)[0]) if statistics else kw

    if not _chained(resume, obs_range, return_checkpoint, obs_per_launch):
        times_obs, n_live = np.arange(0.0, T, obs_dt), [len(p) for p, _ in inits]
        # the large-system kernel takes the same sums (gilm_run); no state array leaves the device either way
        run = run_many_large_raw if _large_shape(first.L, max(n_live)) else run_raw
        return run(states=inits, times_obs=times_obs, **keywords(times_obs, n_live)), times_obs, None
    mask = _anchor_mask(first.is_anchor_site, first.L)
    if resume is None:
        large, ck, n_live = _large_shape(first.L, max(len(p) for p, _ in inits)), None, [len(p) for p, _ in inits]
    else:
        if not isinstance(resume, Checkpoint):
            raise TypeError(f"{who}: resume must be a gillespie.Checkpoint")
        resume.require(L=first.L, K=first.K, periodic=bool(first.periodic), local_kernel_sigma=float(first.local_kernel_sigma),
                       anchor_mask=mask, n_systems=len(systems), obs_dt=float(obs_dt), streams="large" if _large_shape(first.L, resume.n_cap) else "batch",
                       **({} if first.seed is None else {"seed": int(first.seed)}))
        seed, large, ck = resume.seed, resume.streams == "large", resume.arrays()
        n_live = [int(((f & GILR_ALIVE) != 0).sum()) for f in resume.flags]
    r, times_obs = _segment_chain(who, run_resumable_raw, T, obs_dt, inits, ck, obs_range, obs_per_launch,
                                  lambda times_obs, n_obs: keywords(times_obs, n_live, large=large))
    return r, times_obs, Checkpoint(L=first.L, K=first.K, periodic=first.periodic, local_kernel_sigma=first.local_kernel_sigma,
                                    anchor_mask=mask, seed=seed, streams="large" if large else "batch", obs_dt=obs_dt, **r["checkpoint"])


def mixed_variants(sigma_grids, block_tables=None):
    """The variants of a mixed batch: the distinct pairs of a system's sigma_grid and the bytes of its blocking table.  Returns
    (`sigma_grids` [V], `block_tables` [V][...] or None, `variant_of_system` [S]), the variants in the order of their first
    system.  Two interaction ranges are one variant only when they are the same number: whether their weight tables happen to
    have the same taps is not looked at."""
    index, sig, tabs, owner = {}, [], [], []
    for s, sg in enumerate(sigma_grids):
        tab = None if block_tables is None else np.ascontiguousarray(block_tables[s], dtype=np.uint8)
        key = (float(sg), None if tab is None else tab.tobytes())
        if key not in index:
            index[key] = len(sig)
            sig.append(float(sg))
            tabs.append(tab)
        owner.append(index[key])
    return np.array(sig), (None if block_tables is None else np.stack(tabs)), np.array(owner, np.int32)


def mixed_keys(systems, groups=None, large=False):
    """Philox key and system index of every system of a mixed batch.  `groups[s]` is the group of system s, a group being what one
    `run_raw` launch of the host loop would hold: the key is the seed of the group's FIRST system (its `seed`, or a number drawn
    from its rng -- call this after the initial states were drawn, as the per-group functions do) and the index is the place
    within the group.  None: one group.  `large=True`: the keys of the large shape, where a group is one `run_many_large_raw`
    launch -- the key is the group's key plus the place within the group (mod 2^64) and the stream is 0."""
    from .particle_system import batch_seed
    groups = [0] * len(systems) if groups is None else [int(g) for g in groups]
    if len(groups) != len(systems):
        raise ValueError("groups must have one entry per system")
    key, count, seeds, streams = {}, {}, [], []
    for ps, g in zip(systems, groups):
        if g not in key:
            key[g] = batch_seed(ps)
            count[g] = 0
        seeds.append((int(key[g]) + count[g]) % 2 ** 64 if large else int(key[g]))
        streams.append(0 if large else count[g])
        count[g] += 1
    return seeds, streams


_MIXED_PER_SYSTEM = (("n_slots", np.int32), ("seeds", np.uint64), ("streams", np.int32), ("sigma_grids", np.float64))


class MixedCheckpoint(_SavedState):
    """The state of a MIXED batch between two launches of the exact event loop (struct gilx_checkpoint of
    include/gillespie_mixed_resume.h): the six arrays of `Checkpoint` and, per system, the slot count of the run's start
    (`n_slots`: a mixed system groups its rate sums by it, dead slots included), the Philox key and stream (`seeds`, `streams`)
    and the interaction range on the grid (`sigma_grids`).  A run that counts statistics also keeps the systems' blocking tables
    (`block_tables` [systems][K + 1][K + 1]); a structure run keeps `k_max`, `first_obs` (on the run's grid) and the window sums
    so far (`window` [systems][k_max][3], `n_window`, `n_empty`).  `large`: the large-system kernel (its keys' convention).

    The fingerprint is what must not change between segments: L, K, periodic, the anchor mask, the numbers of systems and slots,
    obs_dt, `large`, and per system sigma_grids, seeds, streams and n_slots; a structure run adds k_max and first_obs.  Resuming
    against another value raises ValueError naming the field.  Beta, the rate constants and flip_rate_fn are deliberately NOT
    part of it, as in `Checkpoint`: other values on resume are the exact process with the parameter switched at the
    checkpoint's time."""

    FINGERPRINT = ("L", "K", "periodic", "anchor_mask", "n_systems", "n_cap", "obs_dt", "large", "sigma_grids", "seeds", "streams", "n_slots")
    OPTIONAL = ("k_max", "first_obs")
    META = ("L", "K", "periodic", "obs_dt", "large", "k_max", "first_obs")
    SAVED = ("seeds", "streams", "sigma_grids", "block_tables")

    def __init__(self, *, pos, flags, ref, t, n_events, next_obs, n_slots, seeds, streams, sigma_grids, L, K, periodic, anchor_mask, obs_dt,
                 large=False, block_tables=None, k_max=None, first_obs=None, window=None, n_window=None, n_empty=None):
        given = locals()
        self._take(given, L, anchor_mask)
        S = self.n_systems
        for k, dt in _MIXED_PER_SYSTEM:
            a = [int(x) & (2 ** 64 - 1) for x in given[k]] if k == "seeds" else given[k]
            setattr(self, k, np.ascontiguousarray(a, dtype=dt))
            if getattr(self, k).shape != (S,):
                raise ValueError(f"MixedCheckpoint: {k} must have one entry per system")
        self.K, self.periodic, self.obs_dt, self.large = int(K), bool(periodic), float(obs_dt), bool(large)
        self.block_tables = None if block_tables is None else np.ascontiguousarray(block_tables, dtype=np.uint8)
        if self.block_tables is not None and self.block_tables.shape != (S, self.K + 1, self.K + 1):
            raise ValueError("MixedCheckpoint: block_tables must be [systems][K + 1][K + 1]")
        self.k_max = None if k_max is None else int(k_max)
        self.first_obs = None if first_obs is None else int(first_obs)
        if self.k_max is None:
            self.window = self.n_window = self.n_empty = None
        else:
            if first_obs is None or window is None or n_window is None or n_empty is None:
                raise ValueError("MixedCheckpoint: a structure run needs first_obs, window, n_window and n_empty")
            for (k, dt), shape in zip(_WINDOW_ARRAYS, ((S, self.k_max, 3), (S,), (S,))):
                setattr(self, k, np.ascontiguousarray(given[k], dtype=dt))
                if getattr(self, k).shape != shape:
                    raise ValueError(f"MixedCheckpoint: {k} must have the shape {shape}")

    structure = property(lambda self: self.k_max is not None)

    def arrays(self):
        """The dictionary of arrays `run_mixed_resumable_raw(checkpoint=...)` takes (a structure run: with the window sums, as
        `run_mixed_structure_resumable_raw` takes it)."""
        more = ("n_slots",) + (tuple(k for k, _ in _WINDOW_ARRAYS) if self.structure else ())
        return dict(super().arrays(), **{k: getattr(self, k) for k in more})

    def fingerprint(self):
        return dict(super().fingerprint(), **({k: getattr(self, k) for k in self.OPTIONAL} if self.structure else {}))


class MixedProfileCheckpoint(MixedCheckpoint):
    """`ProfileCheckpoint` for a MIXED batch (gilxpr_run of include/gillespie_profile_resume.h): the arrays and the fingerprint of
    `MixedCheckpoint` without window sums, and `n_bins`, `want_field`, `first_obs` (absolute), `groups` (the ensemble groups) and
    `per_system`, in the fingerprint as well.  `large` is the shape the profile plan gives (`plan_mixed_profiles`)."""

    FINGERPRINT = MixedCheckpoint.FINGERPRINT + _PROFILE_FIELDS
    META = MixedCheckpoint.META + ("n_bins", "want_field", "per_system")
    SAVED = MixedCheckpoint.SAVED + ("groups",)

    def __init__(self, *, n_bins, want_field, first_obs, groups, per_system, **checkpoint):
        if checkpoint.get("k_max") is not None:
            raise ValueError("MixedProfileCheckpoint: a profile run carries no window sums (k_max must be None)")
        super().__init__(**checkpoint)
        _take_profile_fields(self, n_bins, want_field, first_obs, groups, per_system)


class _MixedBatch:
    """A mixed batch, opened for one launch or for a chain of segments (`chained`; then `resume` may be a MixedCheckpoint): the
    checks, the initial states (None on resume: no generator is consumed), then the slot counts and the shape, the refusal of a
    large shape without `allow_large`, and the keys -- those of `mixed_keys` (the large shape's for a large shape), on resume the
    checkpoint's, which must be what this batch would take where its systems state their seeds.  `structure` = (k_max or None,
    start_fraction, want_rows, all_observations): the batch of run_batched_exact_structure_mixed, without states (no large shape).
    `profiles` = the profile keywords of run_mixed_profiles_raw: the batch of run_batched_exact_profiles_mixed, without states; its
    shape is the plan's (`plan_mixed_profiles`), asked before the keys are formed; on resume (a MixedProfileCheckpoint) the plan's
    shape and the profile numbers must be the checkpoint's."""

    def __init__(self, who, systems, T, obs_dt, groups, statistics, uniforms, order, structure, allow_large, resume, chained, profiles=None):
        self.who, self.systems, self.T, self.statistics, self.uniforms, self.order, self.resume, self.chained = (
            who, systems, T, statistics, uniforms, order, resume, chained)
        first, self.inits, _ = _open_batch(who, systems, resume=resume, skip=("local_kernel_sigma",), anchors="their anchor sites", flip=True,
                                           no_exit=statistics, seed=False)
        self.first, self.mask = first, _anchor_mask(first.is_anchor_site, first.L)
        self.sig_sys = np.array([float(ps._sigma_grid) for ps in systems])
        self.k_max = self.first_obs = self.want_rows = self.tables = None
        self.profiles = None if profiles is None else dict(profiles, want_states=False)
        if structure is not None:                              # the window is [first_obs, M) on the WHOLE grid of M observations
            k_max, start_fraction, self.want_rows, all_obs = structure
            self.k_max = first.L if k_max is None else min(int(k_max), first.L)
            self.first_obs = 0 if all_obs else int(start_fraction * len(np.arange(0.0, T, obs_dt)))
        if resume is None:
            self.n_live = [len(p) for p, _ in self.inits]
            self.n_cap = max(1, max(self.n_live))
            self.large = _large_shape(first.L, self.n_cap)
        else:
            more = {} if structure is None else dict(k_max=self.k_max, first_obs=self.first_obs)
            if self.profiles is not None:                      # what keeps the rows of a profile chain together
                more = dict(n_bins=self.profiles["n_bins"], want_field=bool(self.profiles["want_field"]), first_obs=int(self.profiles["first_obs"]),
                            groups=self.profiles["group_of_system"], per_system=bool(self.profiles["per_system"]))
            resume.require(L=first.L, K=first.K, periodic=bool(first.periodic), anchor_mask=self.mask, n_systems=len(systems), obs_dt=float(obs_dt),
                           sigma_grids=self.sig_sys, **more)
            if structure is None and resume.structure:
                raise ValueError(f"{who}: the checkpoint is of a structure run (it carries window sums); resume it with run_batched_exact_structure_mixed")
            self.n_cap, self.large, self.n_live = resume.n_cap, resume.large, [int(n) for n in resume.n_slots]
        if self.profiles is not None:                          # the profile slots may push a batch-shape launch to the large shape
            sig, _, owner = mixed_variants(self.sig_sys)
            numbers = {k: v for k, v in self.profiles.items() if k != "group_of_system"}
            if chained:                                        # a segment's first_obs is the library's to place; the shape does not depend on it
                numbers["first_obs"] = 0
            self.plan = plan_mixed_profiles(L=first.L, K=first.K, periodic=first.periodic, sigma_grids=sig, n_systems=len(systems),
                                            n_cap=self.n_cap, n_obs=len(np.arange(0.0, T, obs_dt)), variant_of_system=owner, order=order, **numbers)
            if resume is not None:
                resume.require(large=self.plan["shape"] == 1)
            self.large = self.plan["shape"] == 1
        if self.large and not (allow_large and structure is None):
            raise ValueError(f"{who}: L = {first.L}, N = {self.n_cap} is a large shape (beyond L = {GIL_MAX_L}, N = {GIL_MAX_N}); "
                             "the large-system kernel takes no mixed batches")
        if resume is None:
            self.seeds, self.streams = mixed_keys(systems, groups, large=self.large)
        else:
            if all(ps.seed is not None for ps in systems):     # the keys this batch would take: no generator is consumed
                seeds, streams = mixed_keys(systems, groups, large=self.large)
                resume.require(seeds=seeds, streams=streams)
            self.seeds, self.streams = [int(x) for x in resume.seeds], resume.streams

    def keywords(self, times_obs, n_obs):
        """The keywords of a launch of at most `n_obs` of the observations `times_obs` (but states, times_obs and a segment's own):
        the variants, where every system of a statistics run is counted with the blocking table of its own particle number (on
        resume: the checkpoint's), and the model.  Notes the plan as `self.plan`; ValueError if it needs more LDS than there is."""
        first, kw = self.first, {}
        if self.statistics:
            kw, self.tables = _statistics_keywords(self.who, first, times_obs, self.n_live, one_table=False)
            if self.resume is not None and self.resume.block_tables is not None:
                self.tables = list(self.resume.block_tables)
        sig, tabs, owner = mixed_variants(self.sig_sys, self.tables)
        shape = dict(L=first.L, K=first.K, periodic=first.periodic, sigma_grids=sig, n_systems=len(self.systems), n_cap=self.n_cap, n_obs=n_obs,
                     variant_of_system=owner)
        if self.profiles is not None:                          # the plan was asked when the batch was opened
            kw = dict(self.profiles)
        elif self.k_max is not None:                           # a segment's plan takes the window's start within the segment
            kw = dict(want_states=False, k_max=self.k_max, first_obs=self.first_obs, want_rows=self.want_rows)
            self.plan = plan_mixed_structure(**shape, **dict(kw, first_obs=min(self.first_obs, n_obs) if self.chained else self.first_obs))
        else:
            self.plan = (plan_mixed_many if self.large else plan_mixed)(**shape, want_states=not self.statistics)
        if self.plan["lds_bytes"] > GILX_LDS_LIMIT:
            raise ValueError(f"{self.who}: the launch needs {self.plan['lds_bytes']} bytes of LDS per system, over the limit of {GILX_LDS_LIMIT} bytes")
        model = _model(first, self.systems, sigma_grids=sig, variant_of_system=owner, block_tables=tabs, T=self.T, uniforms=self.uniforms,
                       seeds=self.seeds, streams=self.streams, order=self.order, n_cap=self.n_cap, **kw)
        del model["sigma_grid"]                                # a mixed launch has a range per variant instead
        return model


def _mixed_launch(who, systems, T, obs_dt, groups, statistics, uniforms=None, order=None, structure=None, allow_large=False, *, resume=None,
                  obs_range=None, return_checkpoint=False, obs_per_launch=None, profiles=None):
    """The launch behind the four mixed functions: one launch of gilx_run / gilxm_run / gilxs_run / gilxp_run (`profiles`: the profile
    keywords of run_mixed_profiles_raw) or, with any of the four keywords,
    a chain of gilxr_run / gilxmr_run / gilxsr_run (include/gillespie_mixed_resume.h) or, with `profiles`, of gilxpr_run
    (include/gillespie_profile_resume.h; the checkpoint is then a MixedProfileCheckpoint).  Returns (raw outputs with `plan`,
    `obs_range`, `first_obs` and `k_max`, their observation times, the MixedCheckpoint at the end of a chain or None).  A structure
    chain's `head` and `structure` cover the range, its `window`, `n_window`, `n_empty` are the last checkpoint's."""
    chained = _chained(resume, obs_range, return_checkpoint, obs_per_launch)
    b, ck = _MixedBatch(who, systems, T, obs_dt, groups, statistics, uniforms, order, structure, allow_large, resume, chained, profiles), None
    if not chained:
        times_obs = np.arange(0.0, T, obs_dt)
        run_fn = (run_mixed_structure_raw if structure is not None else run_mixed_profiles_raw if profiles is not None
                  else run_mixed_many_raw if b.large else run_mixed_raw)
        r = dict(run_fn(states=b.inits, times_obs=times_obs, **b.keywords(times_obs, len(times_obs))), obs_range=(0, len(times_obs)))
    else:
        run_fn, more = ((run_mixed_profiles_resumable_raw, {}) if profiles is not None else (run_mixed_resumable_raw, dict(large=b.large))
                        if structure is None else (run_mixed_structure_resumable_raw, {}))
        r, times_obs = _segment_chain(who, run_fn, T, obs_dt, b.inits, None if resume is None else resume.arrays(), obs_range, obs_per_launch,
                                      lambda times_obs, n_obs: dict(b.keywords(times_obs, n_obs), **more))
        common = dict(L=b.first.L, K=b.first.K, periodic=b.first.periodic, anchor_mask=b.mask, obs_dt=obs_dt, large=b.large, seeds=b.seeds,
                      streams=b.streams, sigma_grids=b.sig_sys, **r["checkpoint"])
        if profiles is not None:
            ck = MixedProfileCheckpoint(n_bins=profiles["n_bins"], want_field=profiles["want_field"], first_obs=profiles["first_obs"],
                                        groups=profiles["group_of_system"], per_system=profiles["per_system"], **common)
        else:
            ck = MixedCheckpoint(k_max=b.k_max, first_obs=b.first_obs, block_tables=None if b.tables is None else np.stack(b.tables), **common)
    r.update(plan=b.plan, first_obs=b.first_obs, k_max=b.k_max)
    return r, times_obs, ck


def run_batched_exact_mixed(systems, T=10.0, obs_dt=0.01, record_fft=False, record_var=False, uniforms=None, want_m_local=True,
                            groups=None, order=None, resume=None, allow_large=False, obs_range=None, return_checkpoint=False,
                            obs_per_launch=None):
    """`run_batched_exact` for systems that may ALSO differ in `local_kernel_sigma`: one mixed launch (include/gillespie_mixed.h).
    Every other attribute the batched functions compare, the anchor sites and the flip table must agree.  `groups[s]`: the group
    of system s; its systems draw what `run_batched_exact` on the group alone draws (`mixed_keys`).  Returns the list of the
    reference's result dictionaries, one per system.
    `allow_large=True`: a batch that is a large shape (L > 4096, or more than 2048 particles in any system) is one mixed launch
    of the large-system kernel (include/gillespie_mixed_many.h) instead of a ValueError, with the large shape's keys
    (`mixed_keys(..., large=True)`).  Its numbers equal `run_batched_exact` on each group alone where every group is itself a
    large shape, which is always so when L > 4096.  A group below the limit in a batch that straddles it runs on the large kernel
    with large keys: it then equals `run_many_large_raw` for it, not the batch kernel.  A batch that is no large shape is
    launched as without the keyword.
    `resume` (a MixedCheckpoint; a plain Checkpoint does not hold what a mixed launch needs and is refused), `obs_range`,
    `return_checkpoint`, `obs_per_launch`: as in run_batched_exact, through the resumable mixed launches
    (include/gillespie_mixed_resume.h); the segments together are, bit for bit, the one launch.  The keys and slot counts are the
    checkpoint's.  With none of the four the run is the one launch it always was."""
    who = "run_batched_exact_mixed"
    _refuse_resume(who, resume, mixed=True)
    r, times_obs, ck = _mixed_launch(who, systems, T, obs_dt, groups, False, uniforms, order, allow_large=allow_large, resume=resume,
                                     obs_range=obs_range, return_checkpoint=return_checkpoint, obs_per_launch=obs_per_launch)
    outs = _exact_outputs(systems, r, times_obs, record_fft, record_var, want_m_local)
    systems[0].kernel_ms = r["kernel_ms"]
    return (outs, ck) if return_checkpoint else outs


def run_batched_exact_statistics_mixed(systems, T=10.0, obs_dt=0.01, groups=None, order=None, resume=None, allow_large=False,
                                       obs_range=None, return_checkpoint=False, obs_per_launch=None):
    """`run_batched_exact_statistics` for systems that may also differ in `local_kernel_sigma` and whose particle numbers may give
    different blocking thresholds: every system is counted with the blocking table of its own particle number, in one mixed
    launch.  `groups`, `allow_large` as in run_batched_exact_mixed.  Returns the DeviceObservables rows, one per system.
    `resume` (a MixedCheckpoint), `obs_range`, `return_checkpoint`, `obs_per_launch`: as in run_batched_exact_statistics; the
    blocking tables are the checkpoint's."""
    who = "run_batched_exact_statistics_mixed"
    _refuse_resume(who, resume, mixed=True)
    r, times_obs, ck = _mixed_launch(who, systems, T, obs_dt, groups, True, None, order, allow_large=allow_large, resume=resume,
                                     obs_range=obs_range, return_checkpoint=return_checkpoint, obs_per_launch=obs_per_launch)
    rows = _statistics_rows(who, systems, r, times_obs)
    systems[0].kernel_ms = r["kernel_ms"]
    return (rows, ck) if return_checkpoint else rows


def run_batched_exact_structure_mixed(systems, T=10.0, obs_dt=0.01, start_fraction=0.5, k_max=None, groups=None, order=None,
                                      reduce="device", return_series=False, resume=None, obs_range=None, return_checkpoint=False,
                                      obs_per_launch=None):
    """`run_batched_exact_structure` for systems that may ALSO differ in `local_kernel_sigma` (and, like there, in beta, state and
    particle number): one mixed launch that takes the structure sums (include/gillespie_mixed_structure.h).  The other attributes,
    the anchor sites and the flip table must agree, as in run_batched_exact_mixed; `groups`, `order` as there (`mixed_keys`).
    Returns one dict per system with the eight keys of observables.DeviceStructure.result.
    `reduce="device"`: the time means and spreads come from the window sums the launch accumulates
    (observables.DeviceStructureWindow): no row, nothing of size observations x modes, leaves the GPU.  `reduce="rows"`: the launch
    returns the full rows and observables.DeviceStructure reduces them on the host (the cross-check route).
    `return_series=True` adds `times_obs`, `var_series` [M] (from the head rows), `m_series` [M] = sum sigma / n (from the scalar
    sums) and, with reduce="rows" (the sums are then taken at every observation), `fft_amp_series` [M][k_max].
    `resume` (a MixedCheckpoint of a structure run), `obs_range`, `return_checkpoint`, `obs_per_launch`: as in run_batched_exact.
    The window is [int(start_fraction * M), M) on the WHOLE grid, and its sums travel in the checkpoint
    (include/gillespie_mixed_resume.h), so a chain of calls or launches returns what the one launch returns.  The observables are
    evaluated by the call that reaches the grid's end; it must hold the window's head rows, so it may not start inside the
    window (ValueError).  A call that ends earlier returns None in place of every system's dict: take its checkpoint.  Series
    entries before the call's first observation are NaN."""
    who = "run_batched_exact_structure_mixed"
    _refuse_resume(who, resume, mixed=True)
    if reduce not in ("device", "rows"):
        raise ValueError("reduce must be 'device' or 'rows'")
    rows_wanted = reduce == "rows"
    r, _, ck = _mixed_launch(who, systems, T, obs_dt, groups, False, None, order, (k_max, start_fraction, rows_wanted, rows_wanted and return_series),
                             resume=resume, obs_range=obs_range, return_checkpoint=return_checkpoint, obs_per_launch=obs_per_launch)

    def results():
        return _structure_mixed_results(who, systems, r, np.arange(0.0, T, obs_dt), start_fraction, rows_wanted, return_series)

    # a chain notes its times before it evaluates (it may refuse, or have nothing to evaluate yet), the one launch afterwards, as ever
    out = None if ck is not None else results()
    systems[0].kernel_ms, systems[0].bytes_back = r["kernel_ms"], r["bytes_back"]
    if ck is not None:
        out = results()
    return (out, ck) if return_checkpoint else out


def _structure_mixed_results(who, systems, r, times_obs, start_fraction, rows_wanted, return_series):
    """The result dictionaries of run_batched_exact_structure_mixed from the raw outputs `r` of the observations r["obs_range"] of
    the whole grid `times_obs`: None for every system where the range ends before the grid does (the window is not complete)."""
    from . import observables
    first, M, (k0, k1) = systems[0], len(times_obs), r["obs_range"]
    if k1 < M:
        for s, ps in enumerate(systems):
            ps.n_events = int(r["n_events"][s])
        return [None] * len(systems)
    if k0 > r["first_obs"]:
        raise ValueError(f"{who}: this call starts at observation {k0}, inside the window that begins at {r['first_obs']}: the head rows of "
                         "the window's earlier observations lie in an earlier call; cut the run before the window or use obs_per_launch")
    if k0 > 0:
        def whole(a):                                          # rows of the whole grid: zeros before this call's first observation
            return None if a is None else np.concatenate([np.zeros((a.shape[0], k0) + a.shape[2:], a.dtype), a], axis=1)
        r = dict(r, head=whole(r["head"]), structure=whole(r["structure"]), scalars=whole(r["scalars"]), n_recorded=r["n_recorded"] + k0)
    L, out = first.L, []
    for s, ps in enumerate(systems):
        _require_recorded(r, s, M)
        win = observables.DeviceStructureWindow(r["head"][s], r["window"][s], r["n_window"][s], r["n_empty"][s], L, first.dx, start_fraction)
        series = None
        if rows_wanted:
            res, series = _reduce_structure_rows(r["structure"][s], M, L, first.dx, start_fraction, r["k_max"], r["first_obs"], return_series)
        else:
            res = win.result()
        if return_series:
            n, sp = r["scalars"][s, :, 0].astype(float), r["scalars"][s, :, 1].astype(float)
            with np.errstate(divide="ignore", invalid="ignore"):
                m_series = np.where(n > 0, sp / n, np.nan)
            res.update(times_obs=times_obs.copy(), var_series=win.var_series(), m_series=m_series)
            if series is not None:
                res["fft_amp_series"] = np.array(series.amp)
        out.append(res)
        ps.n_events = int(r["n_events"][s])
    return out


def run_batched_exact_structure(systems, T=10.0, obs_dt=0.01, start_fraction=0.5, k_max=None, return_series=False, resume=None):
    """The structure observables of PARTICLE_solver_BIOLOGY_local_structure.py:55-103 for many systems under the exact dynamics,
    from sums the event-loop kernel takes at every observation of the window [int(start_fraction * M), M): no state array and
    nothing of size M x L leaves the GPU.  Returns one dict per system with the reference's eight keys
    (observables.DeviceStructure.result); `k_max=None` means all L modes, as in the reference.  `return_series=True` takes the
    sums at every observation and adds `times_obs`, `fft_amp_series` [M][k_max] and `var_series` [M] (what the reference's
    time_to_pattern, :195-202, reads).  Particles may leave (k_exit > 0): n is the live count of the observation."""
    _refuse_resume("run_batched_exact_structure", resume)
    first, inits, seed = _open_batch("run_batched_exact_structure", systems)
    times_obs = np.arange(0.0, T, obs_dt)
    M, L = len(times_obs), first.L
    kk = L if k_max is None else min(int(k_max), L)
    first_obs = 0 if return_series else int(start_fraction * M)
    r = run_structure_raw(**_model(first, systems, states=inits, times_obs=times_obs, T=T, seed=seed, want_states=False, k_max=kk, first_obs=first_obs))
    rows = []
    for s, ps in enumerate(systems):
        _require_recorded(r, s, M)
        res, series = _reduce_structure_rows(r["structure"][s], M, L, first.dx, start_fraction, kk, first_obs, return_series)
        if series is not None:
            res.update(times_obs=times_obs.copy(), fft_amp_series=np.array(series.amp), var_series=np.array(series.var))
        rows.append(res)
        ps.n_events = int(r["n_events"][s])
    first.kernel_ms = r["kernel_ms"]
    return rows


def run_batched_exact_capture(systems, T=10.0, obs_dt=0.01, c_bins=16, h_bins=40, h_dt=None, start_fraction=0.0, uniforms=None, resume=None):
    """The anchor-capture study of PARTICLE_solver_CLASS.py:766-976 (cluster sizes, bound-state lifetimes, survival curve and
    first-passage density, exit positions, cumulative exits per anchor) for many systems under the exact dynamics, from counts
    the event-loop kernel takes at every event and observation: no state array leaves the GPU.  Returns one dict per system
    (observables.DeviceCapture.result: the keys of observables.capture_observables plus the lifetime histograms, their means and
    variances).  The per-observation rows are taken from observation int(start_fraction * M) on; the series are zero before it.
    `h_dt=None`: T / h_bins.  Lifetimes are resolved to the event and follow the particle, where the reference's are quantised
    to obs_dt and, after the first exit, attributed to shifted particle ids."""
    _refuse_resume("run_batched_exact_capture", resume)
    from . import observables
    first, inits, seed = _open_batch("run_batched_exact_capture", systems, anchors="their anchor sites")
    times_obs = np.arange(0.0, T, obs_dt)
    M, L = len(times_obs), first.L
    groups = observables.anchor_groups(first)
    n_groups = len(first.anchor_idxs)
    h_dt = float(T) / int(h_bins) if h_dt is None else float(h_dt)
    r = run_capture_raw(**_model(first, systems, states=inits, times_obs=times_obs, T=T, seed=seed, uniforms=uniforms, want_states=False,
                                 group_of_site=groups if n_groups else None, n_groups=n_groups, c_bins=c_bins, h_bins=h_bins, h_dt=h_dt,
                                 first_obs=int(start_fraction * M)))
    rows = []
    for s, ps in enumerate(systems):
        _require_recorded(r, s, M)
        acc = observables.DeviceCapture(times_obs, L, n_groups, c_bins, h_dt)
        rows.append(acc.result(r["scalars"][s, :, 0], r["capture"][s], r["exits"][s, :int(r["n_exits"][s])], r["life_hist"][s],
                               r["life_sums"][s]))
        ps.n_events = int(r["n_events"][s])
    first.kernel_ms = r["kernel_ms"]
    return rows


def run_batched_exact_profiles(systems, T=10.0, obs_dt=0.01, n_bins=None, groups=None, first_obs=0, want_field=False,
                               per_system=False, uniforms=None, resume=None, obs_range=None, return_checkpoint=False, obs_per_launch=None):
    """The ensemble profiles <rho+(x, t)>, <rho-(x, t)> and <m(x, t)> of many ParticleSystem objects under the exact dynamics
    (the means over runs of the reference's rho_plus_list, rho_minus_list, m_local_list, PARTICLE_solver_CLASS.py:205-213,
    :517-536), coarse-grained to `n_bins` bins of sites and summed over the runs of a group inside the event loop: no state array
    leaves the GPU, and what does is [groups][observations][7][n_bins].  `groups[s]` is the group system s adds to (None: one
    group).  Returns one dict per group, in the order of the group ids (observables.DeviceProfiles.result); `per_system=True`
    adds each member's own counts as `profile_obs` [members][observations][3][n_bins] (single-run heat maps at n_bins = L).
    `resume` (a ProfileCheckpoint; any other checkpoint is refused), `obs_range`, `return_checkpoint`, `obs_per_launch`: as in
    run_batched_exact, through the resumable profile launches (include/gillespie_profile_resume.h).  A row of the sums belongs to
    one observation, so the rows of a chain are the one launch's, bit for bit, and the result over `obs_range=(k0, k1)` is that of
    those observations; `first_obs` stays an index on the whole grid.  `n_bins`, `want_field`, `first_obs`, `groups` and
    `per_system` must be the checkpoint's.  With none of the four the run is the one launch it always was."""
    who = "run_batched_exact_profiles"
    _refuse_resume(who, resume, own=ProfileCheckpoint)
    first, inits, seed = _open_batch(who, systems, resume=resume)
    L = first.L
    n_bins = min(L, GILP_MAX_BINS) if n_bins is None else int(n_bins)
    owner = np.zeros(len(systems), np.int32) if groups is None else np.asarray(groups, dtype=np.int32)
    n_groups = int(owner.max()) + 1 if owner.size else 1
    prof = dict(n_bins=n_bins, first_obs=first_obs, want_field=want_field, group_of_system=owner, n_groups=n_groups, per_system=per_system)
    ck = None
    if not _chained(resume, obs_range, return_checkpoint, obs_per_launch):
        times_obs = np.arange(0.0, T, obs_dt)
        r = run_profiles_raw(**_model(first, systems, states=inits, times_obs=times_obs, T=T, seed=seed, uniforms=uniforms, want_states=False, **prof))
    else:
        r, times_obs, ck = _profile_chain(who, systems, T, obs_dt, inits, seed, uniforms, prof, resume, obs_range, obs_per_launch)
    out = _profile_results(systems, r, times_obs, owner, n_groups, n_bins, want_field, first_obs, per_system)
    return (out, ck) if return_checkpoint else out


def _profile_chain(who, systems, T, obs_dt, inits, seed, uniforms, prof, resume, obs_range, obs_per_launch):
    """The chain of gilpr_run launches behind run_batched_exact_profiles: (merged raw outputs with `n0` = the live particles of the
    start state, their observation times, the ProfileCheckpoint at the end).  The plan is asked first: its shape says which key
    convention the run has (`streams`), and a checkpoint of the other shape is refused by name."""
    first = systems[0]
    mask = _anchor_mask(first.is_anchor_site, first.L)
    if resume is None:
        n_live, ck = [len(p) for p, _ in inits], None
        n_cap = max(1, max(n_live))
    else:
        n_live, ck, n_cap = [int(((f & GILR_ALIVE) != 0).sum()) for f in resume.flags], resume.arrays(), resume.n_cap
    plan = plan_profiles(L=first.L, K=first.K, periodic=first.periodic, sigma_grid=first._sigma_grid, n_systems=len(systems), n_cap=n_cap,
                         n_obs=1, n_bins=prof["n_bins"], n_groups=prof["n_groups"], want_field=prof["want_field"], want_states=False,
                         per_system=prof["per_system"])       # the shape does not depend on the observations
    streams = "large" if plan["shape"] == 1 else "batch"
    if resume is not None:
        resume.require(L=first.L, K=first.K, periodic=bool(first.periodic), local_kernel_sigma=float(first.local_kernel_sigma), anchor_mask=mask,
                       n_systems=len(systems), obs_dt=float(obs_dt), streams=streams, n_bins=prof["n_bins"], want_field=bool(prof["want_field"]),
                       first_obs=int(prof["first_obs"]), groups=prof["group_of_system"], per_system=bool(prof["per_system"]),
                       **({} if first.seed is None else {"seed": int(first.seed)}))
        seed = resume.seed
    r, times_obs = _segment_chain(who, run_profiles_resumable_raw, T, obs_dt, inits, ck, obs_range, obs_per_launch,
                                  lambda times_obs, n_obs: _model(first, systems, T=T, seed=seed, uniforms=uniforms, want_states=False, **prof))
    r.update(plan=plan, n0=np.array(n_live, np.int32))
    return r, times_obs, ProfileCheckpoint(L=first.L, K=first.K, periodic=first.periodic, local_kernel_sigma=first.local_kernel_sigma,
                                           anchor_mask=mask, seed=seed, streams=streams, obs_dt=obs_dt, n_bins=prof["n_bins"],
                                           want_field=prof["want_field"], first_obs=prof["first_obs"], groups=prof["group_of_system"],
                                           per_system=prof["per_system"], **r["checkpoint"])


def _profile_results(systems, r, times_obs, owner, n_groups, n_bins, want_field, first_obs, per_system):
    """One observables.DeviceProfiles.result per group from the raw outputs `r` of a profile launch, or of a chain over
    r["obs_range"] of the grid (`first_obs` is then placed within the range); notes the event counts and the kernel time."""
    from . import observables
    first = systems[0]
    first_row = max(int(first_obs) - r["obs_range"][0], 0) if "obs_range" in r else first_obs
    out = []
    for g in range(n_groups):
        mine = np.flatnonzero(owner == g)
        prof = observables.DeviceProfiles(times_obs, first.L, first.dx, n_bins, r["ensemble_sums"][g], r["members"][g],
                                          n_particles=[int(r["n0"][s]) for s in mine], k_exit=first.k_exit, want_field=want_field,
                                          first_obs=first_row).result()
        if per_system:
            prof["profile_obs"] = r["profile_obs"][mine]
        out.append(prof)
    for s, ps in enumerate(systems):
        ps.n_events = int(r["n_events"][s])
    first.kernel_ms = r["kernel_ms"]
    return out


def run_batched_exact_profiles_mixed(systems, T=10.0, obs_dt=0.01, n_bins=None, groups=None, key_groups=None, order=None, first_obs=0,
                                     want_field=False, per_system=False, uniforms=None, allow_large=False, resume=None, obs_range=None,
                                     return_checkpoint=False, obs_per_launch=None):
    """`run_batched_exact_profiles` for systems that may ALSO differ in `local_kernel_sigma` (and, like there, in beta, state and
    particle number): one mixed launch that adds every system's bin counts to its group's sums (include/gillespie_mixed_profile.h).
    The other attributes, the anchor sites and the flip table must agree, as in run_batched_exact_mixed.  `groups[s]` is the
    ensemble group system s adds to (None: one group); a group may hold systems of different ranges, but its members must start
    with the same particle number.  `key_groups[s]` is the group of `mixed_keys`: the launch of the host loop whose numbers the
    system draws (None: one launch); `order` as in run_batched_exact_mixed.  Returns one dict per ensemble group, in the order of
    the group ids (observables.DeviceProfiles.result); `per_system=True` adds `profile_obs`.
    The shape is the library's (`plan_mixed_profiles`): the kernel of systems in LDS where L <= 4096, N <= 2048 and the profile
    slots fit beside the loop, else the large-system kernel, which needs `allow_large=True` (ValueError otherwise) and takes the
    large shape's keys (`mixed_keys(..., large=True)`).
    `resume` (a MixedProfileCheckpoint; any other checkpoint is refused), `obs_range`, `return_checkpoint`, `obs_per_launch`: as in
    run_batched_exact_profiles, through gilxpr_run (include/gillespie_profile_resume.h).  The shape of every segment is the
    plan's, so a checkpoint carries it (`large`) and `allow_large` keeps its meaning; the keys and slot counts are the
    checkpoint's.  With none of the four the run is the one launch it always was."""
    who = "run_batched_exact_profiles_mixed"
    _refuse_resume(who, resume, own=MixedProfileCheckpoint)
    first = systems[0]
    n_bins = min(first.L, GILP_MAX_BINS) if n_bins is None else int(n_bins)
    owner = np.zeros(len(systems), np.int32) if groups is None else np.asarray(groups, dtype=np.int32)
    n_groups = int(owner.max()) + 1 if owner.size else 1
    r, times_obs, ck = _mixed_launch(who, systems, T, obs_dt, key_groups, False, uniforms, order, allow_large=allow_large, resume=resume,
                                     obs_range=obs_range, return_checkpoint=return_checkpoint, obs_per_launch=obs_per_launch,
                                     profiles=dict(n_bins=n_bins, first_obs=first_obs, want_field=want_field, group_of_system=owner,
                                                   n_groups=n_groups, per_system=per_system))
    out = _profile_results(systems, r, times_obs, owner, n_groups, n_bins, want_field, first_obs, per_system)
    return (out, ck) if return_checkpoint else out


def run_large_raw(*, L, K, periodic, sigma_grid, rate_diffusion, rate_active, beta, state, times_obs, T, seed=0,
                  minus_anchor=True, immobilize=True, suppress_flip=True, crowding=False, k_on=0.0, k_off=0.0, k_exit=0.0,
                  anchor_mask=None, uniforms=None, max_events=None, want_states=True, device=0, flip_table=None):
    """One large system (gil_run_large): state = (pos, sigma[, bound]).  Returns a dict like run_raw's, without a system axis."""
    lib = _lib()
    pos0 = np.ascontiguousarray(state[0], dtype=np.int32)
    sg0 = np.ascontiguousarray(state[1], dtype=np.int8)
    bd0 = None if len(state) < 3 or state[2] is None else np.ascontiguousarray(state[2], dtype=np.uint8)
    n0 = len(pos0)
    times = np.ascontiguousarray(times_obs, dtype=np.float64)
    M = len(times)
    if uniforms is not None:
        uniforms = np.ascontiguousarray(uniforms, dtype=np.float64)
        max_events = uniforms.shape[0]
    elif max_events is None:
        max_events = 2 ** 40
    betas = np.array([float(beta)])
    ncap = max(n0, 1)
    par, keep = _params(L=L, K=K, periodic=periodic, n_systems=1, n_cap=ncap, n_obs=M, sigma_grid=sigma_grid, minus_anchor=minus_anchor,
                        immobilize=immobilize, suppress_flip=suppress_flip, crowding=crowding, device=device, x_wall=0, ref_obs=-1,
                        rate_diffusion=rate_diffusion, rate_active=rate_active, k_on=k_on, k_off=k_off, k_exit=k_exit, T=T, seed=seed,
                        max_events=max_events, beta=betas, times_obs=times, anchor_mask=anchor_mask, flip_table=flip_table)
    pos_obs = np.zeros((M, ncap), np.int32) if want_states else None
    sg_obs = np.zeros((M, ncap), np.int8) if want_states else None
    fl_obs = np.zeros((M, ncap), np.uint8) if want_states else None
    n_rec, n_ev, t_fin, n_exit = np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1), np.zeros(1, np.int32)
    exits = np.zeros((ncap, 3))
    ms = C.c_double()
    rc = lib.gil_run_large(C.byref(par), n0, _p(pos0), _p(sg0), _p(bd0), _p(uniforms), _p(pos_obs), _p(sg_obs), _p(fl_obs), _p(n_rec),
                           _p(n_ev), _p(t_fin), _p(exits), _p(n_exit), C.byref(ms))
    if rc != 0:
        raise capi.ApsError(rc, lib.gil_large_last_error().decode())
    return dict(pos=pos_obs, sigma=sg_obs, flags=fl_obs, n_recorded=int(n_rec[0]), n_events=int(n_ev[0]), t_final=float(t_fin[0]),
                exits=exits, n_exits=int(n_exit[0]), n0=n0, kernel_ms=ms.value)
