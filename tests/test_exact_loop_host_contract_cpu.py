"""CPU suite: the host-side contract of the exact event loop's C ABI, case by case -- the return code of a call, and either every
field of the plan it fills or the exact text of the entry point's *_last_error.  The plans (gilm_plan, gils_plan, gilc_plan,
gilp_plan, gilx_plan, gilxs_plan) are host arithmetic; the ten run functions are walked through every refusal they make before
they ask for a device, and a valid call stops at GIL_ERR_NODEVICE on a machine without a GPU.

The expected values are tests/golden/exact_loop_host_contract.json, recorded from the library as it was BEFORE the run functions
shared one call record and one staging path:

    APS_LIB=<that build's libaps_hip.so> python tests/test_exact_loop_host_contract_cpu.py --record

The case list is CASES below; the fixture holds nothing but names and recorded results."""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"
FIXTURE = os.path.join(ROOT, "tests", "golden", "exact_loop_host_contract.json")
ERR_NODEVICE = -4
GILM_MAX_SYSTEMS = 65535

capi = importlib.import_module(PKG + ".capi")
gil = importlib.import_module(PKG + ".gillespie")

LAST_ERROR = {"gil_run_batch": "gil_last_error", "gil_run_large": "gil_large_last_error", "gilm": "gilm_last_error", "gils": "gils_last_error",
              "gilc": "gilc_last_error", "gilp": "gilp_last_error", "gilx": "gilx_last_error", "gilxs": "gilxs_last_error",
              "gilr": "gilr_last_error", "gilrm": "gilr_last_error"}


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Call:
    """The arguments of one call, with the arrays they point to kept alive.  Keywords: fields of gil_params, and
    n0 / pos / sigma (the start states, [S][n_cap]), null=<name of a required pointer to pass as NULL>, flip (a flip table)."""

    def __init__(self, **kw):
        S, N = kw.get("n_systems", 2), kw.get("n_cap", 4)
        arrays = min(max(S, 1), 8)                             # systems the arrays describe (a refusal on n_systems reads none)
        self.keep = keep = {}
        keep["beta"] = np.full(arrays, 0.5)
        keep["times"] = np.arange(max(1, min(kw.get("n_obs", 2), 8))) * 0.01
        keep["n0"] = np.asarray(kw.pop("n0", [min(2, max(N, 0))] * arrays), np.int32)
        pos = np.zeros((arrays, max(N, 1)), np.int32)
        pos[:, 1:2] = 1                                        # two particles a system, on sites 0 and 1
        keep["pos"] = np.ascontiguousarray(kw.pop("pos", pos), np.int32)
        keep["sigma"] = np.ascontiguousarray(kw.pop("sigma", np.ones((arrays, max(N, 1)), np.int8)), np.int8)
        self.null = kw.pop("null", None)
        flip = kw.pop("flip", None)
        fields = dict(L=64, K=1, periodic=1, n_systems=2, n_cap=4, n_obs=2, sigma_grid=0.0, rate_diffusion=0.1, rate_active=1.0, T=0.01,
                      max_events=16, ref_obs=-1)
        fields.update(kw)
        if flip is not None:
            keep["flip"] = np.ascontiguousarray(flip, np.float64)
            fields.update(flip_n=keep["flip"].shape[1] - 1, flip_table=_ptr(keep["flip"]).value)
        self.par = gil.GilParams(beta=None if self.null == "beta" else _ptr(keep["beta"]).value,
                                 times_obs=None if self.null == "times_obs" else _ptr(keep["times"]).value, **fields)
        self.ms = C.c_double()
        keep["out"] = np.zeros(1 << 16, np.uint8)              # every output of a call that is refused or finds no device: never written

    def p(self):
        return None if self.null == "p" else C.byref(self.par)

    def start(self):
        k = self.keep
        return [None if self.null == n else _ptr(k[n]) for n in ("n0", "pos", "sigma")] + [None, None]   # bound0, uniforms

    def outputs(self, n=9):
        return [_ptr(self.keep["out"])] * n

    def extra(self, name):
        return None if self.null == name else _ptr(self.keep["out"])


def _variants(c, sigma_grid=(0.0, 2.0), n_variants=None, variant_of_system=None, order=None, null=None):
    k = c.keep
    k["v_sigma"] = np.asarray(sigma_grid, np.float64)
    k["v_of"] = np.asarray(np.arange(max(c.par.n_systems, 8)) % 2 if variant_of_system is None else variant_of_system, np.int32)
    k["v_order"] = None if order is None else np.asarray(order, np.int32)
    k["v"] = gil.GilxVariants(n_variants=len(sigma_grid) if n_variants is None else n_variants,
                              sigma_grid=None if null == "sigma_grid" else _ptr(k["v_sigma"]).value,
                              variant_of_system=None if null == "variant_of_system" else _ptr(k["v_of"]).value,
                              order=None if order is None else _ptr(k["v_order"]).value)
    return None if null == "v" else C.byref(k["v"])


def _info(info):
    return {name: int(getattr(info, name)) for name, _ in info._fields_}


def _result(lib, family, rc, info=None):
    if rc == 0:
        return {"rc": 0, "info": _info(info)} if info is not None else {"rc": 0}
    return {"rc": int(rc), "error": getattr(lib, LAST_ERROR[family])().decode()}


# ---- the entry points: each takes the library and the case's keywords and returns {"rc", "info" | "error"}

def gilm_plan(lib, want_states=1, want_scalars=1, null=None, **kw):
    c, info = Call(null=null, **kw), gil.GilmPlanInfo()
    return _result(lib, "gilm", lib.gilm_plan(c.p(), want_states, want_scalars, None if null == "out" else C.byref(info)), info)


def gils_plan(lib, k_max=4, first_obs=0, want_states=1, null=None, **kw):
    c, info = Call(null=null, **kw), gil.GilsPlanInfo()
    return _result(lib, "gils", lib.gils_plan(c.p(), k_max, first_obs, want_states, None if null == "out" else C.byref(info)), info)


def gilc_plan(lib, n_groups=0, c_bins=8, h_bins=8, first_obs=0, want_states=1, null=None, **kw):
    c, info = Call(null=null, **kw), gil.GilcPlanInfo()
    return _result(lib, "gilc", lib.gilc_plan(c.p(), n_groups, c_bins, h_bins, first_obs, want_states, None if null == "out" else C.byref(info)), info)


def gilp_plan(lib, n_bins=8, n_groups=1, first_obs=0, want_field=0, want_states=1, want_per_system=0, null=None, **kw):
    c, info = Call(null=null, **kw), gil.GilpPlanInfo()
    return _result(lib, "gilp", lib.gilp_plan(c.p(), n_bins, n_groups, first_obs, want_field, want_states, want_per_system,
                                              None if null == "out" else C.byref(info)), info)


def gilx_plan(lib, want_states=1, null=None, variants=None, **kw):
    c, info = Call(null=null, **kw), gil.GilxPlanInfo()
    v = _variants(c, null=null, **(variants or {}))
    return _result(lib, "gilx", lib.gilx_plan(c.p(), v, want_states, None if null == "out" else C.byref(info)), info)


def gilxs_plan(lib, k_max=4, first_obs=0, want_states=1, want_rows=1, null=None, variants=None, **kw):
    c, info = Call(null=null, **kw), capi.GilxsPlanInfo()
    v = _variants(c, null=null, **(variants or {}))
    return _result(lib, "gilxs", lib.gilxs_plan(c.p(), v, k_max, first_obs, want_states, want_rows, None if null == "out" else C.byref(info)), info)


def gil_run_batch(lib, **kw):
    c = Call(**kw)
    return _result(lib, "gil_run_batch", lib.gil_run_batch(c.p(), *c.start(), *c.outputs(), C.byref(c.ms)))


def gil_run_large(lib, n0=2, **kw):
    c = Call(**dict(dict(n_systems=1), **kw))
    s = c.start()
    return _result(lib, "gil_run_large", lib.gil_run_large(c.p(), n0, *s[1:], *c.outputs(8), C.byref(c.ms)))


def gilm_run(lib, **kw):
    c = Call(**kw)
    return _result(lib, "gilm", lib.gilm_run(c.p(), *c.start(), *c.outputs(), C.byref(c.ms)))


def gils_run(lib, k_max=4, first_obs=0, **kw):
    c = Call(**kw)
    return _result(lib, "gils", lib.gils_run(c.p(), k_max, first_obs, *c.start(), *c.outputs(), c.extra("structure_obs"), C.byref(c.ms)))


def gilc_run(lib, n_groups=0, c_bins=8, h_bins=8, h_dt=0.1, first_obs=0, group_of_site=None, anchor=None, **kw):
    c = Call(**kw)
    groups = None if group_of_site is None else np.asarray(group_of_site, np.int32)
    if anchor is not None:
        c.keep["anchor"] = np.asarray(anchor, np.uint8)
        c.par.anchor_mask = _ptr(c.keep["anchor"]).value
    return _result(lib, "gilc", lib.gilc_run(c.p(), _ptr(groups), n_groups, c_bins, h_bins, h_dt, first_obs, *c.start(), *c.outputs(),
                                             c.extra("capture_obs"), c.extra("life_hist"), c.extra("life_sums"), C.byref(c.ms)))


def gilp_run(lib, n_bins=8, first_obs=0, want_field=0, group_of_system=None, n_groups=1, **kw):
    c = Call(**kw)
    groups = None if group_of_system is None else np.asarray(group_of_system, np.int32)
    return _result(lib, "gilp", lib.gilp_run(c.p(), n_bins, first_obs, want_field, _ptr(groups), n_groups, *c.start(), *c.outputs(),
                                             c.extra("ensemble_sums"), c.extra("members"), None, C.byref(c.ms)))


def gilx_run(lib, variants=None, **kw):
    c = Call(**kw)
    v = _variants(c, null=c.null, **(variants or {}))
    return _result(lib, "gilx", lib.gilx_run(c.p(), v, *c.start(), *c.outputs(), C.byref(c.ms)))


def gilxs_run(lib, k_max=4, first_obs=0, variants=None, **kw):
    c = Call(**kw)
    v = _variants(c, null=c.null, **(variants or {}))
    return _result(lib, "gilxs", lib.gilxs_run(c.p(), v, k_max, first_obs, *c.start(), *c.outputs(), None, c.extra("head_obs"), c.extra("window"),
                                               c.extra("n_window"), c.extra("n_empty"), C.byref(c.ms)))


def _resumable(entry, family):
    def run(lib, obs_first=0, checkpoint=None, **kw):
        """checkpoint: None (a fresh start), or keywords that overwrite entries of a valid checkpoint of the call's systems"""
        c = Call(**kw)
        S, N = c.par.n_systems, c.par.n_cap
        ck = None
        if checkpoint is not None:
            arr = dict(pos=np.zeros((S, N), np.int32), flags=np.zeros((S, N), np.uint8), ref=np.full((S, N), -1, np.int32), t=np.zeros(S),
                       n_events=np.zeros(S, np.int64), next_obs=np.zeros(S, np.int32))
            arr["pos"][:, 1], arr["flags"][:, :2] = 1, 5
            null = checkpoint.pop("null", None)
            for name, (index, value) in checkpoint.items():
                arr[name][index] = value
            c.keep["ck"] = arr
            ck = gil.GilCheckpoint(**{k: None if k == null else _ptr(v).value for k, v in arr.items()})
        rc = getattr(lib, entry)(c.p(), *c.start(), *c.outputs(), C.byref(c.ms), obs_first, None if ck is None else C.byref(ck), None)
        return _result(lib, family, rc)
    return run


gilr_run, gilrm_run = _resumable("gilr_run", "gilr"), _resumable("gilrm_run", "gilrm")

# ---- the cases

BIG_L = dict(L=4200, n_cap=64)                  # beyond GIL_MAX_L: the large shape
BIG_N = dict(L=4096, n_cap=2049)                # beyond GIL_MAX_N: the large shape
TOO_MANY = dict(n_systems=GILM_MAX_SYSTEMS + 1)
HUGE = dict(n_systems=1 << 20, n_obs=1 << 14)   # batch shape, more than 2^38 bytes of states
TWICE = np.array([[0, 0, 0, 0], [0, 1, 0, 0]])  # K = 1: two particles on site 0 of system 0
BAD_FLIP = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, 1.0]])

CASES = []


def case(name, fn, **kw):
    CASES.append((name, fn, kw))


# plans: the shapes
for tag, fn, extra in (("gils_plan", gils_plan, {}), ("gilc_plan", gilc_plan, {}), ("gilp_plan", gilp_plan, {})):
    case(f"{tag}-batch-64-threads", fn, L=256, n_cap=1024, **extra)
    case(f"{tag}-batch-256-threads", fn, L=2048, n_cap=1030, **extra)
    case(f"{tag}-large-by-L", fn, **BIG_L)
    case(f"{tag}-large-by-n_cap", fn, **BIG_N)
    case(f"{tag}-large-field-table", fn, sigma_grid=40.0, K=2, **BIG_L)
for tag, fn in (("gilx_plan", gilx_plan), ("gilxs_plan", gilxs_plan)):
    case(f"{tag}-batch-64-threads", fn, L=256, n_cap=1024)
    case(f"{tag}-batch-256-threads", fn, L=2048, n_cap=1030)
    case(f"{tag}-no-states", fn, L=256, n_cap=64, want_states=0, n_systems=8)
case("gilxs_plan-no-rows", gilxs_plan, L=256, n_cap=64, want_rows=0)
case("gilm_plan-large-by-L", gilm_plan, **BIG_L)
case("gilm_plan-large-by-n_cap", gilm_plan, **BIG_N)
case("gilm_plan-small-system", gilm_plan, L=64, n_cap=4)
case("gilm_plan-no-states-no-scalars", gilm_plan, want_states=0, want_scalars=0, **BIG_L)
case("gilm_plan-table-in-lds", gilm_plan, sigma_grid=40.0, **BIG_L)
case("gilm_plan-table-in-global-memory", gilm_plan, L=1 << 20, n_cap=1000, sigma_grid=4000.0)
case("gils_plan-phase-table-in-lds", gils_plan, L=1024, n_cap=256, k_max=64)
case("gils_plan-phase-table-does-not-fit", gils_plan, L=4096, n_cap=1030, k_max=64)
case("gils_plan-first_obs-no-states", gils_plan, L=512, n_cap=100, k_max=512, first_obs=2, want_states=0)
case("gilxs_plan-phase-table-in-lds", gilxs_plan, L=1024, n_cap=256, k_max=64)
case("gilxs_plan-phase-table-does-not-fit", gilxs_plan, L=4096, n_cap=1030, k_max=64)
case("gilc_plan-groups", gilc_plan, L=512, n_cap=100, n_groups=3, c_bins=16, h_bins=40)
case("gilc_plan-groups-large", gilc_plan, n_groups=3, c_bins=16, h_bins=40, **BIG_L)
case("gilp_plan-field-per-system", gilp_plan, L=1000, n_cap=500, n_bins=100, n_groups=4, want_field=1, want_per_system=1)
case("gilp_plan-field-large", gilp_plan, n_bins=1024, want_field=1, **BIG_L)
# plans: refused for LDS
case("gilx_plan-largest-lds", gilx_plan, L=4096, n_cap=2048, periodic=0, variants=dict(sigma_grid=(0.0, 1100.0)))   # the largest there is: fits
case("gilxs_plan-lds-with-structure", gilxs_plan, L=4096, n_cap=2048, periodic=0, variants=dict(sigma_grid=(0.0, 1100.0)))
case("gilm_plan-largest-lds", gilm_plan, L=1 << 20, n_cap=1 << 20, sigma_grid=1500.0)
case("gilc_plan-large-near-the-lds-limit", gilc_plan, L=1 << 20, n_cap=1 << 20, sigma_grid=1500.0, n_groups=32, c_bins=64, h_bins=256)
case("gilp_plan-lds-large", gilp_plan, L=1 << 20, n_cap=1 << 20, sigma_grid=1500.0, n_bins=1024, want_field=1)
case("gils_plan-large-near-the-lds-limit", gils_plan, L=1 << 20, n_cap=1 << 20, sigma_grid=1500.0)
# plans: refused for the 2^38 bytes
case("gilm_plan-2^38", gilm_plan, n_systems=1, n_obs=1 << 26, **BIG_N)
for tag, fn in (("gils_plan", gils_plan), ("gilc_plan", gilc_plan), ("gilp_plan", gilp_plan), ("gilxs_plan", gilxs_plan)):
    case(f"{tag}-2^38", fn, **HUGE)
case("gils_plan-2^38-large", gils_plan, n_systems=1, n_obs=1 << 26, **BIG_N)
# plans: every argument refusal
for tag, fn in (("gilm_plan", gilm_plan), ("gils_plan", gils_plan), ("gilc_plan", gilc_plan), ("gilp_plan", gilp_plan), ("gilx_plan", gilx_plan),
                ("gilxs_plan", gilxs_plan)):
    case(f"{tag}-null-p", fn, null="p")
    case(f"{tag}-null-out", fn, null="out")
    case(f"{tag}-L-1", fn, L=1)
    case(f"{tag}-K-0", fn, K=0)
    case(f"{tag}-K-33", fn, K=33)
    case(f"{tag}-n_systems-0", fn, n_systems=0)
    case(f"{tag}-n_cap-0", fn, n_cap=0)
    case(f"{tag}-n_obs-0", fn, n_obs=0)
    case(f"{tag}-max_events-negative", fn, max_events=-1)
for tag, fn in (("gilm_plan", gilm_plan), ("gils_plan", gils_plan), ("gilc_plan", gilc_plan), ("gilp_plan", gilp_plan)):
    case(f"{tag}-too-many-systems", fn, **TOO_MANY, **BIG_L)
    case(f"{tag}-L-beyond-2^25", fn, L=(1 << 25) + 1, n_cap=64)
    case(f"{tag}-K-33-large", fn, K=33, **BIG_L)
    case(f"{tag}-site-map", fn, L=1 << 24, K=16, n_cap=64)
    case(f"{tag}-n_cap-beyond-blocks", fn, L=4200, n_cap=(1 << 20) + 1)
for tag, fn in (("gils_plan", gils_plan), ("gilxs_plan", gilxs_plan)):
    case(f"{tag}-k_max-0", fn, k_max=0)
    case(f"{tag}-k_max-beyond-L", fn, k_max=65)
    case(f"{tag}-first_obs-negative", fn, first_obs=-1)
    case(f"{tag}-first_obs-beyond", fn, first_obs=3)
case("gils_plan-k_max-beyond-GILS_MAX_K", gils_plan, k_max=4097, L=8000)
case("gilc_plan-n_groups-negative", gilc_plan, n_groups=-1)
case("gilc_plan-n_groups-33", gilc_plan, n_groups=33)
case("gilc_plan-c_bins-1", gilc_plan, c_bins=1)
case("gilc_plan-c_bins-65", gilc_plan, c_bins=65)
case("gilc_plan-h_bins-0", gilc_plan, h_bins=0)
case("gilc_plan-h_bins-257", gilc_plan, h_bins=257)
case("gilc_plan-first_obs-negative", gilc_plan, first_obs=-1)
case("gilc_plan-first_obs-beyond", gilc_plan, first_obs=3)
case("gilc_run-h_dt-zero", gilc_run, h_dt=0.0)
case("gilc_run-h_dt-inf", gilc_run, h_dt=float("inf"))
case("gilc_run-h_dt-nan", gilc_run, h_dt=float("nan"))
case("gilc_run-group-id-out-of-range", gilc_run, n_groups=2, group_of_site=[-1] * 10 + [2] + [-1] * 53, anchor=[1] * 64)
case("gilc_run-group-id-below", gilc_run, n_groups=2, group_of_site=[-2] + [-1] * 63, anchor=[1] * 64)
case("gilc_run-group-without-anchor", gilc_run, n_groups=2, group_of_site=[-1] * 5 + [1] + [-1] * 58, anchor=[0] * 5 + [0] + [1] * 58)
case("gilc_run-group-without-anchor-mask", gilc_run, n_groups=2, group_of_site=[0] + [-1] * 63)
case("gilp_plan-n_bins-0", gilp_plan, n_bins=0)
case("gilp_plan-n_bins-beyond-L", gilp_plan, n_bins=65)
case("gilp_plan-n_bins-beyond-GILP_MAX_BINS", gilp_plan, n_bins=1025, **BIG_L)
case("gilp_plan-n_groups-0", gilp_plan, n_groups=0)
case("gilp_plan-n_groups-4097", gilp_plan, n_groups=4097)
case("gilp_plan-first_obs-negative", gilp_plan, first_obs=-1)
case("gilp_plan-first_obs-beyond", gilp_plan, first_obs=3)
case("gilp_plan-want_field-2", gilp_plan, want_field=2)
case("gilp_plan-want_field-overflow", gilp_plan, want_field=1, L=1 << 16, n_systems=1 << 15, n_cap=64)
case("gilp_run-group-id-out-of-range", gilp_run, n_groups=2, group_of_system=[0, 2])
case("gilp_run-group-id-negative", gilp_run, n_groups=2, group_of_system=[-1, 0])
for tag, fn in (("gilx_plan", gilx_plan), ("gilxs_plan", gilxs_plan)):
    case(f"{tag}-null-v", fn, null="v")
    case(f"{tag}-L-beyond-GIL_MAX_L", fn, **BIG_L)
    case(f"{tag}-n_cap-beyond-GIL_MAX_N", fn, **BIG_N)
    case(f"{tag}-n_variants-0", fn, variants=dict(n_variants=0))
    case(f"{tag}-n_variants-4097", fn, variants=dict(n_variants=4097))
    case(f"{tag}-null-sigma_grid", fn, null="sigma_grid")
    case(f"{tag}-sigma_grid-negative", fn, variants=dict(sigma_grid=(0.0, -1.0)))
    case(f"{tag}-sigma_grid-nan", fn, variants=dict(sigma_grid=(float("nan"), 1.0)))
    case(f"{tag}-variant-index", fn, variants=dict(variant_of_system=[0, 2]))
    case(f"{tag}-variant-index-negative", fn, variants=dict(variant_of_system=[-1, 0]))
    case(f"{tag}-order-outside", fn, variants=dict(order=[0, 2]))
    case(f"{tag}-order-twice", fn, variants=dict(order=[1, 1]))
    case(f"{tag}-order-valid", fn, variants=dict(order=[1, 0]))

# the run functions
RUNS = (("gil_run_batch", gil_run_batch, {}), ("gil_run_large", gil_run_large, {}), ("gilm_run", gilm_run, {}), ("gils_run", gils_run, {}),
        ("gilc_run", gilc_run, {}), ("gilp_run", gilp_run, {}), ("gilx_run", gilx_run, {}), ("gilxs_run", gilxs_run, {}), ("gilr_run", gilr_run, {}),
        ("gilrm_run", gilrm_run, {}))
REQUIRED = {"gils_run": ("structure_obs",), "gilc_run": ("capture_obs", "life_hist", "life_sums"), "gilp_run": ("ensemble_sums", "members"),
            "gilx_run": ("v", "variant_of_system"), "gilxs_run": ("v", "variant_of_system", "head_obs", "window", "n_window", "n_empty")}
for tag, fn, extra in RUNS:
    for name in ("p", "pos", "sigma", "beta", "times_obs") + (() if tag == "gil_run_large" else ("n0",)) + REQUIRED.get(tag, ()):
        case(f"{tag}-null-{name}", fn, null=name)
    if tag == "gil_run_large":
        case(f"{tag}-n0-negative", fn, n0=-1)
        case(f"{tag}-n0-beyond-n_cap", fn, n0=5)
        case(f"{tag}-two-systems", fn, n_systems=2)
    else:
        case(f"{tag}-n0-negative", fn, n0=[2, -1])
        case(f"{tag}-n0-beyond-n_cap", fn, n0=[5, 2])
    case(f"{tag}-position-outside", fn, pos=[[0, 64, 0, 0], [0, 1, 0, 0]])
    case(f"{tag}-position-negative", fn, pos=[[0, -1, 0, 0], [0, 1, 0, 0]])
    case(f"{tag}-site-capacity", fn, pos=TWICE)
    case(f"{tag}-sigma-zero", fn, sigma=[[1, 0, 1, 1], [1, 1, 1, 1]])
    case(f"{tag}-flip-table-negative-rate", fn, flip=BAD_FLIP)
    case(f"{tag}-flip-table-nan", fn, flip=np.array([[1.0, 1.0], [np.nan, 1.0]]))
    case(f"{tag}-flip_n-0", fn, flip=np.ones((2, 2)), flip_n=0)
    case(f"{tag}-L-1", fn, L=1)
    case(f"{tag}-K-0", fn, K=0)
    case(f"{tag}-K-33", fn, K=33)
    case(f"{tag}-n_systems-0", fn, n_systems=0)
    case(f"{tag}-n_cap-0", fn, n_cap=0)
    case(f"{tag}-n_obs-0", fn, n_obs=0)
    case(f"{tag}-max_events-negative", fn, max_events=-1)
    case(f"{tag}-valid", fn)
    case(f"{tag}-valid-flip-table", fn, flip=np.ones((2, 9)))
for tag, fn in (("gil_run_batch", gil_run_batch), ("gilx_run", gilx_run), ("gilxs_run", gilxs_run), ("gilr_run", gilr_run)):
    case(f"{tag}-L-beyond-GIL_MAX_L", fn, **BIG_L)
    case(f"{tag}-n_cap-beyond-GIL_MAX_N", fn, **BIG_N)
for tag, fn in (("gilm_run", gilm_run), ("gils_run", gils_run), ("gilc_run", gilc_run), ("gilp_run", gilp_run), ("gilrm_run", gilrm_run)):
    case(f"{tag}-too-many-systems", fn, **TOO_MANY, **BIG_L)
    case(f"{tag}-large-valid", fn, **BIG_L)
    case(f"{tag}-large-valid-by-n_cap", fn, **BIG_N)
    case(f"{tag}-large-n0-beyond-n_cap", fn, n0=[65, 2], **BIG_L)
    case(f"{tag}-large-site-capacity", fn, pos=np.zeros((2, 64), np.int32), **BIG_L)
    case(f"{tag}-large-flip-table-negative-rate", fn, flip=BAD_FLIP, **BIG_L)
    case(f"{tag}-large-L-beyond-2^25", fn, L=(1 << 25) + 1, n_cap=64)
case("gil_run_large-large-valid", gil_run_large, **BIG_L)
case("gil_run_large-L-beyond-2^25", gil_run_large, L=(1 << 25) + 1, n_cap=64)
for tag, fn in (("gils_run", gils_run), ("gilxs_run", gilxs_run)):
    case(f"{tag}-k_max-0", fn, k_max=0)
    case(f"{tag}-first_obs-beyond", fn, first_obs=3)
case("gilx_run-variant-index", gilx_run, variants=dict(variant_of_system=[0, 2]))
case("gilx_run-order-twice", gilx_run, variants=dict(order=[1, 1]))
case("gilxs_run-order-outside", gilxs_run, variants=dict(order=[0, 2]))
# the resumable launches: gilr_prepare's refusals, with and without a checkpoint
for tag, fn, shape in (("gilr_run", gilr_run, {}), ("gilrm_run", gilrm_run, {}), ("gilrm_run-large", gilrm_run, BIG_L)):
    case(f"{tag}-obs_first-negative", fn, obs_first=-1, **shape)
    case(f"{tag}-checkpoint-valid", fn, checkpoint={}, **shape)
    case(f"{tag}-checkpoint-without-start-state", fn, checkpoint={}, null="n0", **shape)
    case(f"{tag}-checkpoint-null-array", fn, checkpoint=dict(null="ref"), **shape)
    case(f"{tag}-checkpoint-position-outside", fn, checkpoint=dict(pos=((1, 0), shape.get("L", 64))), **shape)
    case(f"{tag}-checkpoint-origin-outside", fn, checkpoint=dict(ref=((0, 1), -2)), **shape)
    case(f"{tag}-checkpoint-unknown-flag", fn, checkpoint=dict(flags=((0, 3), 8)), **shape)
    case(f"{tag}-checkpoint-site-capacity", fn, checkpoint=dict(pos=((0, 1), 0)), **shape)
    case(f"{tag}-checkpoint-negative-time", fn, checkpoint=dict(t=(1, -1.0)), **shape)
    case(f"{tag}-checkpoint-nan-time", fn, checkpoint=dict(t=(0, float("nan"))), **shape)
    case(f"{tag}-checkpoint-negative-events", fn, checkpoint=dict(n_events=(0, -1)), **shape)
    case(f"{tag}-checkpoint-next_obs-beyond", fn, checkpoint=dict(next_obs=(1, 5)), obs_first=2, **shape)
    case(f"{tag}-checkpoint-next_obs-before-obs_first", fn, checkpoint=dict(next_obs=(0, 1)), obs_first=2, **shape)
    case(f"{tag}-checkpoint-ended-before-obs_first", fn, checkpoint=dict(next_obs=(0, 1), t=(0, float("inf"))), obs_first=2, **shape)
    case(f"{tag}-checkpoint-flip-table-negative-rate", fn, checkpoint={}, flip=BAD_FLIP, **shape)

assert len({name for name, _, _ in CASES}) == len(CASES), "case names must be unique"


def run_case(lib, fn, kw):
    kw = {k: (dict(v) if isinstance(v, dict) else v) for k, v in kw.items()}        # a case may run twice: hand it its own dictionaries
    return fn(lib, **kw)


@pytest.fixture(scope="module")
def lib():
    return gil._lib()


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_and_case_list_agree(recorded):
    assert sorted(recorded) == sorted(name for name, _, _ in CASES)


@pytest.mark.parametrize("name,fn,kw", CASES, ids=[name for name, _, _ in CASES])
def test_host_contract(lib, recorded, name, fn, kw):
    want = recorded[name]
    if want["rc"] == ERR_NODEVICE and capi.device_count() > 0:
        pytest.skip("GPU present: the call would run")
    got = run_case(lib, fn, kw)
    assert got["rc"] == want["rc"], got
    assert sorted(got) == sorted(want)
    if "info" in want:
        for field, value in want["info"].items():
            assert got["info"][field] == value, (field, got["info"])
        assert sorted(got["info"]) == sorted(want["info"])
    if "error" in want:
        assert got["error"] == want["error"]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: APS_LIB=<the build to record from> python tests/test_exact_loop_host_contract_cpu.py --record")
    if capi.device_count() > 0:
        sys.exit("record on a machine without a GPU: the valid calls must stop at GIL_ERR_NODEVICE")
    out = {name: run_case(gil._lib(), fn, kw) for name, fn, kw in CASES}
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cases recorded from {capi.LIB_PATH} into {FIXTURE}")
