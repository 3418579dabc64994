"""CPU suite: the Python side of the exact event loop (gillespie.py), call by call -- what every public function hands to the C
entry points and what it makes of what they return.

`gillespie._lib` is replaced by a stand-in whose `*_run` attributes are Python callables.  For every call the stand-in notes
the entry's name and the number of arguments, every scalar field of gil_params, every scalar argument and, for every pointer,
either NULL or a CRC of the bytes it must point to; the extents are restated here from the headers (n_systems, n_cap, n_obs, L,
K, flip_n, the variant count), and the bytes are read inside the stand-in after a gc.collect(): an array that nothing keeps alive
until the C call returns shows as other bytes.  The arrays behind gilx_variants, gil_checkpoint and gilx_checkpoint (its six
base arrays, n_slots and, with k_max > 0, the window sums) are read the same way.  The
stand-in then fills the outputs from a generator seeded by the case's name with values a launch could return (n_recorded =
n_obs, positions in [0, L), flags with the alive bit, next_obs at the segment's end, finite sums; in a gilx_checkpoint n_slots
as they came in, or n0 on a fresh start, a positive window, n_window = the window's observations up to the segment's end and
n_empty = 0), so that the post-processing runs.  The plans go to the real library: they are host arithmetic.

Recorded per case, and compared for equality (no tolerance; arrays by CRC of their bytes, so NaNs compare by bits): the calls,
the returned structure or the exception's type and text, and per system n_events, kernel_ms, bytes_back and the state of
rng.bit_generator after the call.

The expected values are tests/golden/exact_loop_python_contract.json, recorded from gillespie.py and particle_system.py of
commit 9100240, the parent of the commit that added this file (there every entry point wrote its launch keywords, its batch
opening and its C call out for itself), by this file's own

    python tests/test_exact_loop_python_contract_cpu.py --record      (run in a checkout of 9100240 that holds a copy of this file)

The cases of the large mixed launch, of the mixed checkpoints and segment chains and of their raw functions (gilxm_run,
gilxr_run, gilxmr_run, gilxsr_run, MixedCheckpoint, plan_mixed_many; NEWER below) were recorded the same way from commit
5dbba22, where the mixed chain stood beside the mixed launch and the plain chain as a copy of both; every older entry came out
of that recording byte for byte as 9100240 had given it.

The case list is CASES below; the fixture holds nothing but names and recorded results (CRCs and texts).  Where a case asks
for a number that the library refuses on the host before it looks for a device (n_bins = 0, k_max = 0, h_bins = 0), the
stand-in notes the call and hands it on to the real library (`ask_library`), so that the refusal and its text are the library's
own.  No shape the mixed kernels accept is over the LDS limit of a mixed launch (the largest, L = 4096, N = 2048 with the longest
table, fits: `gilx_plan-largest-lds` of test_exact_loop_host_contract_cpu.py), so the cases of that refusal lower the limit."""
import ctypes as C
import gc
import importlib
import json
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"
FIXTURE = os.path.join(ROOT, "tests", "golden", "exact_loop_python_contract.json")

capi = importlib.import_module(PKG + ".capi")
gil = importlib.import_module(PKG + ".gillespie")
psm = importlib.import_module(PKG + ".particle_system")
ParticleSystem = psm.ParticleSystem


# ---- digests

def crc_bytes(b):
    return f"{zlib.crc32(b):08x}"


def crc_json(x):
    return crc_bytes(json.dumps(x, sort_keys=True).encode())


def digest(x):
    """A structure of dicts, lists, arrays and scalars as JSON: a CRC (with dtype and shape) per array, repr for scalars."""
    if isinstance(x, gil.MixedCheckpoint):
        return {"MixedCheckpoint": digest({**x.arrays(), **x.fingerprint(), "block_tables": x.block_tables})}
    if isinstance(x, gil.Checkpoint):
        return {"Checkpoint": digest({**x.arrays(), **x.fingerprint()})}
    if isinstance(x, dict):
        return {str(k): digest(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [digest(v) for v in x]
    if isinstance(x, (np.ndarray, np.generic)):
        a = np.ascontiguousarray(x)
        return f"{a.dtype.str}{list(a.shape)}:{crc_bytes(a.tobytes())}"
    return repr(x)


# ---- the C ABI as the headers state it: the arguments of every entry point, and the extents of what they point to

IN = {"n0": ("<i4", "S"), "pos0": ("<i4", "S,N"), "sigma0": ("|i1", "S,N"), "bound0": ("|u1", "S,N"), "uniforms": ("<f8", "S,E,4"),
      "group_of_site": ("<i4", "L"), "group_of_system": ("<i4", "S"),
      "large_pos0": ("<i4", "n0"), "large_sigma0": ("|i1", "n0"), "large_bound0": ("|u1", "n0"), "large_uniforms": ("<f8", "E,4")}
PAR_POINTERS = {"beta": ("<f8", "S"), "anchor_mask": ("|u1", "L"), "times_obs": ("<f8", "M"), "front_lo": ("<i4", "L"),
                "block_table": ("|u1", "(K+1)*(K+1)"), "flip_table": ("<f8", "2*(F+1)")}
VARIANT_POINTERS = {"sigma_grid": ("<f8", "V"), "block_table": ("|u1", "V*(K+1)*(K+1)"), "variant_of_system": ("<i4", "S"),
                    "seed": ("<u8", "S"), "stream": ("<i4", "S"), "order": ("<i4", "S")}
CHECKPOINT_POINTERS = {"pos": ("<i4", "S,N"), "flags": ("|u1", "S,N"), "ref": ("<i4", "S,N"), "t": ("<f8", "S"), "n_events": ("<i8", "S"),
                       "next_obs": ("<i4", "S")}
MIXED_CHECKPOINT_POINTERS = {"n_slots": ("<i4", "S"), "window": ("<f8", "S,k_max,3"), "n_window": ("<i4", "S"), "n_empty": ("<i4", "S")}


def _scalars(g, c, shape):
    """The twelve sums of gillespie.SCALARS per observation, as a launch without exits could return them."""
    a = np.zeros(shape, np.int64)
    N, L = c["N"], c["L"]
    a[..., 0], a[..., 1], a[..., 2] = N, g.integers(-N, N + 1, shape[:2]), g.integers(0, N * L, shape[:2])
    a[..., 3], a[..., 4], a[..., 5] = g.integers(0, 3, shape[:2]), g.integers(0, L, shape[:2]), g.integers(0, N + 1, shape[:2])
    a[..., 6], a[..., 7], a[..., 8] = g.integers(10, 100, shape[:2]), g.integers(0, 10, shape[:2]), g.integers(-50, 50, shape[:2])
    a[..., 9], a[..., 10], a[..., 11] = g.integers(100, 1000, shape[:2]), N, g.integers(0, 1000, shape[:2])
    return a


def _short(c):
    """The observations each system stays short of n_obs: in a batch the first system records them all."""
    a = np.full(c["S"], c["short"])
    a[:min(1, c["S"] - 1)] = 0
    return a


def _rows(g, c, shape):
    a = g.random(shape) + 0.5
    a[..., 0] = c["N"]
    return a


def _exits(g, c, shape):
    a = g.random(shape)
    a[..., 1] = g.integers(0, c["L"], shape[:-1])
    return a


OUT = {"pos": ("<i4", "S,M,N", lambda g, c, s: g.integers(0, c["L"], s)),
       "sigma": ("|i1", "S,M,N", lambda g, c, s: g.choice([1, -1], s)),
       "flags": ("|u1", "S,M,N", lambda g, c, s: g.choice([2, 3, 3, 0], s)),                 # 2: alive, 1: bound
       "scalars": ("<i8", "S,M,12", _scalars),
       "n_recorded": ("<i4", "S", lambda g, c, s: c["M"] - _short(c)),
       "n_events": ("<i8", "S", lambda g, c, s: g.integers(100, 1000, s)),
       "t_final": ("<f8", "S", lambda g, c, s: g.random(s) + 1.0),
       "exits": ("<f8", "S,N,3", _exits),
       "n_exits": ("<i4", "S", lambda g, c, s: g.integers(0, min(c["N"], 3) + 1, s)),
       "structure": ("<f8", "S,M,4+2*max(k_max,0)", _rows),
       "head": ("<f8", "S,M,4", _rows),
       "window": ("<f8", "S,max(k_max,0),3", lambda g, c, s: g.random(s) + 0.5),
       "n_window": ("<i4", "S", lambda g, c, s: np.full(s, c["M"] - c["first_obs"])),
       "n_empty": ("<i4", "S", lambda g, c, s: np.zeros(s)),
       "capture": ("<i8", "S,M,9+max(n_groups,0)+max(c_bins,0)", lambda g, c, s: g.integers(0, 50, s)),
       "life_hist": ("<i8", "S,2,max(h_bins,1)", lambda g, c, s: g.integers(0, 20, s)),
       "life_sums": ("<f8", "S,2,2", lambda g, c, s: g.random(s) * 10.0),
       "ensemble_sums": ("<i8", "max(n_groups,1),M,7,max(n_bins,1)", lambda g, c, s: g.integers(0, 40, s)),
       "members": ("<i4", "max(n_groups,1),M", lambda g, c, s: g.integers(2, 4, s)),
       "profile_obs": ("<i4", "S,M,3,max(n_bins,1)", lambda g, c, s: g.integers(0, 3, s))}
START = [("in", k) for k in ("n0", "pos0", "sigma0", "bound0", "uniforms")]
RESULTS = [("out", k) for k in ("pos", "sigma", "flags", "scalars", "n_recorded", "n_events", "t_final", "exits", "n_exits")]
RESUMABLE = ["par"] + START + RESULTS + ["ms", ("int", "obs_first"), "ck_in", "ck_out"]
MIXED_RESUMABLE = ["par", "variants"] + START + RESULTS + ["ms", ("int", "obs_first"), "xck_in", "xck_out"]
ENTRIES = {
    "gil_run_batch": ["par"] + START + RESULTS + ["ms"],
    "gilm_run": ["par"] + START + RESULTS + ["ms"],
    "gilr_run": RESUMABLE,
    "gilrm_run": RESUMABLE,
    "gils_run": ["par", ("int", "k_max"), ("int", "first_obs")] + START + RESULTS + [("out", "structure"), "ms"],
    "gilc_run": ["par", ("in", "group_of_site"), ("int", "n_groups"), ("int", "c_bins"), ("int", "h_bins"), ("float", "h_dt"), ("int", "first_obs")]
                + START + RESULTS + [("out", "capture"), ("out", "life_hist"), ("out", "life_sums"), "ms"],
    "gilp_run": ["par", ("int", "n_bins"), ("int", "first_obs"), ("int", "want_field"), ("in", "group_of_system"), ("int", "n_groups")]
                + START + RESULTS + [("out", "ensemble_sums"), ("out", "members"), ("out", "profile_obs"), "ms"],
    "gilx_run": ["par", "variants"] + START + RESULTS + ["ms"],
    "gilxs_run": ["par", "variants", ("int", "k_max"), ("int", "first_obs")] + START + RESULTS
                 + [("out", k) for k in ("structure", "head", "window", "n_window", "n_empty")] + ["ms"],
    "gilxm_run": ["par", "variants"] + START + RESULTS + ["ms"],
    "gilxr_run": MIXED_RESUMABLE,
    "gilxmr_run": MIXED_RESUMABLE,
    "gilxsr_run": ["par", "variants", ("int", "k_max"), ("int", "first_obs")] + START + RESULTS + [("out", "structure"), ("out", "head")]
                  + ["ms", ("int", "obs_first"), "xck_in", "xck_out"],
    "gil_run_large": ["par", ("int", "n0")] + [("in", "large_" + k) for k in ("pos0", "sigma0", "bound0", "uniforms")]
                     + [("out", k) for k in ("pos", "sigma", "flags", "n_recorded", "n_events", "t_final", "exits", "n_exits")] + ["ms"],
}
LAST_ERROR = {"gil_run_batch": "gil_last_error", "gil_run_large": "gil_large_last_error", "gilm_run": "gilm_last_error", "gils_run": "gils_last_error",
              "gilc_run": "gilc_last_error", "gilp_run": "gilp_last_error", "gilx_run": "gilx_last_error", "gilxs_run": "gilxs_last_error",
              "gilr_run": "gilr_last_error", "gilrm_run": "gilr_last_error", "gilxm_run": "gilxm_last_error", "gilxr_run": "gilxr_last_error",
              "gilxmr_run": "gilxr_last_error", "gilxsr_run": "gilxr_last_error"}


def _address(a):
    if a is None:
        return None
    return a.value if isinstance(a, C.c_void_p) else int(a)


def _shape(text, ctx):
    s = eval(text, {"max": max}, ctx)                          # noqa: S307  (the extents above, on the call's own numbers)
    return s if isinstance(s, tuple) else (s,)


def _read(address, dtype, text, ctx):
    if not address:
        return "NULL"
    shape = _shape(text, ctx)
    return f"{dtype}{list(shape)}:{crc_bytes(C.string_at(address, int(np.prod(shape)) * np.dtype(dtype).itemsize))}"


def _write(address, values, dtype, shape):
    n = int(np.prod(shape))
    if n:
        np.frombuffer((C.c_char * (n * np.dtype(dtype).itemsize)).from_address(address), dtype=dtype)[:] = np.asarray(values).astype(dtype).reshape(-1)


def _struct(obj, pointers, ctx):
    """The scalar fields of a structure by repr, its pointer fields by what they point to."""
    scalars = {f: repr(getattr(obj, f)) for f, t in obj._fields_ if t is not C.c_void_p}
    return scalars, {f: _read(getattr(obj, f), *pointers[f], ctx) for f, t in obj._fields_ if t is C.c_void_p}


def _values(address, dtype, n):
    return np.frombuffer(C.string_at(address, n * np.dtype(dtype).itemsize), dtype=dtype).copy()


def _mixed_checkpoint(obj, ctx):
    """What a gilx_checkpoint to start from points to: the six base arrays, n_slots and, with k_max > 0, the window sums."""
    rec = _struct(obj.base, CHECKPOINT_POINTERS, ctx)[1]
    for k, (dtype, text) in MIXED_CHECKPOINT_POINTERS.items():
        if k == "n_slots" or ctx.get("k_max", 0) > 0:
            rec[k] = _read(getattr(obj, k), dtype, text, ctx)
    return rec


class StandIn:
    """What gillespie._lib() returns during a case.  `rc`: what every run returns (non-zero: nothing is filled); `short`: the
    observations every system but the first of a batch stays short of n_obs; `missing`: attributes the library does not have (an
    older build); `ask_library`: every run, once noted, goes to the real library, which refuses it on the host; `rc_after`: the
    runs that succeed before `rc` sets in."""

    def __init__(self, real, name, rc=0, short=0, missing=(), ask_library=False, rc_after=0):
        self.real, self.rc, self.short, self.missing, self.ask_library, self.rc_after = real, rc, short, missing, ask_library, rc_after
        self.rng = np.random.default_rng(zlib.crc32(name.encode()))
        self.calls = []

    def __getattr__(self, attr):
        if attr.startswith("__") or attr in self.missing:
            raise AttributeError(attr)
        if attr in ENTRIES:
            return lambda *args: self.run(attr, *args)
        if attr in LAST_ERROR.values() and self.rc:
            return lambda: f"{attr}: the stand-in refuses".encode()
        return getattr(self.real, attr)                        # the plans and their refusals: host arithmetic of the real library

    def run(self, entry, *args):
        gc.collect()
        spec = ENTRIES[entry]
        rec = {"entry": entry, "n_args": len(args), "pointers": {}, "scalars": {}}
        if len(args) != len(spec):
            self.calls.append(rec)
            return -1
        par = args[0]._obj
        ctx = dict(S=par.n_systems, N=par.n_cap, M=par.n_obs, L=par.L, K=par.K, E=par.max_events, F=par.flip_n, short=self.short)
        rec["par"], rec["par_pointers"] = _struct(par, PAR_POINTERS, ctx)
        outs, n_slots = [], None
        for what, a in zip(spec[1:], args[1:]):
            if what == "variants":
                ctx["V"] = a._obj.n_variants
                rec["variants"] = _struct(a._obj, VARIANT_POINTERS, ctx)
            elif what == "ck_in":
                rec["ck_in"] = "NULL" if a is None else _struct(a._obj, CHECKPOINT_POINTERS, ctx)[1]
            elif what == "xck_in":                             # the window sums are read where the header has them: with k_max > 0
                rec["ck_in"] = "NULL" if a is None else _mixed_checkpoint(a._obj, ctx)
                n_slots = n0 if a is None or not a._obj.n_slots else _values(a._obj.n_slots, "<i4", ctx["S"])
            elif what in ("ck_out", "xck_out"):
                outs.append((what, a._obj))
            elif what == "ms":
                outs.append(("ms", a._obj))
            elif what[0] in ("int", "float"):
                assert isinstance(a, (int, float)) and not isinstance(a, bool), (entry, what, a)
                ctx[what[1]] = a
                rec["scalars"][what[1]] = repr(a)
            elif what[0] == "in":
                rec["pointers"][what[1]] = _read(_address(a), *IN[what[1]], ctx)
                if what[1] == "n0":
                    n0 = _values(_address(a), "<i4", ctx["S"])
            else:
                rec["pointers"][what[1]] = "NULL" if not _address(a) else "out"
                outs.append((what[1], _address(a)))
        self.calls.append(rec)
        if self.ask_library:
            rc = getattr(self.real, entry)(*args)
            assert rc != 0, f"{entry}: the library accepted what the case expects it to refuse"
            return rc
        if self.rc and len(self.calls) > self.rc_after:
            return self.rc
        for name, target in outs:
            if name == "ms":
                target.value = float(self.rng.integers(1, 1000)) / 8.0
            elif name in ("ck_out", "xck_out"):
                S, N, L = ctx["S"], ctx["N"], ctx["L"]
                more, target = target, target.base if name == "xck_out" else target
                fill = dict(pos=self.rng.integers(0, L, (S, N)), flags=4 | self.rng.integers(0, 4, (S, N)), ref=self.rng.integers(-1, L, (S, N)),
                            t=self.rng.random(S), n_events=self.rng.integers(100, 1000, S), next_obs=ctx["obs_first"] + ctx["M"] - _short(ctx))
                for k, (dtype, text) in CHECKPOINT_POINTERS.items():
                    _write(getattr(target, k), fill[k], dtype, _shape(text, ctx))
                if name == "xck_out":
                    kk = max(ctx.get("k_max", 0), 0)
                    fill = dict(n_slots=n_slots, window=self.rng.random((S, kk, 3)) + 0.5 if more.window else None, n_empty=np.zeros(S),
                                n_window=np.full(S, max(ctx["obs_first"] + ctx["M"] - ctx.get("first_obs", 0), 0)))
                    for k, (dtype, text) in MIXED_CHECKPOINT_POINTERS.items():
                        if getattr(more, k):
                            _write(getattr(more, k), fill[k], dtype, _shape(text, dict(ctx, k_max=kk)))
            elif target:
                dtype, text, make = OUT[name]
                shape = _shape(text, ctx)
                _write(target, make(self.rng, ctx, shape), dtype, shape)
        return 0


# ---- the systems and raw keywords of the cases

T, DT = 0.2, 0.02


def systems(n=3, L=64, N=20, seed=5, **kw):
    kw = dict(dict(site_capacity=1), **kw)
    return [ParticleSystem(L, 1.0, 0.01, 0.1, 0.5 + 0.25 * i, N=N, seed=seed, rng=np.random.default_rng(100 + i), **kw) for i in range(n)]


def large(n=2, N=40, seed=5, **kw):
    return [ParticleSystem(4100, 1.0, 41.0, 6.4, 0.5 + 0.25 * i, N=N, seed=seed, scale_rates=False, rng=np.random.default_rng(200 + i), **kw)
            for i in range(n)]


def poisson(n=3, seed=5, **kw):
    """Particle numbers that differ from system to system."""
    return [ParticleSystem(64, 1.0, 0.01, 0.1, 0.5, init="poisson", rho0_plus=lambda x, i=i: 0.1 + 0.1 * i, rho0_minus=lambda x: 0.1, seed=seed,
                           rng=np.random.default_rng(300 + i), **kw) for i in range(n)]


def two_densities(**kw):
    """Particle numbers on either side of L: the blocking thresholds of the statistics differ."""
    return systems(2, site_capacity=2, **kw) + systems(1, N=100, site_capacity=2, **kw)


def flip(sigma, m):
    return 1.0 + 0.5 * sigma * m


ANCHORS = dict(anchor_positions=[0.3, 0.7], anchor_radius=0.02, k_exit=0.5)
SIGMAS = dict(local_kernel_sigma=0.02)


def with_sigmas(make=systems, **kw):
    def build():
        out = make(**kw)
        for i, ps in enumerate(out):
            ps.local_kernel_sigma = 0.005 * (1 + i % 2)
            ps._sigma_grid = ps.local_kernel_sigma / ps.dx
        return out
    return build


def altered(attr, value, make=systems, **kw):
    def build():
        out = make(**kw)
        setattr(out[-1], attr, value)
        return out
    return build


def other_anchors():
    out = systems(**ANCHORS)
    out[-1].is_anchor_site = np.roll(out[-1].is_anchor_site, 1)
    return out


def other_flip():
    return systems(2, flip_rate_fn=flip, mode="gillespie_gpu") + systems(1, flip_rate_fn=lambda s, m: 2.0 + 0.0 * m, mode="gillespie_gpu")


def uniforms(S, E=7):
    return np.random.default_rng(9).random((S, E, 4))


def checkpoint(next_obs=(2, 2, 2), S=3, N=20, L=64, streams="batch", **kw):
    g = np.random.default_rng(17)
    fields = dict(L=L, K=1, periodic=False, local_kernel_sigma=0.005, anchor_mask=None, seed=5, streams=streams, obs_dt=DT)
    fields.update(kw)
    return gil.Checkpoint(pos=g.integers(0, L, (S, N)), flags=np.full((S, N), gil.GILR_ALIVE | gil.GILR_PLUS), ref=np.full((S, N), -1), t=g.random(S) * 0.01,
                          n_events=g.integers(0, 50, S), next_obs=np.asarray(next_obs)[:S], **fields)


STATES = [(np.array([3, 9, 11]), np.array([1, -1, 1])), (np.array([0, 5, 5, 60, 61]), np.array([-1, -1, 1, 1, 1]), np.array([0, 1, 0, 0, 1]))]


def raw(**kw):
    base = dict(L=64, K=2, periodic=True, sigma_grid=1.5, rate_diffusion=0.3, rate_active=1.2, betas=[0.5, 0.9], states=STATES,
                times_obs=np.arange(5) * 0.1, T=0.5, seed=2 ** 64 + 7)
    base.update(kw)
    return {k: v for k, v in base.items() if v is not Ellipsis}


FULL = dict(minus_anchor=False, immobilize=False, suppress_flip=False, crowding=True, k_on=0.25, k_off=0.125, k_exit=0.0625,
            anchor_mask=np.arange(64) % 7 == 0, max_events=50, want_states=False, x_wall=60, ref_obs=3, front_lo=np.arange(64) // 2,
            block_table=np.arange(9).reshape(3, 3) % 2, device=0, flip_table=np.linspace(0.5, 1.5, 10).reshape(2, 5), n_cap=8)
MIXED = dict(sigma_grid=Ellipsis, sigma_grids=[1.5, 3.0], variant_of_system=[1, 0])
CK_RAW = dict(pos=np.arange(12).reshape(2, 6), flags=np.full((2, 6), 5), ref=np.full((2, 6), -1), t=[0.25, 0.3], n_events=[40, 50], next_obs=[3, 2])
PLAN = dict(L=256, K=2, periodic=False, n_systems=4, n_cap=100, n_obs=8)
PLAN_LARGE = dict(PLAN, L=4100)

CASES = []


def case(name, make, call, **standin):
    CASES.append((name, make, call, standin))


def none():
    return []


E, ES = gil.run_batched_exact, gil.run_batched_exact_statistics
EM, ESM, ETM = gil.run_batched_exact_mixed, gil.run_batched_exact_statistics_mixed, gil.run_batched_exact_structure_mixed
ET, EC, EP = gil.run_batched_exact_structure, gil.run_batched_exact_capture, gil.run_batched_exact_profiles
RUN = dict(T=T, obs_dt=DT)


def two_segments(fn, **kw):
    """A run cut at observation 4: the first segment with its checkpoint, the rest resumed from it."""
    def call(s):
        head, ck = fn(s, obs_range=(0, 4), return_checkpoint=True, **RUN, **kw)
        return head, ck, fn(s, resume=ck, **RUN, **kw)
    return call


# run_batched_exact
case("exact", systems, lambda s: E(s, want_m_local=False, **RUN))
case("exact-seed-drawn", lambda: systems(seed=None), lambda s: E(s, want_m_local=False, **RUN))
case("exact-one-system-fft-var", lambda: systems(1), lambda s: E(s, record_fft=True, record_var=True, want_m_local=False, **RUN))
case("exact-fft-only", lambda: systems(2), lambda s: E(s, record_fft=True, want_m_local=False, **RUN))
case("exact-K2-uniforms", lambda: systems(site_capacity=2), lambda s: E(s, uniforms=uniforms(3), want_m_local=False, **RUN))
case("exact-anchors-exits", lambda: systems(**ANCHORS), lambda s: E(s, want_m_local=False, **RUN))
case("exact-flip-table", lambda: systems(flip_rate_fn=flip, mode="gillespie_gpu"), lambda s: E(s, want_m_local=False, **RUN))
case("exact-poisson", poisson, lambda s: E(s, want_m_local=False, **RUN))
case("exact-large", large, lambda s: E(s, want_m_local=False, **RUN))
case("exact-large-by-N", lambda: systems(2, L=4096, N=2049), lambda s: E(s, want_m_local=False, T=0.04, obs_dt=0.02))
case("exact-short", systems, lambda s: E(s, want_m_local=False, **RUN), short=2)
case("exact-two-segments", systems, two_segments(E, want_m_local=False))
case("exact-two-segments-seed-drawn", lambda: systems(seed=None), two_segments(E, want_m_local=False))
case("exact-two-segments-large", large, two_segments(E, want_m_local=False))
case("exact-chain", systems, lambda s: E(s, obs_per_launch=3, want_m_local=False, **RUN))
case("exact-chain-uniforms-checkpoint", lambda: systems(**ANCHORS),
     lambda s: E(s, obs_per_launch=4, uniforms=uniforms(3), return_checkpoint=True, want_m_local=False, **RUN))
case("exact-obs_range", systems, lambda s: E(s, obs_range=(0, 6), want_m_local=False, **RUN))
case("exact-resume-given", systems, lambda s: E(s, resume=checkpoint((2, 3, 5)), want_m_local=False, **RUN))
case("exact-resume-range-chain", systems, lambda s: E(s, resume=checkpoint(), obs_range=(3, 9), obs_per_launch=4, return_checkpoint=True,
                                                      want_m_local=False, **RUN))
case("exact-resume-short", systems, lambda s: E(s, resume=checkpoint(), want_m_local=False, **RUN), short=1)
case("exact-differ", altered("k_on", 0.3), lambda s: E(s, **RUN))
case("exact-differ-periodic", altered("periodic", True), lambda s: E(s, resume=checkpoint(), **RUN))
case("exact-resume-not-a-checkpoint", systems, lambda s: E(s, resume={"pos": 0}, **RUN))
case("exact-resume-other-L", systems, lambda s: E(s, resume=checkpoint(L=65), **RUN))
case("exact-resume-other-seed", systems, lambda s: E(s, resume=checkpoint(seed=6), **RUN))
case("exact-resume-other-seed-seed-drawn", lambda: systems(seed=None), lambda s: E(s, resume=checkpoint(seed=6), want_m_local=False, **RUN))
case("exact-resume-other-streams", systems, lambda s: E(s, resume=checkpoint(streams="large"), **RUN))
case("exact-resume-other-anchors", lambda: systems(**ANCHORS), lambda s: E(s, resume=checkpoint(), **RUN))
case("exact-resume-other-systems", lambda: systems(2), lambda s: E(s, resume=checkpoint(), **RUN))
case("exact-resume-other-obs_dt", systems, lambda s: E(s, resume=checkpoint(), T=T, obs_dt=0.01))
case("exact-obs_range-empty", systems, lambda s: E(s, obs_range=(4, 4), **RUN))
case("exact-obs_range-beyond", systems, lambda s: E(s, obs_range=(0, 99), **RUN))
case("exact-obs_range-late-start", systems, lambda s: E(s, obs_range=(2, 5), **RUN))
case("exact-obs_per_launch-0", systems, lambda s: E(s, obs_per_launch=0, **RUN))
def lds_limit(fn, limit=1024, **kw):
    """`fn` with the LDS a mixed launch may have lowered to `limit` bytes."""
    def call(s):
        saved, gil.GILX_LDS_LIMIT = gil.GILX_LDS_LIMIT, limit
        try:
            return fn(s, **RUN, **kw)
        finally:
            gil.GILX_LDS_LIMIT = saved
    return call


case("exact-refused", systems, lambda s: E(s, want_m_local=False, **RUN), rc=-1)
case("exact-large-refused", large, lambda s: E(s, want_m_local=False, **RUN), rc=-2)
case("exact-chain-refused", systems, lambda s: E(s, obs_per_launch=3, want_m_local=False, **RUN), rc=-1)
case("exact-chain-older-build", systems, lambda s: E(s, obs_per_launch=3, want_m_local=False, **RUN), missing=("gilr_run", "gilrm_run"))
# run_batched_exact_statistics
case("statistics", systems, lambda s: ES(s, **RUN))
case("statistics-seed-drawn", lambda: systems(seed=None), lambda s: ES(s, **RUN))
case("statistics-K2-flip-table", lambda: systems(site_capacity=2, flip_rate_fn=flip, mode="gillespie_gpu"), lambda s: ES(s, **RUN))
case("statistics-anchors", lambda: systems(anchor_positions=[0.5]), lambda s: ES(s, **RUN))
case("statistics-large", large, lambda s: ES(s, **RUN))
case("statistics-two-segments", systems, two_segments(ES))
case("statistics-two-segments-large", large, two_segments(ES))
case("statistics-chain", lambda: systems(seed=None), lambda s: ES(s, obs_per_launch=3, **RUN))
case("statistics-chain-checkpoint", systems, lambda s: ES(s, obs_per_launch=7, return_checkpoint=True, **RUN))
case("statistics-resume-range", systems, lambda s: ES(s, resume=checkpoint(), obs_range=(2, 8), **RUN))
case("statistics-short", systems, lambda s: ES(s, **RUN), short=1)
case("statistics-chain-short", systems, lambda s: ES(s, obs_per_launch=5, **RUN), short=1)
case("statistics-differ", altered("rate_active", 7.0), lambda s: ES(s, **RUN))
case("statistics-k_exit", lambda: systems(k_exit=0.5), lambda s: ES(s, **RUN))
case("statistics-differ-before-k_exit", altered("K", 2, k_exit=0.5), lambda s: ES(s, **RUN))
case("statistics-k_exit-negative-zero", lambda: systems(k_exit=-0.0), lambda s: ES(s, **RUN))
case("statistics-chain-k_exit-negative-zero", lambda: systems(k_exit=-0.0), lambda s: ES(s, obs_per_launch=5, **RUN))
case("statistics-thresholds", two_densities, lambda s: ES(s, **RUN))
case("statistics-thresholds-chain", two_densities, lambda s: ES(s, obs_per_launch=5, **RUN))
case("statistics-resume-different-observations", systems, lambda s: ES(s, resume=checkpoint((2, 3, 3)), **RUN))
case("statistics-refused", systems, lambda s: ES(s, **RUN), rc=-3)
# the mixed launches
case("mixed", with_sigmas(), lambda s: EM(s, want_m_local=False, **RUN))
case("mixed-groups-order-seed-drawn", with_sigmas(n=4, seed=None), lambda s: EM(s, groups=[0, 1, 0, 1], order=[3, 2, 1, 0], record_fft=True,
                                                                             record_var=True, uniforms=uniforms(4), want_m_local=False, **RUN))
case("mixed-anchors-flip-table", with_sigmas(flip_rate_fn=flip, mode="gillespie_gpu", **ANCHORS), lambda s: EM(s, want_m_local=False, **RUN))
case("mixed-differ", altered("k_off", 0.3), lambda s: EM(s, **RUN))
case("mixed-differ-anchors", other_anchors, lambda s: EM(s, **RUN))
case("mixed-differ-flip", other_flip, lambda s: EM(s, **RUN))
case("mixed-differ-flip-none", lambda: systems(2, flip_rate_fn=flip, mode="gillespie_gpu") + systems(1), lambda s: EM(s, **RUN))
case("mixed-large", large, lambda s: EM(s, **RUN))
case("mixed-groups-length", systems, lambda s: EM(s, groups=[0, 1], **RUN))
case("mixed-order-length", systems, lambda s: EM(s, order=[0, 1], want_m_local=False, **RUN))
case("mixed-resume", systems, lambda s: EM(s, resume=checkpoint(), **RUN))
case("mixed-lds-limit", with_sigmas(), lds_limit(EM, want_m_local=False))
case("statistics_mixed-lds-limit", with_sigmas(), lds_limit(ESM))
case("structure_mixed-lds-limit", with_sigmas(), lds_limit(ETM))
case("structure_mixed-rows-lds-limit-large-before", large, lds_limit(ETM, reduce="rows"))
case("structure_mixed-k_max-0", systems, lambda s: ETM(s, k_max=0, **RUN), ask_library=True)
case("mixed-refused", systems, lambda s: EM(s, want_m_local=False, **RUN), rc=-1)
case("statistics_mixed", with_sigmas(two_densities), lambda s: ESM(s, **RUN))
case("statistics_mixed-groups-seed-drawn", with_sigmas(poisson, seed=None), lambda s: ESM(s, groups=[1, 1, 0], order=[2, 0, 1], **RUN))
case("statistics_mixed-k_exit-negative-zero", lambda: systems(k_exit=-0.0), lambda s: ESM(s, **RUN))
case("statistics_mixed-k_exit", lambda: systems(k_exit=0.5), lambda s: ESM(s, **RUN))
case("statistics_mixed-short", systems, lambda s: ESM(s, **RUN), short=1)
case("statistics_mixed-resume", systems, lambda s: ESM(s, resume=checkpoint(), **RUN))
for reduce in ("device", "rows"):
    case(f"structure_mixed-{reduce}", with_sigmas(), lambda s, r=reduce: ETM(s, reduce=r, **RUN))
    case(f"structure_mixed-{reduce}-series", with_sigmas(seed=None), lambda s, r=reduce: ETM(s, reduce=r, return_series=True, k_max=7, start_fraction=0.3,
                                                                                                groups=[0, 0, 1], **RUN))
    case(f"structure_mixed-{reduce}-short", systems, lambda s, r=reduce: ETM(s, reduce=r, **RUN), short=1)
case("structure_mixed-k_max-beyond-L", systems, lambda s: ETM(s, k_max=100, order=[2, 1, 0], **RUN))
case("structure_mixed-reduce", systems, lambda s: ETM(s, reduce="host", **RUN))
case("structure_mixed-resume-before-reduce", systems, lambda s: ETM(s, reduce="host", resume=checkpoint(), **RUN))
case("structure_mixed-differ", altered("xlim", 2.0), lambda s: ETM(s, **RUN))
case("structure_mixed-large", large, lambda s: ETM(s, **RUN))
case("structure_mixed-refused", systems, lambda s: ETM(s, **RUN), rc=-1)
# structure, capture, profiles
case("structure", systems, lambda s: ET(s, **RUN))
case("structure-series-seed-drawn", lambda: systems(seed=None, **ANCHORS), lambda s: ET(s, return_series=True, k_max=5, start_fraction=0.25, **RUN))
case("structure-k_max-beyond-L", lambda: systems(flip_rate_fn=flip, mode="gillespie_gpu"), lambda s: ET(s, k_max=1000, **RUN))
case("structure-large", large, lambda s: ET(s, k_max=16, **RUN))
case("structure-short", systems, lambda s: ET(s, **RUN), short=3)
case("structure-differ", altered("local_kernel_sigma", 0.01), lambda s: ET(s, **RUN))
case("structure-resume", systems, lambda s: ET(s, resume=checkpoint(), **RUN))
case("structure-k_max-0", systems, lambda s: ET(s, k_max=0, **RUN), ask_library=True)
case("structure-refused", systems, lambda s: ET(s, **RUN), rc=-1)
case("capture", lambda: systems(**ANCHORS), lambda s: EC(s, **RUN))
case("capture-no-anchors-seed-drawn", lambda: systems(seed=None), lambda s: EC(s, c_bins=8, h_bins=10, h_dt=0.05, start_fraction=0.5,
                                                                             uniforms=uniforms(3), **RUN))
case("capture-flip-table", lambda: systems(flip_rate_fn=flip, mode="gillespie_gpu", **ANCHORS), lambda s: EC(s, **RUN))
case("capture-large", lambda: large(**ANCHORS), lambda s: EC(s, **RUN))
case("capture-short", lambda: systems(**ANCHORS), lambda s: EC(s, **RUN), short=1)
case("capture-differ", altered("minus_anchor", False), lambda s: EC(s, **RUN))
case("capture-differ-anchors", other_anchors, lambda s: EC(s, **RUN))
case("capture-resume", systems, lambda s: EC(s, resume=checkpoint(), **RUN))
case("capture-h_bins-0", lambda: systems(**ANCHORS), lambda s: EC(s, h_bins=0, h_dt=0.01, **RUN), ask_library=True)
case("capture-c_bins-1", systems, lambda s: EC(s, c_bins=1, **RUN), ask_library=True)
case("capture-refused", systems, lambda s: EC(s, **RUN), rc=-1)
case("profiles", systems, lambda s: EP(s, **RUN))
case("profiles-groups-per_system-field", lambda: systems(4, seed=None), lambda s: EP(s, n_bins=16, groups=[0, 1, 1, 0], first_obs=2, want_field=True,
                                                                                   per_system=True, uniforms=uniforms(4), **RUN))
case("profiles-flip-table-anchors", lambda: systems(flip_rate_fn=flip, mode="gillespie_gpu", anchor_positions=[0.5]), lambda s: EP(s, n_bins=10, **RUN))
case("profiles-large", large, lambda s: EP(s, per_system=True, **RUN))
case("profiles-differ", altered("suppress_flip_when_bound", False), lambda s: EP(s, **RUN))
case("profiles-k_exit", lambda: systems(k_exit=0.5), lambda s: EP(s, **RUN))
case("profiles-particle-numbers", poisson, lambda s: EP(s, **RUN))
case("profiles-resume", systems, lambda s: EP(s, resume=checkpoint(), **RUN))
case("profiles-n_bins-0", systems, lambda s: EP(s, n_bins=0, **RUN), ask_library=True)
case("profiles-n_bins-0-per_system", lambda: systems(seed=None), lambda s: EP(s, n_bins=0, per_system=True, groups=[0, 1, 0], **RUN), ask_library=True)
case("profiles-refused", systems, lambda s: EP(s, **RUN), rc=-1)
# mixed_keys, mixed_variants, Checkpoint
case("mixed_keys-one-group", lambda: systems(seed=None), lambda s: gil.mixed_keys(s))
case("mixed_keys-groups", lambda: systems(5, seed=None), lambda s: gil.mixed_keys(s, [2, 0, 2, 1, 0]))
case("mixed_keys-seeds-given", lambda: systems(2, seed=11) + systems(2, seed=None), lambda s: gil.mixed_keys(s, [0, 0, 1, 1]))
case("mixed_keys-length", systems, lambda s: gil.mixed_keys(s, [0]))
case("mixed_variants", none, lambda s: gil.mixed_variants([1.0, 2.0, 1.0, 1.0], np.array([[[0, 1], [1, 1]]] * 3 + [[[0, 0], [1, 1]]])))
case("checkpoint-shapes", none, lambda s: checkpoint(next_obs=(1, 2)))
case("checkpoint-streams", none, lambda s: checkpoint(streams="other"))
# the raw functions
RAW = (("run_raw", gil.run_raw, {}), ("run_many_large_raw", gil.run_many_large_raw, {}), ("run_resumable_raw", gil.run_resumable_raw, {}),
       ("run_resumable_raw-large", gil.run_resumable_raw, dict(large=True)),
       ("run_structure_raw", gil.run_structure_raw, {}), ("run_capture_raw", gil.run_capture_raw, {}), ("run_profiles_raw", gil.run_profiles_raw, {}),
       ("run_mixed_raw", gil.run_mixed_raw, MIXED), ("run_mixed_structure_raw", gil.run_mixed_structure_raw, MIXED))
for tag, fn, extra in RAW:
    full = dict(FULL, **extra)
    if "sigma_grids" in extra:
        full["block_tables"] = np.arange(18).reshape(2, 3, 3) % 2
        del full["block_table"]
    case(f"{tag}-defaults", none, lambda s, fn=fn, kw=extra: fn(**raw(**kw)))
    case(f"{tag}-every-keyword", none, lambda s, fn=fn, kw=full: fn(**raw(**kw)))
    case(f"{tag}-uniforms", none, lambda s, fn=fn, kw=extra: fn(**raw(uniforms=uniforms(2, 5), max_events=3, **kw)))
    case(f"{tag}-uniforms-shape", none, lambda s, fn=fn, kw=extra: fn(**raw(uniforms=uniforms(3, 5), **kw)))
    case(f"{tag}-n_cap-small", none, lambda s, fn=fn, kw=extra: fn(**raw(n_cap=4, **kw)))
    case(f"{tag}-empty-anchor-mask", none, lambda s, fn=fn, kw=extra: fn(**raw(anchor_mask=np.zeros(64, bool), betas=0.75, **kw)))
    case(f"{tag}-refused", none, lambda s, fn=fn, kw=extra: fn(**raw(**kw)), rc=-4)
case("run_resumable_raw-checkpoint", none, lambda s: gil.run_resumable_raw(**raw(checkpoint=CK_RAW, obs_first=2, states=None)))
case("run_resumable_raw-checkpoint-large-n_cap", none, lambda s: gil.run_resumable_raw(**raw(checkpoint=CK_RAW, obs_first=3, states=None, n_cap=6, large=True)))
case("run_resumable_raw-checkpoint-other-n_cap", none, lambda s: gil.run_resumable_raw(**raw(checkpoint=CK_RAW, states=None, n_cap=7)))
case("run_resumable_raw-checkpoint-shapes", none, lambda s: gil.run_resumable_raw(**raw(checkpoint=dict(CK_RAW, t=[0.25]), states=None)))
case("run_resumable_raw-older-build", none, lambda s: gil.run_resumable_raw(**raw()), missing=("gilr_run",))
case("run_resumable_raw-large-older-build", none, lambda s: gil.run_resumable_raw(**raw(large=True)), missing=("gilrm_run",))
case("run_structure_raw-k_max-first_obs", none, lambda s: gil.run_structure_raw(**raw(k_max=3, first_obs=2, want_states=False)))
case("run_structure_raw-k_max-0", none, lambda s: gil.run_structure_raw(**raw(k_max=0)), ask_library=True)
case("run_structure_raw-k_max-negative", none, lambda s: gil.run_structure_raw(**raw(k_max=-3, want_states=False)), ask_library=True)
case("run_structure_raw-large-L-k_max", none, lambda s: gil.run_structure_raw(**raw(L=5000, want_states=False)))
case("run_capture_raw-groups", none, lambda s: gil.run_capture_raw(**raw(group_of_site=np.arange(64) % 3 - 1, c_bins=4, h_bins=6, first_obs=1,
                                                                         anchor_mask=np.ones(64))))
case("run_capture_raw-groups-given", none, lambda s: gil.run_capture_raw(**raw(group_of_site=np.arange(64) % 3 - 1, n_groups=5, h_dt=0.01)))
case("run_capture_raw-h_bins-0", none, lambda s: gil.run_capture_raw(**raw(h_bins=0, h_dt=0.01)), ask_library=True)
case("run_capture_raw-c_bins-n_groups-negative", none, lambda s: gil.run_capture_raw(**raw(c_bins=-2, n_groups=-1)), ask_library=True)
case("run_capture_raw-groups-shape", none, lambda s: gil.run_capture_raw(**raw(group_of_site=np.zeros(63))))
case("run_profiles_raw-groups", none, lambda s: gil.run_profiles_raw(**raw(n_bins=7, first_obs=1, want_field=True, group_of_system=[1, 0], per_system=True)))
case("run_profiles_raw-groups-given", none, lambda s: gil.run_profiles_raw(**raw(group_of_system=[0, 0], n_groups=3)))
case("run_profiles_raw-n_bins-0", none, lambda s: gil.run_profiles_raw(**raw(n_bins=0)), ask_library=True)
case("run_profiles_raw-n_bins-negative-per_system", none, lambda s: gil.run_profiles_raw(**raw(n_bins=-5, per_system=True, n_groups=0)), ask_library=True)
case("run_profiles_raw-groups-shape", none, lambda s: gil.run_profiles_raw(**raw(group_of_system=[0])))
case("run_profiles_raw-large-L-n_bins", none, lambda s: gil.run_profiles_raw(**raw(L=5000, want_states=False)))
for tag, fn in (("run_mixed_raw", gil.run_mixed_raw), ("run_mixed_structure_raw", gil.run_mixed_structure_raw)):
    case(f"{tag}-keys-order", none, lambda s, fn=fn: fn(**raw(**dict(MIXED, seeds=[2 ** 64 + 3, -1], streams=[4, 0], order=[1, 0]))))
    case(f"{tag}-no-variant_of_system", none, lambda s, fn=fn: fn(**raw(**dict(MIXED, variant_of_system=None))))
    for name in ("variant_of_system", "seeds", "streams", "order"):
        case(f"{tag}-{name}-length", none, lambda s, fn=fn, name=name: fn(**raw(**dict(MIXED, **{name: [0]}))))
    case(f"{tag}-block_tables-shape", none, lambda s, fn=fn: fn(**raw(**dict(MIXED, block_tables=np.zeros((2, 2, 2))))))
case("run_mixed_structure_raw-k_max-0", none, lambda s: gil.run_mixed_structure_raw(**raw(k_max=0, **MIXED)), ask_library=True)
case("run_mixed_structure_raw-k_max-negative-no-rows", none, lambda s: gil.run_mixed_structure_raw(**raw(k_max=-1, want_rows=False, **MIXED)), ask_library=True)
case("run_mixed_structure_raw-no-rows", none, lambda s: gil.run_mixed_structure_raw(**raw(want_rows=False, want_states=False, k_max=4, first_obs=1, **MIXED)))
LARGE_RAW = dict(L=4100, K=1, periodic=False, sigma_grid=2.0, rate_diffusion=0.3, rate_active=1.2, beta=0.75, state=STATES[0],
                 times_obs=np.arange(4) * 0.1, T=0.4)
case("run_large_raw-defaults", none, lambda s: gil.run_large_raw(**LARGE_RAW))
case("run_large_raw-every-keyword", none, lambda s: gil.run_large_raw(**dict(
    LARGE_RAW, state=STATES[1], K=2, seed=-3, anchor_mask=np.arange(4100) % 7 == 0, **{k: v for k, v in FULL.items() if k not in ("x_wall", "ref_obs", "front_lo", "block_table", "n_cap", "anchor_mask")})))
case("run_large_raw-uniforms", none, lambda s: gil.run_large_raw(**dict(LARGE_RAW, uniforms=uniforms(1, 6)[0], max_events=2)))
case("run_large_raw-empty-state", none, lambda s: gil.run_large_raw(**dict(LARGE_RAW, state=((), ()), anchor_mask=np.zeros(4100))))
case("run_large_raw-refused", none, lambda s: gil.run_large_raw(**LARGE_RAW), rc=-2)
# the plans (the real library)
PLANS = (("plan_many_large", gil.plan_many_large, dict(PLAN_LARGE, sigma_grid=3.0), dict(want_states=False, want_scalars=False)),
         ("plan_structure", gil.plan_structure, dict(PLAN, sigma_grid=3.0, k_max=16), dict(first_obs=2, want_states=False)),
         ("plan_capture", gil.plan_capture, dict(PLAN, sigma_grid=3.0), dict(n_groups=3, c_bins=8, h_bins=20, first_obs=1, want_states=False)),
         ("plan_profiles", gil.plan_profiles, dict(PLAN, sigma_grid=3.0, n_bins=32), dict(n_groups=2, first_obs=1, want_field=True, want_states=False,
                                                                                        per_system=True)),
         ("plan_mixed", gil.plan_mixed, dict(PLAN, sigma_grids=[1.0, 3.0]), dict(variant_of_system=[0, 1, 1, 0], order=[3, 2, 1, 0], want_states=False)),
         ("plan_mixed_structure", gil.plan_mixed_structure, dict(PLAN, sigma_grids=[1.0, 3.0], k_max=16),
          dict(first_obs=2, variant_of_system=[0, 1, 1, 0], order=[3, 2, 1, 0], want_states=False, want_rows=False)),
         ("plan_mixed_many", gil.plan_mixed_many, dict(PLAN, sigma_grids=[1.0, 3.0]), dict(variant_of_system=[0, 1, 1, 0], order=[3, 2, 1, 0],
                                                                                           want_states=False)))
for tag, fn, kw, more in PLANS:
    case(f"{tag}-defaults", none, lambda s, fn=fn, kw=kw: fn(**kw))
    case(f"{tag}-every-keyword", none, lambda s, fn=fn, kw=dict(kw, **more): fn(**kw))
    case(f"{tag}-periodic-large-L", none, lambda s, fn=fn, kw=dict(kw, L=4100, periodic=True): fn(**kw))
    case(f"{tag}-refused", none, lambda s, fn=fn, kw=dict(kw, K=0): fn(**kw))
case("plan_mixed-order-length", none, lambda s: gil.plan_mixed(**dict(PLAN, sigma_grids=[1.0], order=[0])))


# ---- NEWER: the large mixed launch, MixedCheckpoint, the mixed segment chains, their raw functions and plan_mixed_many

def mixed_checkpoint(next_obs=(2, 2, 2), make=with_sigmas(), N=20, structure=False, tables=False, **kw):
    """A MixedCheckpoint that the systems of `make` (seed = 5, one group) can resume from; `kw` replaces constructor keywords."""
    like = make()
    S, first, g = len(like), like[0], np.random.default_rng(23)
    large = gil._large_shape(first.L, N)
    fields = dict(L=first.L, K=first.K, periodic=first.periodic, anchor_mask=first.is_anchor_site, obs_dt=DT, large=large,
                  sigma_grids=[ps._sigma_grid for ps in like], seeds=[5 + s if large else 5 for s in range(S)],
                  streams=[0 if large else s for s in range(S)], n_slots=[N] * S,
                  pos=g.integers(0, first.L, (S, N)), flags=np.full((S, N), gil.GILR_ALIVE | gil.GILR_PLUS), ref=np.full((S, N), -1),
                  t=g.random(S) * 0.01, n_events=g.integers(0, 50, S), next_obs=np.asarray(next_obs)[:S])
    if tables:
        fields["block_tables"] = g.integers(0, 2, (S, first.K + 1, first.K + 1))
    if structure:
        kk = first.L
        fields.update(k_max=kk, first_obs=5, window=g.random((S, kk, 3)) + 0.5, n_window=[0] * S, n_empty=[0] * S)
    fields.update(kw)
    return gil.MixedCheckpoint(**fields)


GOO = dict(groups=[0, 1, 0], order=[2, 1, 0])
# one launch, large
case("mixed-allow_large", large, lambda s: EM(s, allow_large=True, want_m_local=False, **RUN))
case("statistics_mixed-allow_large", large, lambda s: ESM(s, allow_large=True, **RUN))
case("mixed-allow_large-small-shape", with_sigmas(), lambda s: EM(s, allow_large=True, want_m_local=False, **RUN))
case("statistics_mixed-allow_large-small-shape", with_sigmas(), lambda s: ESM(s, allow_large=True, **RUN))
case("structure_mixed-large-resume", large, lambda s: ETM(s, resume=mixed_checkpoint(make=large, N=40, structure=True), **RUN))
# segments
case("mixed-two-segments", with_sigmas(), two_segments(EM, want_m_local=False))
case("mixed-two-segments-seed-drawn", with_sigmas(seed=None), two_segments(EM, want_m_local=False))
case("mixed-two-segments-groups-order-uniforms", with_sigmas(), two_segments(EM, want_m_local=False, uniforms=uniforms(3), **GOO))
case("mixed-two-segments-allow_large", large, two_segments(EM, want_m_local=False, allow_large=True))
case("statistics_mixed-two-segments", with_sigmas(two_densities), two_segments(ESM))
case("statistics_mixed-two-segments-allow_large", large, two_segments(ESM, allow_large=True))
for reduce in ("device", "rows"):
    case(f"structure_mixed-cut-in-two-{reduce}", with_sigmas(), two_segments(ETM, reduce=reduce))
# chains
case("mixed-chain", with_sigmas(), lambda s: EM(s, obs_per_launch=3, want_m_local=False, **RUN))
case("statistics_mixed-chain-checkpoint", with_sigmas(two_densities), lambda s: ESM(s, obs_per_launch=7, return_checkpoint=True, **RUN))
case("structure_mixed-chain-rows-series", with_sigmas(), lambda s: ETM(s, obs_per_launch=4, reduce="rows", return_series=True, k_max=7, start_fraction=0.3,
                                                                      **RUN))
case("structure_mixed-chain-device-series-checkpoint", with_sigmas(seed=None), lambda s: ETM(s, obs_per_launch=3, return_series=True, return_checkpoint=True,
                                                                                             groups=[0, 0, 1], **RUN))
case("mixed-chain-short", with_sigmas(), lambda s: EM(s, obs_per_launch=3, want_m_local=False, **RUN), short=1)
case("statistics_mixed-chain-short", with_sigmas(), lambda s: ESM(s, obs_per_launch=5, **RUN), short=1)
case("structure_mixed-chain-short", with_sigmas(), lambda s: ETM(s, obs_per_launch=4, **RUN), short=1)
# ranges
case("mixed-obs_range", with_sigmas(), lambda s: EM(s, obs_range=(0, 6), want_m_local=False, **RUN))
case("structure_mixed-obs_range-checkpoint", with_sigmas(), lambda s: ETM(s, obs_range=(0, 6), return_checkpoint=True, **RUN))
case("structure_mixed-obs_range", with_sigmas(), lambda s: ETM(s, obs_range=(0, 6), **RUN))
case("mixed-resume-given", with_sigmas(), lambda s: EM(s, resume=mixed_checkpoint((2, 3, 5)), want_m_local=False, **RUN))
case("mixed-resume-range-chain", with_sigmas(), lambda s: EM(s, resume=mixed_checkpoint(), obs_range=(3, 9), obs_per_launch=4, return_checkpoint=True,
                                                             want_m_local=False, **RUN))
case("statistics_mixed-resume-tables", with_sigmas(), lambda s: ESM(s, resume=mixed_checkpoint(tables=True), return_checkpoint=True, **RUN))
case("statistics_mixed-resume-range", with_sigmas(), lambda s: ESM(s, resume=mixed_checkpoint(), obs_range=(2, 8), **RUN))
case("structure_mixed-resume-given", with_sigmas(), lambda s: ETM(s, resume=mixed_checkpoint(structure=True), return_series=True, **RUN))
case("structure_mixed-resume-inside-window", with_sigmas(), lambda s: ETM(s, resume=mixed_checkpoint((7, 7, 7), structure=True), **RUN))
case("statistics_mixed-resume-different-observations", with_sigmas(), lambda s: ESM(s, resume=mixed_checkpoint((2, 3, 3)), **RUN))
# refusals before any launch
case("mixed-resume-structure-checkpoint", with_sigmas(), lambda s: EM(s, resume=mixed_checkpoint(structure=True), **RUN))
case("statistics_mixed-resume-structure-checkpoint", with_sigmas(), lambda s: ESM(s, resume=mixed_checkpoint(structure=True), **RUN))
case("structure_mixed-resume-plain-mixed-checkpoint", with_sigmas(), lambda s: ETM(s, resume=mixed_checkpoint(), **RUN))
case("structure_mixed-resume-plain-checkpoint", with_sigmas(), lambda s: ETM(s, resume=checkpoint(), **RUN))
case("mixed-resume-arrays", with_sigmas(), lambda s: EM(s, resume=mixed_checkpoint().arrays(), **RUN))
case("exact-resume-mixed-checkpoint", systems, lambda s: E(s, resume=mixed_checkpoint(make=systems), **RUN))
case("statistics-resume-mixed-checkpoint", systems, lambda s: ES(s, resume=mixed_checkpoint(make=systems), **RUN))
case("mixed-resume-other-L", with_sigmas(), lambda s: EM(s, resume=mixed_checkpoint(L=65), **RUN))
case("mixed-resume-other-K", with_sigmas(), lambda s: EM(s, resume=mixed_checkpoint(K=2), **RUN))
case("mixed-resume-other-periodic", with_sigmas(), lambda s: EM(s, resume=mixed_checkpoint(periodic=True), **RUN))
case("mixed-resume-other-anchors", with_sigmas(**ANCHORS), lambda s: EM(s, resume=mixed_checkpoint(), **RUN))
case("mixed-resume-other-systems", with_sigmas(n=2), lambda s: EM(s, resume=mixed_checkpoint(), **RUN))
case("mixed-resume-other-obs_dt", with_sigmas(), lambda s: EM(s, resume=mixed_checkpoint(), T=T, obs_dt=0.01))
case("mixed-resume-other-sigma_grids", systems, lambda s: EM(s, resume=mixed_checkpoint(), **RUN))
case("mixed-resume-other-seeds", with_sigmas(), lambda s: EM(s, resume=mixed_checkpoint(seeds=[5, 6, 5]), **RUN))
case("mixed-resume-other-seeds-seed-drawn", with_sigmas(seed=None), lambda s: EM(s, resume=mixed_checkpoint(seeds=[5, 6, 5]), want_m_local=False, **RUN))
case("mixed-resume-other-streams", with_sigmas(), lambda s: EM(s, resume=mixed_checkpoint(), groups=[0, 1, 2], **RUN))
case("mixed-resume-other-large-keys", large, lambda s: EM(s, resume=mixed_checkpoint(make=large, N=40, seeds=[5, 5]), allow_large=True, **RUN))
case("structure_mixed-resume-other-k_max", with_sigmas(), lambda s: ETM(s, resume=mixed_checkpoint(structure=True), k_max=6, **RUN))
case("structure_mixed-resume-other-first_obs", with_sigmas(), lambda s: ETM(s, resume=mixed_checkpoint(structure=True), start_fraction=0.4, **RUN))
for tag, fn in (("mixed", EM), ("statistics_mixed", ESM), ("structure_mixed", ETM)):
    case(f"{tag}-obs_range-empty", with_sigmas(), lambda s, fn=fn: fn(s, obs_range=(4, 4), **RUN))
    case(f"{tag}-obs_range-beyond", with_sigmas(), lambda s, fn=fn: fn(s, obs_range=(0, 99), **RUN))
    case(f"{tag}-obs_range-late-start", with_sigmas(), lambda s, fn=fn: fn(s, obs_range=(2, 5), **RUN))
    case(f"{tag}-obs_per_launch-0", with_sigmas(), lambda s, fn=fn: fn(s, obs_per_launch=0, **RUN))
    case(f"{tag}-chain-lds-limit", with_sigmas(), lds_limit(fn, obs_per_launch=3))
    case(f"{tag}-chain-large", large, lambda s, fn=fn: fn(s, obs_per_launch=3, **RUN))
    case(f"{tag}-chain-differ", altered("k_off", 0.3), lambda s, fn=fn: fn(s, obs_per_launch=3, **RUN))
case("mixed-resume-large-not-allowed", large, lambda s: EM(s, resume=mixed_checkpoint(make=large, N=40), **RUN))
case("statistics_mixed-chain-k_exit", lambda: systems(k_exit=0.5), lambda s: ESM(s, obs_per_launch=3, **RUN))
# the library's side
case("mixed-chain-refused-second", with_sigmas(), lambda s: EM(s, obs_per_launch=3, want_m_local=False, **RUN), rc=-1, rc_after=1)
case("structure_mixed-chain-refused-second", with_sigmas(), lambda s: ETM(s, obs_per_launch=3, **RUN), rc=-5, rc_after=1)
case("exact-chain-refused-second", systems, lambda s: E(s, obs_per_launch=3, want_m_local=False, **RUN), rc=-1, rc_after=1)
case("mixed-chain-older-build", with_sigmas(), lambda s: EM(s, obs_per_launch=3, **RUN), missing=("gilxr_run",))
case("mixed-chain-allow_large-older-build", large, lambda s: EM(s, obs_per_launch=3, allow_large=True, **RUN), missing=("gilxmr_run",))
case("structure_mixed-chain-older-build", with_sigmas(), lambda s: ETM(s, obs_per_launch=3, **RUN), missing=("gilxsr_run",))
case("mixed-allow_large-older-build", large, lambda s: EM(s, allow_large=True, **RUN), missing=("gilxm_run",))
# MixedCheckpoint itself
case("mixed_checkpoint", none, lambda s: mixed_checkpoint(tables=True))
case("mixed_checkpoint-structure", none, lambda s: mixed_checkpoint(structure=True))
case("mixed_checkpoint-shapes", none, lambda s: mixed_checkpoint(next_obs=(1, 2)))
case("mixed_checkpoint-pos-1d", none, lambda s: mixed_checkpoint(pos=np.zeros(3)))
for name in ("n_slots", "seeds", "streams", "sigma_grids"):
    case(f"mixed_checkpoint-{name}-length", none, lambda s, name=name: mixed_checkpoint(**{name: [1, 2]}))
case("mixed_checkpoint-structure-without-window", none, lambda s: mixed_checkpoint(structure=True, window=None))
case("mixed_checkpoint-structure-without-first_obs", none, lambda s: mixed_checkpoint(structure=True, first_obs=None))
case("mixed_checkpoint-window-shape", none, lambda s: mixed_checkpoint(structure=True, window=np.zeros((3, 5, 3))))
case("mixed_checkpoint-n_window-shape", none, lambda s: mixed_checkpoint(structure=True, n_window=[0, 0]))
case("mixed_checkpoint-block_tables-shape", none, lambda s: mixed_checkpoint(block_tables=np.zeros((3, 3, 3))))
case("mixed_checkpoint-require-every-field", none, lambda s: mixed_checkpoint(structure=True).require(**mixed_checkpoint(structure=True).fingerprint()))
for name, other in (("n_cap", 21), ("large", True), ("n_slots", [20, 19, 20]), ("streams", [0, 1, 1]), ("anchor_mask", np.arange(64) == 3)):
    case(f"mixed_checkpoint-require-{name}", none, lambda s, name=name, other=other: mixed_checkpoint(structure=True).require(**{name: other}))
case("checkpoint-require-every-field", none, lambda s: checkpoint().require(**checkpoint().fingerprint()))
for name, other in (("K", 2), ("local_kernel_sigma", 0.01), ("n_cap", 21), ("anchor_mask", np.arange(64) == 3)):
    case(f"checkpoint-require-{name}", none, lambda s, name=name, other=other: checkpoint().require(**{name: other}))
# the raw functions and the plan
NEWER_RAW = (("run_mixed_many_raw", gil.run_mixed_many_raw, MIXED), ("run_mixed_resumable_raw", gil.run_mixed_resumable_raw, MIXED),
             ("run_mixed_resumable_raw-large", gil.run_mixed_resumable_raw, dict(MIXED, large=True)),
             ("run_mixed_structure_resumable_raw", gil.run_mixed_structure_resumable_raw, MIXED))
for tag, fn, extra in NEWER_RAW:
    full = dict(FULL, block_tables=np.arange(18).reshape(2, 3, 3) % 2, seeds=[2 ** 64 + 3, -1], streams=[4, 0], order=[1, 0], **extra)
    del full["block_table"]
    if "structure" in tag:
        full.update(k_max=3, first_obs=2, want_rows=False)
    if "resumable" in tag:
        full.update(obs_first=0)
    case(f"{tag}-defaults", none, lambda s, fn=fn, kw=extra: fn(**raw(**kw)))
    case(f"{tag}-every-keyword", none, lambda s, fn=fn, kw=full: fn(**raw(**kw)))
    case(f"{tag}-uniforms", none, lambda s, fn=fn, kw=extra: fn(**raw(uniforms=uniforms(2, 5), max_events=3, **kw)))
    case(f"{tag}-uniforms-shape", none, lambda s, fn=fn, kw=extra: fn(**raw(uniforms=uniforms(3, 5), **kw)))
    case(f"{tag}-n_cap-small", none, lambda s, fn=fn, kw=extra: fn(**raw(n_cap=4, **kw)))
    case(f"{tag}-empty-anchor-mask", none, lambda s, fn=fn, kw=extra: fn(**raw(anchor_mask=np.zeros(64, bool), betas=0.75, **kw)))
    case(f"{tag}-refused", none, lambda s, fn=fn, kw=extra: fn(**raw(**kw)), rc=-4)
    case(f"{tag}-no-variant_of_system", none, lambda s, fn=fn, kw=extra: fn(**raw(**dict(kw, variant_of_system=None))))
    case(f"{tag}-block_tables-shape", none, lambda s, fn=fn, kw=extra: fn(**raw(**dict(kw, block_tables=np.zeros((2, 2, 2))))))
CK_MIXED = dict(CK_RAW, n_slots=[5, 6])
CK_WINDOW = dict(CK_MIXED, window=np.arange(24).reshape(2, 4, 3) + 0.5, n_window=[1, 0], n_empty=[0, 2])
XR, XSR = gil.run_mixed_resumable_raw, gil.run_mixed_structure_resumable_raw
case("run_mixed_resumable_raw-checkpoint", none, lambda s: XR(**raw(checkpoint=CK_MIXED, obs_first=2, states=None, **MIXED)))
case("run_mixed_resumable_raw-checkpoint-large-n_cap", none, lambda s: XR(**raw(checkpoint=CK_MIXED, obs_first=3, states=None, n_cap=6, large=True, **MIXED)))
case("run_mixed_resumable_raw-checkpoint-with-window", none, lambda s: XR(**raw(checkpoint=CK_WINDOW, obs_first=2, states=None, **MIXED)))
case("run_mixed_structure_resumable_raw-checkpoint", none, lambda s: XSR(**raw(checkpoint=CK_WINDOW, obs_first=2, states=None, k_max=4, first_obs=3, **MIXED)))
case("run_mixed_structure_resumable_raw-checkpoint-no-rows", none, lambda s: XSR(**raw(checkpoint=CK_WINDOW, obs_first=4, states=None, k_max=4, first_obs=3,
                                                                                        want_rows=False, want_states=False, **MIXED)))
case("run_mixed_structure_resumable_raw-checkpoint-no-window", none, lambda s: XSR(**raw(checkpoint=CK_MIXED, obs_first=2, states=None, k_max=4, **MIXED)))
case("run_mixed_structure_resumable_raw-checkpoint-window-shape", none,
     lambda s: XSR(**raw(checkpoint=dict(CK_WINDOW, window=np.zeros((2, 3, 3))), states=None, k_max=4, **MIXED)))
case("run_mixed_structure_resumable_raw-checkpoint-n_empty-shape", none,
     lambda s: XSR(**raw(checkpoint=dict(CK_WINDOW, n_empty=[0]), states=None, k_max=4, **MIXED)))
case("run_mixed_structure_resumable_raw-k_max-0", none, lambda s: XSR(**raw(k_max=0, **MIXED)), ask_library=True)
for tag, fn, more in (("run_mixed_resumable_raw", XR, {}), ("run_mixed_structure_resumable_raw", XSR, dict(k_max=4))):
    case(f"{tag}-checkpoint-other-n_cap", none, lambda s, fn=fn, more=more: fn(**raw(checkpoint=CK_WINDOW, states=None, n_cap=7, **more, **MIXED)))
    case(f"{tag}-checkpoint-shapes", none, lambda s, fn=fn, more=more: fn(**raw(checkpoint=dict(CK_WINDOW, t=[0.25]), states=None, **more, **MIXED)))
    case(f"{tag}-checkpoint-n_slots-shape", none, lambda s, fn=fn, more=more: fn(**raw(checkpoint=dict(CK_WINDOW, n_slots=[5]), states=None, **more, **MIXED)))
    case(f"{tag}-checkpoint-no-n_slots", none, lambda s, fn=fn, more=more: fn(**raw(checkpoint=CK_RAW, states=None, **more, **MIXED)))
    case(f"{tag}-older-build", none, lambda s, fn=fn, more=more: fn(**raw(**more, **MIXED)), missing=("gilxr_run", "gilxsr_run"))
case("run_mixed_resumable_raw-large-older-build", none, lambda s: XR(**raw(large=True, **MIXED)), missing=("gilxmr_run",))
case("run_mixed_many_raw-older-build", none, lambda s: gil.run_mixed_many_raw(**raw(**MIXED)), missing=("gilxm_run",))
case("plan_mixed_many-order-length", none, lambda s: gil.plan_mixed_many(**dict(PLAN, sigma_grids=[1.0], order=[0])))

assert len({name for name, _, _, _ in CASES}) == len(CASES), "case names must be unique"


def run_case(name, make, call, standin):
    fake = StandIn(REAL(), name, **standin)
    saved, gil._lib = gil._lib, lambda: fake
    try:
        batch = make()
        try:
            got = {"result": crc_json(digest(call(batch)))}
        except (ValueError, TypeError, RuntimeError, AssertionError) as exc:
            got = {"error": [type(exc).__name__, str(exc)]}
    finally:
        gil._lib = saved
    got["calls"] = [f"{c['entry']}/{c['n_args']} " + " ".join(f"{k}:{crc_json(c[k])}" for k in sorted(c) if k not in ("entry", "n_args")) for c in fake.calls]
    if batch:
        got["systems"] = crc_json([[repr(getattr(ps, k, None)) for k in ("n_events", "kernel_ms", "bytes_back")] for ps in batch])
        got["rng"] = crc_json([digest(ps.rng.bit_generator.state) for ps in batch])
    return got, fake.calls


_real = []


def REAL():
    if not _real:
        _real.append(gil._lib())
    return _real[0]


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_and_case_list_agree(recorded):
    assert sorted(recorded) == sorted(name for name, _, _, _ in CASES)


@pytest.mark.parametrize("name,make,call,standin", CASES, ids=[name for name, _, _, _ in CASES])
def test_python_contract(recorded, name, make, call, standin):
    got, calls = run_case(name, make, call, standin)
    assert got == recorded[name], json.dumps(calls, indent=1)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_exact_loop_python_contract_cpu.py --record   (in a checkout of the commit to record from)")
    out = {name: run_case(name, make, call, standin)[0] for name, make, call, standin in CASES}
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(out[k], sort_keys=True)}" for k in sorted(out)) + "\n}\n")
    errors = sum("error" in v for v in out.values())
    print(f"{len(out)} cases ({errors} of them end in an exception) recorded from {gil.__file__} into {FIXTURE}")
