"""CPU suite: the mixed launch with ensemble profiles (include/gillespie_mixed_profile.h) as far as it can be checked without a
GPU -- the header and the exported symbols, gilxp_plan_info against its ctypes mirror, the plan's host arithmetic restated here
(LDS, bins, bytes, the shape rule with its three ways into the large shape), every refusal by the value it names, from the plan
and from gilxp_run before it looks for a device, and the Python side with a stand-in for gilxp_run: what
`run_batched_exact_profiles_mixed` and the two sweep drivers hand over, that the plan is asked before the keys are formed, their
refusals and the grouping of what they return.

One restatement differs from the plain sum "mixed launch's LDS + profile slots": in the batch shape the loop's bytes are
rounded up to 8 first (as gilp_plan_info documents for gilp_run), because the profile slots hold 64-bit words; with an odd
n_cap the mixed launch's own bytes end on a multiple of 4."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"
HEADER = "gillespie_mixed_profile.h"
NEW = ["gilxp_last_error", "gilxp_plan", "gilxp_run"]
ERR_ARG, ERR_NODEVICE = -1, -4
BATCH, LARGE = 0, 1
LDS_LIMIT = 160 * 1024


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


def include_dir(capi):
    return os.path.dirname(capi.HEADER_PATH)


def header_text(capi, name=HEADER):
    with open(os.path.join(include_dir(capi), name)) as fh:
        return fh.read()


# ---- header, exports, layout, argtypes

def test_header_declares_the_three_names_and_the_library_exports_them(capi):
    text = header_text(capi)
    assert sorted(set(re.findall(r"\b(gilxp_[a-z_0-9]+)\s*\(", text))) == NEW
    lib = C.CDLL(capi.LIB_PATH)
    for n in NEW:
        assert hasattr(lib, n), f"{n} declared in include/{HEADER} but not exported"
    for name in os.listdir(include_dir(capi)):                     # no other header knows the prefix
        if name != HEADER:
            assert not re.findall(r"\bgilxp_[a-z_0-9]+", header_text(capi, name)), name
    # nothing else in the library matches the prefix
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b\w*gilxp_\w*", out))) == NEW
    # gil_params and gilx_variants are reused, not restated
    for inc in ('"gillespie.h"', '"gillespie_mixed.h"', '"gillespie_profile.h"'):
        assert "#include " + inc in text
    assert "typedef struct gil_params" not in text and "typedef struct gilx_variants" not in text


def test_plan_info_matches_the_mirror_field_for_field(capi, gil, tmp_path):
    body = re.search(r"typedef struct gilxp_plan_info \{(.*?)\} gilxp_plan_info;", header_text(capi), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.split() for d in body.split(";") if d.strip()]
    fields = [d[-1] for d in decls]
    assert fields == [f[0] for f in gil.GilxpPlanInfo._fields_] == ["shape", "threads", "lds_bytes", "max_tlen", "bin_width", "n_bins_used",
                                                                    "table_doubles", "work_bytes", "output_bytes"]
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    assert [ctype[d[0]] for d in decls] == [f[1] for f in gil.GilxpPlanInfo._fields_]
    prints = "".join(f'printf("%zu ", offsetof(gilxp_plan_info, {f}));' for f in fields)
    src = (f'#include "{HEADER}"\n#include <stddef.h>\n#include <stdio.h>\n'
           'int main(){printf("%zu ", sizeof(gilxp_plan_info));' + prints + 'return 0;}\n')
    c, exe = tmp_path / "s.c", tmp_path / "s"
    c.write_text(src)
    subprocess.run(["gcc", "-I", include_dir(capi), str(c), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(gil.GilxpPlanInfo) == 6 * 4 + 3 * 8
    assert got[1:] == [getattr(gil.GilxpPlanInfo, f).offset for f in fields]


def test_argtypes(gil):
    lib = gil._lib()
    x, p, xp = lib.gilx_run.argtypes, lib.gilp_run.argtypes, lib.gilxp_run.argtypes
    profile_in, profile_out = p[1:6], p[-4:-1]                     # n_bins, first_obs, want_field, group_of_system, n_groups; the three outputs
    assert profile_in == [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32] and profile_out == [C.c_void_p] * 3
    assert xp == x[:2] + profile_in + x[2:-1] + profile_out + x[-1:]
    assert len(xp) == 2 + 5 + 14 + 3 + 1 and xp[1] == C.POINTER(gil.GilxVariants)
    e = gil.ENTRIES["gilxp_run"]
    assert e.last_error == "gilxp_last_error" and e.header == "include/" + HEADER
    assert lib.gilxp_plan.argtypes == [C.POINTER(gil.GilParams), C.POINTER(gil.GilxVariants)] + [C.c_int32] * 6 + [C.POINTER(gil.GilxpPlanInfo)]
    assert lib.gilxp_last_error.restype == C.c_char_p


# ---- the plan's arithmetic, restated

def _profile_bytes(n_bins, field):
    return 8 * -(-3 * n_bins // 2) + (8 * n_bins if field else 0)


def _outputs(S, O, N, G, B, states, per_system):
    """gilp_plan_info's formula"""
    return S * ((O * N * 6 if states else 0) + O * 12 * 8 + N * 24 + 24) + G * O * (7 * B * 8 + 4) + (S * O * 3 * B * 4 if per_system else 0)


def _bins(L, n_bins):
    width = -(-L // n_bins)
    return width, -(-L // width)


def test_plan_batch_shape(gil):
    mixed = dict(K=2, periodic=False, sigma_grids=[5.0, 0.0, 2.0], n_systems=7, n_obs=41)
    for L, n_cap, n_bins, field, threads in ((160, 100, 33, True, 64), (160, 101, 7, False, 64), (900, 1100, 900, True, 256), (64, 17, 64, True, 64)):
        own = gil.plan_mixed(L=L, n_cap=n_cap, **mixed)
        p = gil.plan_mixed_profiles(L=L, n_cap=n_cap, n_bins=n_bins, n_groups=3, want_field=field, per_system=not field, **mixed)
        width, used = _bins(L, n_bins)
        assert p == dict(shape=BATCH, threads=threads, lds_bytes=((own["lds_bytes"] + 7) & ~7) + _profile_bytes(n_bins, field),
                         max_tlen=own["max_tlen"], bin_width=width, n_bins_used=used, table_doubles=own["table_doubles"], work_bytes=7 * 4,
                         output_bytes=_outputs(7, 41, n_cap, 3, n_bins, True, not field)), (L, n_cap)
        assert own["threads"] == threads and own["max_tlen"] == 21     # sigma_grid = 5 with walls: taps at distances 0 .. 20
    assert gil.plan_mixed(L=160, n_cap=101, **mixed)["lds_bytes"] % 8 == 4      # the case above exercises the rounding
    assert _profile_bytes(33, True) == 8 * 50 + 8 * 33 and _profile_bytes(7, False) == 8 * 11
    assert (_bins(1001, 7), _bins(1000, 300), _bins(1000, 7), _bins(64, 1)) == ((143, 7), (4, 250), (143, 7), (64, 1))
    kw = dict(K=1, periodic=True, sigma_grids=[0.0, 1.5], n_systems=2, n_cap=10, n_obs=2)
    for L, n_bins in ((1001, 7), (1000, 300), (1000, 1000), (1000, 7), (64, 1)):
        p = gil.plan_mixed_profiles(L=L, n_bins=n_bins, **kw)
        assert (p["bin_width"], p["n_bins_used"]) == _bins(L, n_bins)


def test_plan_shape_rule(gil):
    mixed = dict(K=1, periodic=False, sigma_grids=[5.0, 2.0], n_systems=3, n_obs=5)

    def large(L, n_cap, n_bins, field, **more):
        kw = dict(mixed, **more)
        own = gil.plan_mixed_many(L=L, n_cap=n_cap, **kw)
        p = gil.plan_mixed_profiles(L=L, n_cap=n_cap, n_bins=n_bins, want_field=field, **kw)
        width, used = _bins(L, n_bins)
        S = kw["n_systems"]
        assert p == dict(shape=LARGE, threads=1024, lds_bytes=own["lds_bytes"] + _profile_bytes(n_bins, field), max_tlen=own["max_tlen"],
                         bin_width=width, n_bins_used=used, table_doubles=own["table_doubles"], work_bytes=S * own["work_bytes_per_system"] + S * 4,
                         output_bytes=_outputs(S, 5, n_cap, 1, n_bins, True, False)), (L, n_cap)
        return p

    assert gil.plan_mixed_profiles(L=4096, n_cap=100, n_bins=16, **mixed)["shape"] == BATCH
    large(4097, 100, 16, False)                                    # one site more
    assert gil.plan_mixed_profiles(L=1000, n_cap=2048, n_bins=16, **mixed)["shape"] == BATCH
    large(1000, 2049, 16, True)                                    # one slot more
    large(10050, 40, 1000, True, sigma_grids=[2613.0, 20.1, 0.0])  # a table read from global memory beside one kept in LDS
    # the profile slots alone push a launch that gilx_run takes over the 160 KB: the largest shape with the longest table
    tight = dict(K=1, periodic=False, sigma_grids=[600.0, 5.0], n_systems=1, n_obs=5, L=4096, n_cap=2048)
    own = (gil.plan_mixed(**tight)["lds_bytes"] + 7) & ~7
    assert own + _profile_bytes(4, False) <= LDS_LIMIT < own + _profile_bytes(1024, True)     # found with the test's own formula
    p = gil.plan_mixed_profiles(n_bins=4, **tight)
    assert (p["shape"], p["threads"], p["lds_bytes"]) == (BATCH, 256, own + _profile_bytes(4, False))
    large(4096, 2048, 1024, True, **{k: v for k, v in tight.items() if k not in ("L", "n_cap")})


# ---- refusals

def _refused(capi, call, text):
    with pytest.raises(capi.ApsError) as exc:
        call()
    assert exc.value.code == ERR_ARG and str(exc.value).endswith(text), str(exc.value)


def test_plan_refusals_name_the_value(capi, gil):
    kw = dict(L=1000, K=1, periodic=False, sigma_grids=[5.0, 0.0], n_systems=2, n_cap=900, n_obs=41)
    for bad, text in ((dict(n_bins=0), "gilxp_plan: n_bins = 0 is outside [1, min(L, GILP_MAX_BINS) = 1000]"),
                      (dict(n_bins=1001), "gilxp_plan: n_bins = 1001 is outside [1, min(L, GILP_MAX_BINS) = 1000]"),
                      (dict(n_bins=10, n_groups=0), "gilxp_plan: n_groups = 0 is outside [1, 4096]"),
                      (dict(n_bins=10, n_groups=4097), "gilxp_plan: n_groups = 4097 is outside [1, 4096]"),
                      (dict(n_bins=10, first_obs=42), "gilxp_plan: first_obs = 42 is outside [0, n_obs = 41]"),
                      (dict(n_bins=10, first_obs=-1), "gilxp_plan: first_obs = -1 is outside [0, n_obs = 41]"),
                      (dict(n_bins=10, want_field=2), "gilxp_plan: want_field = 2 is neither 0 nor 1"),
                      # the mixed launch's refusals come first
                      (dict(n_bins=0, sigma_grids=[5.0, -1.0]), "gilxp_plan: sigma_grid = -1.000000 of variant 1 must be finite and not negative"),
                      (dict(n_bins=0, variant_of_system=[0, 2]), "gilxp_plan: variant index 2 of system 1 is outside [0, n_variants = 2)"),
                      (dict(n_bins=0, order=[1, 1]), "gilxp_plan: order is not a permutation: system 1 appears twice (second time at 1)"),
                      (dict(n_bins=0, sigma_grids=[]), "gilxp_plan: n_variants = 0 is outside [1, 4096]")):
        _refused(capi, lambda: gil.plan_mixed_profiles(**dict(kw, **bad)), text)
    _refused(capi, lambda: gil.plan_mixed_profiles(n_bins=1025, **dict(kw, L=3000)), "gilxp_plan: n_bins = 1025 is outside [1, min(L, GILP_MAX_BINS) = 1024]")
    # in the large shape the same order: gilxm_plan's limits, then the profile's
    _refused(capi, lambda: gil.plan_mixed_profiles(n_bins=0, **dict(kw, L=(1 << 25) + 1)), f"gilxp_plan: L = {(1 << 25) + 1} is outside [2, 2^25 = {1 << 25}]")
    _refused(capi, lambda: gil.plan_mixed_profiles(n_bins=0, **dict(kw, L=5000)), "gilxp_plan: n_bins = 0 is outside [1, min(L, GILP_MAX_BINS) = 1024]")
    assert gil.plan_mixed_profiles(n_bins=1000, n_groups=4096, first_obs=41, want_field=True, **kw)["n_bins_used"] == 1000
    # the fixed-point field sum: L * n_systems = 2^31 is refused, one system fewer is not
    wide = dict(K=1, periodic=True, sigma_grids=[0.0], n_cap=4, n_obs=1, L=1 << 16, n_bins=8, want_states=False)
    _refused(capi, lambda: gil.plan_mixed_profiles(n_systems=1 << 15, want_field=True, **wide),
             f"gilxp_plan: want_field with L * n_systems = {1 << 31} >= 2^31: the fixed-point field sum could overflow 64 bits")
    assert gil.plan_mixed_profiles(n_systems=(1 << 15) - 1, want_field=True, **wide)["shape"] == LARGE
    with pytest.raises(capi.ApsError) as exc:                          # 4096 x 4096 x 7 x 1024 x 8 bytes of sums
        gil.plan_mixed_profiles(n_bins=1024, n_groups=4096, want_states=False, **dict(kw, L=2000, n_obs=4096))
    assert exc.value.code == ERR_ARG and "gilxp_plan: the batch needs" in str(exc.value)
    assert str(exc.value).endswith(f"more than the {1 << 38} bytes a plan accepts")


def _direct_call(gil, L=64, sigma_grids=(2.0, 0.0)):
    """gilxp_run by ctypes on two one-particle systems; returns call(**changes) -> (rc, text)"""
    lib = gil._lib()
    keep = [np.array([0.5, 0.5]), np.array([0.0, 0.01]), np.array([1, 1], np.int32), np.array([0, 3], np.int32), np.array([1, -1], np.int8),
            np.zeros(3 * 2 * 7 * 8, np.int64), np.zeros(3 * 2, np.int32)]
    par = gil.GilParams(L=L, K=1, periodic=1, n_systems=2, n_cap=1, n_obs=2, ref_obs=-1, rate_diffusion=0.1, rate_active=1.0, T=0.01,
                        max_events=16, beta=keep[0].ctypes.data, times_obs=keep[1].ctypes.data)
    desc, keep_desc = gil._mixed_descriptor(2, 1, list(sigma_grids), [0, 1])
    ms = C.c_double()

    def call(n_bins=8, first_obs=0, want_field=0, groups=None, n_groups=3, sums=keep[5], members=keep[6], p=par, v=desc):
        rc = lib.gilxp_run(C.byref(p), None if v is None else C.byref(v), n_bins, first_obs, want_field, gil._p(groups), n_groups, gil._p(keep[2]),
                           gil._p(keep[3]), gil._p(keep[4]), *[None] * 11, gil._p(sums), gil._p(members), None, C.byref(ms))
        return rc, lib.gilxp_last_error().decode()

    call.keep, call.par = (keep, keep_desc, desc), par
    return call


def test_run_refusals_come_before_any_device(capi, gil):
    call = _direct_call(gil)
    assert call(sums=None) == (ERR_ARG, "gilxp_run: null argument")      # the two ensemble outputs are required
    assert call(members=None) == (ERR_ARG, "gilxp_run: null argument")
    assert call(v=None) == (ERR_ARG, "gilxp_run: null argument")
    assert call(n_bins=65) == (ERR_ARG, "gilxp_run: n_bins = 65 is outside [1, min(L, GILP_MAX_BINS) = 64]")
    assert call(n_bins=0) == (ERR_ARG, "gilxp_run: n_bins = 0 is outside [1, min(L, GILP_MAX_BINS) = 64]")
    assert call(n_groups=0) == (ERR_ARG, "gilxp_run: n_groups = 0 is outside [1, 4096]")
    assert call(n_groups=5000) == (ERR_ARG, "gilxp_run: n_groups = 5000 is outside [1, 4096]")
    assert call(first_obs=3) == (ERR_ARG, "gilxp_run: first_obs = 3 is outside [0, n_obs = 2]")
    assert call(first_obs=-1) == (ERR_ARG, "gilxp_run: first_obs = -1 is outside [0, n_obs = 2]")
    assert call(want_field=-1) == (ERR_ARG, "gilxp_run: want_field = -1 is neither 0 nor 1")
    assert call(groups=np.array([0, 3], np.int32)) == (ERR_ARG, "gilxp_run: group id 3 of system 1 is outside [0, n_groups = 3)")
    assert call(groups=np.array([-1, 2], np.int32)) == (ERR_ARG, "gilxp_run: group id -1 of system 0 is outside [0, n_groups = 3)")
    bad_desc, keep = gil._mixed_descriptor(2, 1, [2.0, 0.0], [0, 2])      # the mixed launch's refusal comes before the profile's
    assert call(n_bins=0, v=bad_desc) == (ERR_ARG, "gilxp_run: variant index 2 of system 1 is outside [0, n_variants = 2)")
    huge = gil.GilParams.from_buffer_copy(call.par)
    huge.L, huge.n_systems = 1 << 16, 1 << 15                            # the numbers are checked before any array is read
    wide, keep2 = gil._mixed_descriptor(1 << 15, 1, [0.0], np.zeros(1 << 15, np.int32))
    rc, text = call(want_field=1, p=huge, v=wide)
    assert rc == ERR_ARG and text == f"gilxp_run: want_field with L * n_systems = {1 << 31} >= 2^31: the fixed-point field sum could overflow 64 bits"
    nobody, keep3 = gil._mixed_descriptor(2, 1, [2.0, 0.0], None)
    assert call(v=nobody) == (ERR_ARG, "gilxp_run: null argument")       # variant_of_system is required by the run
    # an acceptable call fails loudly where no device is, in both shapes (or runs where one is)
    rc, text = call(groups=np.array([2, 0], np.int32), want_field=1)
    assert (rc, text) == (ERR_NODEVICE, "gilxp_run: no HIP device") or rc == 0
    rc, text = _direct_call(gil, L=4100)(groups=np.array([2, 0], np.int32), want_field=1)
    assert (rc, text) == (ERR_NODEVICE, "gilxp_run: no HIP device") or rc == 0
    # the Python entry point refuses the same, by the library's text
    common = dict(L=64, K=1, periodic=True, sigma_grids=[2.0, 0.0], variant_of_system=[0, 1], rate_diffusion=0.1, rate_active=1.0, betas=[0.5, 0.5],
                  states=[(np.array([0]), np.array([1])), (np.array([3]), np.array([-1]))], times_obs=[0.0, 0.01], T=0.01, max_events=16)
    for bad, text in ((dict(n_bins=65), "n_bins = 65 is outside"), (dict(n_bins=8, group_of_system=[0, 2], n_groups=2), "group id 2 of system 1"),
                      (dict(n_bins=8, first_obs=3), "first_obs = 3 is outside"), (dict(n_bins=8, n_groups=0), "n_groups = 0 is outside")):
        with pytest.raises(capi.ApsError) as exc:
            gil.run_mixed_profiles_raw(**common, **bad)
        assert exc.value.code == ERR_ARG and "gilxp_run: " in str(exc.value) and text in str(exc.value), (bad, str(exc.value))
    with pytest.raises(ValueError):
        gil.run_mixed_profiles_raw(n_bins=8, group_of_system=[0, 1, 1], **common)     # one id per system
    if capi.device_count() == 0:
        with pytest.raises(capi.ApsError) as exc:
            gil.run_mixed_profiles_raw(n_bins=8, group_of_system=[0, 1], **common)
        assert exc.value.code == ERR_NODEVICE and "gilxp_run: no HIP device" in str(exc.value)


# ---- the Python side, with a stand-in for gilxp_run (the method of tests/test_exact_loop_python_contract_cpu.py, restated for the
# one entry point: its ENTRIES table does not know gilxp_run)

def _array(address, dtype, n):
    if address is None or (isinstance(address, C.c_void_p) and not address.value):
        return None
    a = address.value if isinstance(address, C.c_void_p) else int(address)
    return np.frombuffer(C.string_at(a, n * np.dtype(dtype).itemsize), dtype=dtype).copy()


def _fill(address, values):
    values = np.ascontiguousarray(values)
    C.memmove(address.value, values.ctypes.data, values.nbytes)


class StandIn:
    """What gillespie._lib() returns during a case: gilxp_run is noted and answered with what a launch could return (every system
    records every observation, every group's members are its systems, sums that tell group, observation and column apart);
    everything else -- the plans, host arithmetic -- is the real library's."""

    def __init__(self, real, log, missing=()):
        self.real, self.log, self.missing, self.calls = real, log, missing, []

    def __getattr__(self, attr):
        if attr.startswith("__") or attr in self.missing:
            raise AttributeError(attr)
        if attr == "gilxp_run":
            return self.run
        if attr == "gilp_run":
            return self.unmixed
        return getattr(self.real, attr)

    def unmixed(self, *args):
        self.log.append("gilp_run")
        return -1

    def run(self, *args):
        self.log.append("gilxp_run")
        assert len(args) == 25
        par, v = args[0]._obj, args[1]._obj
        S, N, M, V = par.n_systems, par.n_cap, par.n_obs, v.n_variants
        n_bins, first_obs, want_field, _, n_groups = args[2:7]
        rec = dict(L=par.L, K=par.K, S=S, n_cap=N, n_obs=M, T=par.T, par_sigma_grid=par.sigma_grid, par_block_table=par.block_table,
                   n_bins=n_bins, first_obs=first_obs, want_field=want_field, n_groups=n_groups, n_variants=V,
                   groups=_array(args[5], np.int32, S), sigma_grid=_array(v.sigma_grid, np.float64, V), block_table=v.block_table,
                   variant_of_system=_array(v.variant_of_system, np.int32, S), seed=_array(v.seed, np.uint64, S),
                   stream=_array(v.stream, np.int32, S), order=_array(v.order, np.int32, S), n0=_array(args[7], np.int32, S),
                   betas=_array(par.beta, np.float64, S), want_states=args[12] is not None, per_system=args[23] is not None)
        self.calls.append(rec)
        _fill(args[16], np.full(S, M, np.int32))                   # n_recorded
        _fill(args[17], np.arange(100, 100 + S, dtype=np.int64))   # n_events
        g, k, c, b = np.meshgrid(np.arange(n_groups), np.arange(M), np.arange(7), np.arange(n_bins), indexing="ij")
        _fill(args[21], (1000 * g + 10 * k + c + (b == 0)).astype(np.int64))
        members = np.bincount(rec["groups"], minlength=n_groups).astype(np.int32)
        _fill(args[22], np.repeat(members[:, None], M, axis=1))
        args[24]._obj.value = 1.5
        return 0


SIGMAS = (0.3, 0.3, 0.05, 0.3, 0.0, 0.05)


def _systems(psm, sigmas=SIGMAS, L=64, N=20, seeds=None, **kw):
    seeds = [100 + i for i in range(len(sigmas))] if seeds is None else seeds
    return [psm.ParticleSystem(L, 1.0, 0.01, 0.1, 0.5 + 0.25 * i, N=N, seed=seeds[i], rng=np.random.default_rng(100 + i), local_kernel_sigma=sg, **kw)
            for i, sg in enumerate(sigmas)]


@pytest.fixture()
def stand_in(gil, monkeypatch):
    log = []
    real = gil._lib()
    box = StandIn(real, log)
    monkeypatch.setattr(gil, "_lib", lambda: box)
    for name in ("plan_mixed_profiles", "mixed_keys"):
        def wrapped(*a, _f=getattr(gil, name), _n=name, **kw):
            log.append(_n)
            out = _f(*a, **kw)
            if _n == "mixed_keys":
                box.keys_large = kw.get("large", False)
            return out
        monkeypatch.setattr(gil, name, wrapped)
    return box


def test_what_the_mixed_profile_function_hands_over(gil, stand_in):
    psm = importlib.import_module(PKG + ".particle_system")
    sys_ = _systems(psm)
    groups, key_groups = [0, 1, 1, 0, 2, 2], [0, 0, 1, 1, 1, 0]
    out = gil.run_batched_exact_profiles_mixed(sys_, T=0.2, obs_dt=0.02, n_bins=7, groups=groups, key_groups=key_groups, order=[5, 4, 3, 2, 1, 0],
                                               first_obs=2, want_field=True, per_system=True)
    assert stand_in.log == ["plan_mixed_profiles", "mixed_keys", "gilxp_run"]       # the plan before the keys
    (c,) = stand_in.calls
    sg = [ps._sigma_grid for ps in sys_]
    assert c["sigma_grid"].tolist() == [sg[0], sg[2], sg[4]] and sg[4] == 0.0        # variants in the order of first appearance
    assert c["variant_of_system"].tolist() == [0, 0, 1, 0, 2, 1] and c["n_variants"] == 3
    # mixed_keys with key_groups, restated: the key is the seed of the key group's first system, the stream the place within it
    assert c["seed"].tolist() == [100, 100, 102, 102, 102, 100] and c["stream"].tolist() == [0, 1, 0, 1, 2, 2]
    assert c["groups"].tolist() == groups and c["n_groups"] == 3 and c["order"].tolist() == [5, 4, 3, 2, 1, 0]
    assert (c["n_cap"], c["n0"].tolist(), c["S"], c["n_obs"]) == (20, [20] * 6, 6, 10)
    assert (c["n_bins"], c["first_obs"], c["want_field"], c["want_states"], c["per_system"]) == (7, 2, 1, False, True)
    assert c["par_sigma_grid"] == 0.0 and not c["par_block_table"] and not c["block_table"]
    assert c["betas"].tolist() == [0.5 + 0.25 * i for i in range(6)]
    # one result per ensemble group, in the order of the ids, from that group's rows
    assert len(out) == 3 and [o["members"].tolist() for o in out] == [[2] * 10] * 3
    for g, o in enumerate(out):
        assert o["profile_obs"].shape == (2, 10, 3, 7) and o["bin_width"] == 10 and o["n_bins_used"] == 7
        np.testing.assert_array_equal(o["plus_mean"][:, 1], (1000 * g + 10 * np.arange(10)) / 2)      # column 0, a bin that is not bin 0
        np.testing.assert_array_equal(o["minus_mean"][:, 0], (1000 * g + 10 * np.arange(10) + 2) / 2)
        assert "field_mean" in o
    assert [ps.n_events for ps in sys_] == list(range(100, 106)) and sys_[0].kernel_ms == 1.5


def test_defaults_and_refusals_of_the_mixed_profile_function(capi, gil, stand_in):
    psm = importlib.import_module(PKG + ".particle_system")
    out = gil.run_batched_exact_profiles_mixed(_systems(psm), T=0.2, obs_dt=0.02)
    (c,) = stand_in.calls
    assert c["n_bins"] == 64 and c["n_groups"] == 1 and c["groups"].tolist() == [0] * 6 and c["order"] is None and len(out) == 1
    assert c["seed"].tolist() == [100] * 6 and c["stream"].tolist() == list(range(6)) and not c["per_system"] and c["want_field"] == 0
    # resume: profiles have no resumable form
    with pytest.raises(ValueError, match="run_batched_exact_profiles_mixed cannot resume from a checkpoint"):
        gil.run_batched_exact_profiles_mixed(_systems(psm), T=0.2, obs_dt=0.02, resume=object())
    # a large plan without allow_large: the other mixed functions' text; nothing is launched and no key is formed
    del stand_in.log[:], stand_in.calls[:]
    big = _systems(psm, sigmas=(0.3, 0.05), L=4100, N=40)
    with pytest.raises(ValueError) as exc:
        gil.run_batched_exact_profiles_mixed(big, T=0.2, obs_dt=0.02, n_bins=100)
    assert str(exc.value) == ("run_batched_exact_profiles_mixed: L = 4100, N = 40 is a large shape (beyond L = 4096, N = 2048); "
                              "the large-system kernel takes no mixed batches")
    assert stand_in.log == ["plan_mixed_profiles"] and not stand_in.calls
    with pytest.raises(ValueError) as other:
        gil.run_batched_exact_mixed(_systems(psm, sigmas=(0.3, 0.05), L=4100, N=40), T=0.2, obs_dt=0.02)
    assert str(other.value) == str(exc.value).replace("run_batched_exact_profiles_mixed", "run_batched_exact_mixed")
    # with allow_large the keys are the large shape's: key + place within the key group, stream 0
    del stand_in.log[:]
    out = gil.run_batched_exact_profiles_mixed(_systems(psm, sigmas=(0.3, 0.05, 0.3), L=4100, N=40), T=0.2, obs_dt=0.02, n_bins=100,
                                               key_groups=[0, 1, 0], groups=[0, 1, 0], allow_large=True)
    assert stand_in.log == ["plan_mixed_profiles", "mixed_keys", "gilxp_run"] and stand_in.keys_large
    c = stand_in.calls[-1]
    assert c["seed"].tolist() == [100, 101, 101] and c["stream"].tolist() == [0, 0, 0] and len(out) == 2
    # the profile slots alone make the plan a large one (L = 4096, N = 2048, the longest table, 1024 bins with the field)
    tight = _systems(psm, sigmas=(0.15,), L=4096, N=2048)
    assert tight[0]._sigma_grid > 600.0
    with pytest.raises(ValueError, match="is a large shape"):
        gil.run_batched_exact_profiles_mixed(tight, T=0.2, obs_dt=0.02, n_bins=1024, want_field=True)
    # an older build without the entry point: the error names the header
    stand_in.missing = ("gilxp_run",)
    with pytest.raises(capi.ApsError, match=r"the loaded library has no gilxp_run \(include/gillespie_mixed_profile.h\)"):
        gil.run_batched_exact_profiles_mixed(_systems(psm), T=0.2, obs_dt=0.02)


def test_what_the_two_sweep_drivers_hand_over(ens, gil, stand_in):
    ps_kwargs = dict(L=64, xlim=1.0, rate_diffusion=0.01, rate_active=0.1, site_capacity=1)
    run_kwargs, seeds = dict(T=0.2, obs_dt=0.02), [[1, 2], [3, 4], [5, 6]]
    betas, sigmas = [0.5, 1.0, 2.0], [0.3, 0.0, 0.05]
    res = ens.profile_sweep_over_sigmas(sigmas, betas, 2, ps_kwargs, dict(N=20), run_kwargs, 16, rng_seeds=seeds, want_field=True)
    assert stand_in.log == ["plan_mixed_profiles", "mixed_keys", "gilxp_run"]
    (c,) = stand_in.calls
    assert c["S"] == 18 and c["n_groups"] == 9 and c["n_bins"] == 16 and c["want_field"] == 1 and c["n_cap"] == 20
    assert c["groups"].tolist() == [g for g in range(9) for _ in range(2)]           # (sigma index, beta index), sigma outermost
    assert c["variant_of_system"].tolist() == [v for v in range(3) for _ in range(6)] and c["sigma_grid"].tolist() == [0.3 * 64, 0.0, 0.05 * 64]
    assert c["stream"].tolist() == list(range(6)) * 3                                # the key group is the sigma index
    assert [len(set(c["seed"][6 * si:6 * si + 6])) for si in range(3)] == [1, 1, 1]  # one key per sigma, drawn from its first system's rng
    assert c["betas"].tolist() == [b for _ in range(3) for b in betas for _ in range(2)]
    assert list(res) == sigmas and all(list(res[s]) == betas for s in sigmas)
    for si, s in enumerate(sigmas):
        for bi, b in enumerate(betas):                                               # each entry is its own group's row
            np.testing.assert_array_equal(res[s][b]["plus_mean"][:, 1], (1000 * (3 * si + bi) + 10 * np.arange(10)) / 2)
    # the density driver: the group is (N index, beta index), the key group the N index, one variant, n_cap the largest N
    del stand_in.log[:], stand_in.calls[:]
    res = ens.profile_sweep_over_densities([10, 30.0], betas[:2], 2, dict(ps_kwargs, local_kernel_sigma=0.05), {}, run_kwargs, 8, rng_seeds=seeds)
    (c,) = stand_in.calls
    assert c["S"] == 8 and c["n_groups"] == 4 and c["n_cap"] == 30 and c["n0"].tolist() == [10] * 4 + [30] * 4
    assert c["groups"].tolist() == [0, 0, 1, 1, 2, 2, 3, 3] and c["stream"].tolist() == [0, 1, 2, 3] * 2 and c["n_variants"] == 1
    assert list(res) == [10, 30] and list(res[30]) == betas[:2]
    np.testing.assert_array_equal(res[30][1.0]["plus_mean"][:, 1], (1000 * 3 + 10 * np.arange(10)) / 2)
    # refusals: unknown run_kwargs, the stepper, fractional particle numbers
    with pytest.raises(ValueError, match=r"run_kwargs may hold T and obs_dt; got \['record_fft'\]"):
        ens.profile_sweep_over_sigmas(sigmas, betas, 2, ps_kwargs, dict(N=20), dict(run_kwargs, record_fft=True), 16)
    with pytest.raises(ValueError, match=r"run_kwargs may hold T and obs_dt; got \['k_max'\]"):
        ens.profile_sweep_over_densities([10], betas, 2, ps_kwargs, {}, dict(k_max=3), 16)
    with pytest.raises(ValueError, match="profile_sweep_over_sigmas needs the exact dynamics"):
        ens.profile_sweep_over_sigmas(sigmas, betas, 2, dict(ps_kwargs, dt=0.01), dict(N=20), run_kwargs, 16)
    with pytest.raises(ValueError, match="particle numbers must be integral"):
        ens.profile_sweep_over_densities([10.5], betas, 2, ps_kwargs, {}, run_kwargs, 16)
    # one_launch=False is the host loop: one gilp_run launch per outer value, no mixed launch
    del stand_in.log[:]
    with pytest.raises(Exception):
        ens.profile_sweep_over_sigmas(sigmas, betas, 2, ps_kwargs, dict(N=20), run_kwargs, 16, one_launch=False)
    assert stand_in.log == ["gilp_run"]
