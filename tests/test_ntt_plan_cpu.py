"""CPU suite: aps_ntt_plan (include/aps.h), the rule by which a single handle cuts its lattice into blocks for the exact
convolution (csrc/ntt_conv.hpp).  Pure host arithmetic: no GPU is touched."""
import ctypes
import importlib
import os

import pytest

PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"


@pytest.fixture(scope="module")
def capi():
    mod = importlib.import_module(PKG + ".capi")
    if not os.path.exists(mod.LIB_PATH):
        importlib.import_module(PKG + ".build").build()
    return mod


def smallest_m(span, primes):
    m = 15 if primes == 2 else 14
    while (1 << m) < span:
        m += 1
    return m


def check_tiling(plan, L, Rt, primes, cap):
    """The blocks tile [0, L) disjointly, the last one is not empty, a block and its overlap fit its transform, which fits the cap."""
    B, S, m = plan["blocks"], plan["block_sites"], plan["log2_m"]
    assert B >= 1 and S >= 1, plan
    ranges = [(b * S, min(L, (b + 1) * S)) for b in range(B)]
    assert ranges[0][0] == 0 and ranges[-1][1] == L, (plan, L)
    assert all(lo < hi for lo, hi in ranges), (plan, L)                       # none empty, the last one included
    assert all(ranges[b][1] == ranges[b + 1][0] for b in range(B - 1)), (plan, L)
    assert S + 2 * Rt <= (1 << m), (plan, L, Rt)
    assert (15 if primes == 2 else 14) <= m <= cap, (plan, cap)
    assert m == smallest_m(S + 2 * Rt, primes), (plan, L, Rt)
    assert B == -(-L // ((1 << cap) - 2 * Rt)), (plan, L, Rt, cap)           # the rule: as few blocks as the cap allows


@pytest.mark.parametrize("primes", [1, 2])
def test_one_block_wherever_one_transform_holds_the_lattice(capi, primes):
    """L + 2 Rt <= 2^21: one block with the smallest admissible m -- the plan of a handle before there were blocks."""
    top = 1 << 21
    for L in (2, 100, 16000, 16384, 90000, 120000, 1 << 20, 2_000_000, top - 2 * 40000, top):
        for Rt in (0, 1, 191, 2400, 8192, 40000, 250000, 524288):
            if L + 2 * Rt > top:
                continue
            plan = capi.ntt_plan(L, Rt, primes)
            assert plan == dict(blocks=1, log2_m=smallest_m(L + 2 * Rt, primes), block_sites=L), (L, Rt, plan)
            assert plan == capi.ntt_plan(L, Rt, primes, max_log2=21) == capi.ntt_plan(L, Rt, primes, max_log2=30)
    # BASELINE config 5 (L = 2e6, Rt = 40000) sits under the edge; the first lattice past it takes two blocks
    assert capi.ntt_plan(2_000_000, 40000, primes) == dict(blocks=1, log2_m=21, block_sites=2_000_000)
    assert capi.ntt_plan(top - 80000 + 1, 40000, primes)["blocks"] == 2


@pytest.mark.parametrize("primes", [1, 2])
def test_blocks_beyond_the_cap(capi, primes):
    for L in (2_097_153, 2_200_000, 4_000_000, 4_000_001, 10_000_019, 1 << 25):
        for Rt in (0, 4400, 40000, 300000, 524288):
            plan = capi.ntt_plan(L, Rt, primes)
            assert plan["blocks"] >= 2 or L + 2 * Rt <= (1 << 21), (L, Rt, plan)
            check_tiling(plan, L, Rt, primes, 21)
    # BASELINE config 5 at twice the size (sigma = 0.005 of L = 4e6 sites: Rt = 80000): three blocks of full length
    assert capi.ntt_plan(4_000_000, 80000, primes) == dict(blocks=3, log2_m=21, block_sites=1_333_334)
    assert capi.ntt_plan(2_200_000, 4400, primes) == dict(blocks=2, log2_m=21, block_sites=1_100_000)


@pytest.mark.parametrize("primes", [1, 2])
@pytest.mark.parametrize("cap", [14, 15, 16])
def test_small_caps_cut_small_lattices(capi, primes, cap):
    if cap < (15 if primes == 2 else 14):
        assert capi.ntt_plan(60000, 100, primes, max_log2=cap)["blocks"] == 0          # below the shortest transform of two primes
        return
    for L in (2, 5000, 16384, 40000, 60000, 70000, 90000, 90001, 1_000_003):
        for Rt in (0, 1, 240, 2400, (1 << cap) // 4):
            check_tiling(capi.ntt_plan(L, Rt, primes, max_log2=cap), L, Rt, primes, cap)
    if cap == 14:                                                  # six blocks, the last one ragged
        assert capi.ntt_plan(60000, 2400, 1, max_log2=14) == dict(blocks=6, log2_m=14, block_sites=10000)
        assert capi.ntt_plan(60001, 2400, 1, max_log2=14) == dict(blocks=6, log2_m=14, block_sites=10001)


@pytest.mark.parametrize("primes", [1, 2])
@pytest.mark.parametrize("cap", [14, 15, 16, 21])
def test_more_than_half_a_block_of_overlap_is_not_eligible(capi, primes, cap):
    quarter = (1 << cap) // 4                                      # 2 Rt = 2^cap / 2 exactly: still eligible
    if cap >= (15 if primes == 2 else 14):
        assert capi.ntt_plan(3_000_000, quarter, primes, max_log2=cap)["blocks"] >= 1
    for Rt in (quarter + 1, 2 * quarter, 5 * quarter):
        assert capi.ntt_plan(3_000_000, Rt, primes, max_log2=cap) == dict(blocks=0, log2_m=0, block_sites=0), (cap, Rt)


def test_bad_arguments_are_refused(capi):
    for args in ((1, 10, 1), ((1 << 25) + 1, 10, 1), (1000, -1, 1), (1000, 10, 0), (1000, 10, 3)):
        with pytest.raises(capi.ApsError):
            capi.ntt_plan(*args)


def test_symbols_declared_and_exported(capi):
    names = capi.header_symbols()
    lib = ctypes.CDLL(capi.LIB_PATH)
    for n in ("aps_ntt_plan", "aps_ntt_blocks"):
        assert n in names, f"{n} is not declared in include/aps.h"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in capi.load()._aps_protos
