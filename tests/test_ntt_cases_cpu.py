"""CPU suite: the case list of tests/ntt_cases.py is what it claims to be -- a census, without a GPU, of the transform every case
runs (reach from so.build_table, plan from capi.ntt_plan, ntt_setup's eligibility rules restated in ntt_cases.eligible) -- and
`scatter_field`, the N x taps reference for {W, S, occupancy} on all sites, equals the oracle's own field_sites() on all sites of
small lattices and the window stencil of tests/test_gpu_parity.py on a large one."""
import collections
import importlib
import os
import time

import numpy as np
import pytest

import ntt_cases as X
from oracle import sync_oracle as so
from test_gpu_parity import _oracle_window_field

PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"
CASES = X.all_cases()
TAKEN = [c for c in CASES if c["log2_m"] is not None]


@pytest.fixture(scope="module")
def capi():
    return importlib.import_module(PKG + ".capi")                  # ntt_plan needs the library, not a device


def plan(capi, case):
    return capi.ntt_plan(case["L"], X.reach(case), X.primes(case))


def test_the_list_is_the_reviewed_one():
    tags = [c["tag"] for c in CASES]
    assert len(set(tags)) == len(tags) == 21 and len(X.runs()) == 38, (len(tags), len(X.runs()))
    for c in CASES:
        assert c["blocks"] == (X.LARGE_BLOCKS if (c["log2_m"] or 0) >= 19 else X.SMALL_BLOCKS), c["tag"]
        assert 1 <= c["K"] <= 2 and c["N"] <= c["K"] * c["L"] and set(c["fused"]) <= {"0", "1"} and len(c["betas"]) in (1, 2)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["tag"])
def test_case_runs_the_transform_it_names(capi, case):
    L, Rt = case["L"], X.reach(case)
    edge = case["tag"].startswith(("walls_m17_edge_reach", "walls_edge_reach_plus_one"))
    ok, why = X.eligible(case, *((X.EDGE_FRAME, X.EDGE_OWN) if edge else ()))
    p = plan(capi, case)
    print(case["tag"], "L", L, "reach", Rt, "L + 2 reach", L + 2 * Rt, "plan", p, "eligible", ok, why)
    if case["log2_m"] is None:
        assert not ok and why.startswith("walls"), why
        return
    assert ok, why
    m = case["log2_m"]
    assert p == dict(blocks=1, log2_m=m, block_sites=L), p
    assert (1 << m) >= L + 2 * Rt and (m == (14 if case["fp32"] else 15) or (1 << (m - 1)) < L + 2 * Rt)
    assert min(14 if case["fp32"] else 15, m) <= m <= 21
    for f in case["fused"]:
        assert X.expected_launches(m, f) == (3 if m == 14 or f == "1" else 5)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["tag"])
def test_particles_sit_where_the_convolution_can_go_wrong(case):
    L, K, Rt = case["L"], case["K"], X.reach(case)
    for e in range(len(case["betas"])):
        pos, spin = X.initial_state(case, e)
        assert len(pos) == len(spin) == case["N"] and pos.dtype == np.int32 and set(np.unique(spin)) == {-1, 1}
        occ = np.bincount(pos, minlength=L)
        assert len(occ) == L and occ.max() <= K and occ[0] >= 1 and occ[L - 1] >= 1
        near = min(Rt, L // 4)
        # within the reach of both walls (torus: on both sides of the seam), more than the end sites alone; and the interior
        assert (pos < near).sum() >= 20 and (pos >= L - near).sum() >= 20
        assert ((pos >= Rt) & (pos < L - Rt)).sum() >= 20 or 2 * Rt >= L - 2 * X.TILE_TERMS_MAX
        assert ((pos > L // 4) & (pos < 3 * L // 4)).sum() >= 100
    if len(case["betas"]) > 1:
        assert not np.array_equal(X.initial_state(case, 0)[0], X.initial_state(case, 1)[0])


def test_census(capi):
    count = collections.Counter()
    for c in TAKEN:
        for f in c["fused"]:
            count[("i32" if c["fp32"] else "f64", c["log2_m"], X.expected_launches(c["log2_m"], f), "fused" if f == "1" else "unfused")] += 1
    print(sorted(count.items()))
    # one block at EVERY size: 14 .. 21 with one prime, 15 .. 21 with two; from 15 on in three launches (ntt_mid) and in five
    assert count[("i32", 14, 3, "fused")] >= 1
    for width, sizes in (("i32", range(15, 22)), ("f64", range(15, 22))):
        for m in sizes:
            assert count[(width, m, 3, "fused")] >= 1 and count[(width, m, 5, "unfused")] >= 1, (width, m)
    assert not any(k[0] == "f64" and k[1] < 15 for k in count)
    # the radices of the i2 sweeps: a2 = m - 14 = 0 .. 7 (one prime), 1 .. 7 (two)
    assert {c["log2_m"] - 14 for c in TAKEN if c["fp32"]} == set(range(8)) and {c["log2_m"] - 14 for c in TAKEN if not c["fp32"]} == set(range(1, 8))
    for periodic in (False, True):
        for fp32 in (True, False):
            assert len({c["log2_m"] for c in TAKEN if c["periodic"] == periodic and c["fp32"] == fp32}) >= 3, (periodic, fp32)
    assert all(plan(capi, c)["blocks"] == 1 for c in TAKEN)
    assert any(c["K"] == 1 for c in TAKEN) and any(c["K"] == 2 for c in TAKEN)


@pytest.mark.parametrize("fp32", [True, False], ids=["i32", "f64"])
def test_exact_fit_and_its_neighbour(capi, fp32):
    w = "_i32" if fp32 else "_f64"
    fit, past = X.by_tag("walls_m15_exact_fit" + w), X.by_tag("walls_m16_one_past_fit" + w)
    assert X.search_exact_fit(15, fp32, sigma=fit["sigma"], K=fit["K"]) == fit["L"]          # found by search: the reach depends on L
    assert fit["L"] + 2 * X.reach(fit) == 1 << 15 and plan(capi, fit)["log2_m"] == 15
    assert past["L"] == fit["L"] + 1 and past["L"] + 2 * X.reach(past) == (1 << 15) + 1 and plan(capi, past)["log2_m"] == 16
    assert (past["sigma"], past["K"], past["N"]) == (fit["sigma"], fit["K"], fit["N"])


@pytest.mark.parametrize("fp32", [True, False], ids=["i32", "f64"])
def test_ring_wide_tables_on_an_even_and_an_odd_ring(capi, fp32):
    w = "_i32" if fp32 else "_f64"
    even, odd = X.by_tag("torus_m17_even_ring_wide" + w), X.by_tag("torus_m18_odd_ring_wide" + w)
    assert even["L"] % 2 == 0 and 2 * X.reach(even) == even["L"] and even["L"] + 2 * X.reach(even) == 1 << 17     # the half-ring tap; and an exact fit
    assert odd["L"] % 2 == 1 and 2 * X.reach(odd) == odd["L"] - 1 and odd["L"] == even["L"] + 1
    assert plan(capi, even)["log2_m"] == 17 and plan(capi, odd)["log2_m"] == 18
    assert X.table(even)[0][-1] > 0.0                              # the half-ring tap is a weight, not a zero that could count twice unnoticed


@pytest.mark.parametrize("fp32", [True, False], ids=["i32", "f64"])
def test_edge_of_the_walls_rule(fp32):
    edge = X.by_tag("walls_m17_edge_reach" + ("_i32" if fp32 else "_f64"))
    L, Rt = edge["L"], X.reach(edge)
    tiles = X.EDGE_FRAME + X.EDGE_OWN
    assert 2 * Rt + tiles + 4 < L <= 2 * (Rt + 1) + tiles + 4      # the largest reach the rule admits
    if fp32:
        over = X.by_tag("walls_edge_reach_plus_one_sweeps_i32")
        assert over["L"] == L and X.reach(over) == Rt + 1 and over["sigma"] > edge["sigma"] and over["N"] == edge["N"]
        assert X.eligible(over, X.EDGE_FRAME, X.EDGE_OWN) == (False, "walls: 2 reach + frame + own + 4 >= L")
        # refused by the reach alone: as a ring, or with shorter tile terms, the same table would be taken
        assert 2 * X.reach(over) <= L and X.eligible(over, X.EDGE_FRAME, X.EDGE_OWN - 2)[0]


def test_two_ensembles_of_the_binary64_field():
    case = X.by_tag("walls_m15_two_ensembles_f64")
    assert not case["fp32"] and len(case["betas"]) == 2 and case["betas"][0] != case["betas"][1] and case["fused"] == X.BOTH
    ref = X.reference(case)
    assert any(len(e["snaps"][-1]["exits"]) > 0 for e in ref["ens"]) and any(e["snaps"][-1]["bound"].any() for e in ref["ens"])
    assert not np.array_equal(ref["ens"][0]["snaps"][-1]["pos"], ref["ens"][1]["snaps"][-1]["pos"])


# ---- scatter_field against the oracle

SMALL = [dict(L=700, K=1, sigma=0.03, periodic=False), dict(L=901, K=3, sigma=0.08, periodic=False), dict(L=601, K=2, sigma=0.05, periodic=True),
         dict(L=600, K=2, sigma=0.4, periodic=True), dict(L=601, K=3, sigma=0.4, periodic=True), dict(L=512, K=1, sigma=0.01, periodic=True),
         dict(L=400, K=2, sigma=0.124, periodic=False)]


@pytest.mark.parametrize("fp32", [True, False], ids=["i32", "f64"])
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "-".join(f"{k}{v}" for k, v in s.items()))
def test_scatter_field_equals_the_oracle_on_all_sites(shape, fp32):
    case = dict(shape, fp32=fp32, betas=(1.1,), extra={}, seed=3, dt=0.05)
    par = X.params(case)
    orc = so.SyncOracle(par, dt=0.05, seed=3, **(dict(sum_bits=29) if fp32 else {}))
    L, K = shape["L"], shape["K"]
    Rt = len(orc.table) - 1
    if shape["periodic"] and shape["sigma"] > 0.3:
        assert Rt == L // 2                                        # ring-wide (even: the half-ring tap)
    rng = np.random.default_rng(5)
    N = L * K // 2
    pos = np.concatenate([[0, L - 1], rng.choice(np.repeat(np.arange(1, L - 1), K), size=N - 2, replace=False)]).astype(np.int32)
    spin = rng.choice(np.array([1, -1], np.int8), size=N)
    alive = (rng.random(N) > 0.1).astype(np.uint8)                 # a particle that has left deposits nothing
    orc.set_state(pos, spin, alive=alive)
    for _ in range(2):
        cp, cm, _m = orc.field_sites()
        S0, W0 = orc.last_site_sums
        W, S, occ = X.scatter_field(orc.table, orc.pos, orc.spin, orc.alive, L, shape["periodic"])
        assert np.array_equal(occ, cp + cm) and np.array_equal(W, W0) and np.array_equal(S, S0)
        assert W.max() > 0 and np.abs(S).max() > 0
        orc.run(3)


def test_scatter_field_equals_the_window_stencil_on_a_large_case():
    case = X.by_tag("walls_m19_i32")
    tab, _ = X.table(case)
    pos, spin = X.initial_state(case)
    L, Rt = case["L"], X.reach(case)
    W, S, occ = X.scatter_field(tab, pos, spin, np.ones(len(pos), np.uint8), L, False)
    assert np.array_equal(occ, np.bincount(pos, minlength=L))
    for a, b in ((0, 600), (Rt - 300, Rt + 300), (L // 2 - 300, L // 2 + 300), (L - Rt - 300, L - Rt + 300), (L - 600, L)):
        W0, S0 = _oracle_window_field(tab, pos.astype(np.int64), spin, L, a, b)
        assert np.array_equal(W[a:b], W0) and np.array_equal(S[a:b], S0), a


def test_reference_costs_a_few_seconds_per_case_and_moves_particles():
    """The oracle's trajectory and the scatter of a case, as the device test will use them (cached there as here).  Prints the
    seconds per case (the docstring of ntt_cases records one such run); asserts what the device test relies on.  APS_NTT_ALL_REFERENCES=1
    includes the cases of m >= 19 (4 to 5 s each), which otherwise only the device test computes."""
    for case in CASES if os.environ.get("APS_NTT_ALL_REFERENCES") == "1" else [c for c in CASES if c["blocks"] == X.SMALL_BLOCKS]:
        t0 = time.perf_counter()
        ref = X.reference(case)
        dt = time.perf_counter() - t0
        print(f'    "{case["tag"]}": {dt:.1f},')
        for e in ref["ens"]:
            assert len(e["snaps"]) == len(case["blocks"]) + 1
            first, last = e["snaps"][0], e["snaps"][-1]
            assert np.array_equal(first["pos"], e["pos"]) and first["W"].shape == (case["L"],)
            moved = (last["pos"] != e["pos"]).mean()
            assert moved > (0.4 if case["blocks"] == X.SMALL_BLOCKS else 0.05), (case["tag"], moved)
            assert not np.array_equal(first["W"], last["W"]) and not np.array_equal(first["S"], last["S"])
