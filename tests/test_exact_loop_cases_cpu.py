"""CPU suite: the parameter sets of tests/exact_loop_cases.py are what they claim to be.  Every case runs through the oracle
alone (cached in that module, shared with nothing on this machine's side but these tests): the runs are long enough, the named
edges do what their names say, no draw of any case lies within MARGIN_FLOOR of a threshold it is compared with (a condition
on the INPUTS of the GPU parity test, asserted for every case, none skipped), the features the list was written for occur
often enough, and `table_callable` is the piecewise-linear reading of a flip table that channels() makes."""
import collections
import zlib

import numpy as np
import pytest

import exact_loop_cases as X

CASES = X.all_cases()
# fewer than 200 events by construction: the lone particle of random_30 sits on an anchor site, binds and leaves for good
LOW_ACTIVITY = {"random_30_half"}
RANDOM_DIGEST = 2854591485
FULL = [c for c in CASES if c["N"] == c["kw"]["L"] * c["kw"]["site_capacity"]]


def test_the_list_is_the_reviewed_one():
    tags = [c["tag"] for c in CASES]
    assert len(set(tags)) == len(tags) and len(X.hand_cases()) == 22 and len(X.random_cases()) == 32
    # the draw is part of the file: another seed, range or order of draws shows here and is a reviewed change
    digest = zlib.crc32(repr([sorted((k, repr(v)) for k, v in c.items()) for c in X.random_cases()]).encode())
    print("digest of the random cases", digest)
    assert digest == RANDOM_DIGEST
    Ls = [c["kw"]["L"] for c in X.random_cases()]
    assert min(Ls) >= 2 and max(Ls) <= 400 and all(1 <= c["N"] <= c["kw"]["L"] * c["kw"]["site_capacity"] for c in CASES)
    assert {c["N"] for c in X.hand_cases()} >= {1, 64, 65, 1024, 1025}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["tag"])
def test_case_is_valid_and_keeps_its_margins(case):
    r, p = X.oracle_run(case), X.prepared(case)
    print(case["tag"], "events", r["ev"], "recorded", len(r["snaps"]), "margins", r["margin"])
    assert r["ev"] <= 1500 and r["ev"] < X.N_ROWS                  # the run ended on T or on its last observation, not on the table
    if case["tag"] not in LOW_ACTIVITY:
        assert r["ev"] >= 200, (case["tag"], r["ev"])
    assert len(r["snaps"]) >= 2 and len(r["snaps"]) == len(r["live"]) == len(r["events"])
    assert min(r["margin"].values()) >= X.MARGIN_FLOOR, (case["tag"], r["margin"])
    assert np.isfinite(r["margin"]["particle"]) and np.isfinite(r["margin"]["channel"]) and np.isfinite(r["margin"]["time"])
    K, L = case["kw"]["site_capacity"], case["kw"]["L"]
    for pos, sigma, bound in r["snaps"]:                           # every recorded state is a state of the model
        assert pos.size == sigma.size == bound.size and np.all(np.abs(sigma) == 1)
        assert pos.size == 0 or (pos.min() >= 0 and pos.max() < L and np.bincount(pos, minlength=L).max() <= K)
    if case["table"] is not None:
        assert p["flip_table"].shape == (2, case["table"][1] + 1) and np.all(p["flip_table"] > 0.3)


def test_all_leave_ends_empty_with_one_exit_per_particle():
    case = X.by_tag("all_leave")
    r = X.oracle_run(case)
    assert r["frozen"] and r["n_left"] == 0 and np.isinf(r["t"])
    assert len(r["exits"][0]) == case["N"] == len(r["exits"][1]) and r["live"][-1] < case["N"]
    assert np.all(np.diff(r["exits"][0]) >= 0) and np.all(X.prepared(case)["orc"].par.is_anchor_site[np.array(r["exits"][1])])
    assert 2 <= len(r["snaps"]) < X.N_OBS                          # observations before it emptied, none after


@pytest.mark.parametrize("case", FULL, ids=lambda c: c["tag"])
def test_full_lattices_fire_flips_only(case):
    r, p = X.oracle_run(case), X.prepared(case)
    flipped = 0
    for (pos, sigma, _), (_, before, _) in zip(r["snaps"][1:], r["snaps"]):
        assert np.array_equal(pos, p["pos0"])                      # nobody moved, nobody left
        flipped += int(np.any(sigma != before))
    assert len(r["exits"][0]) == 0 and r["n_left"] == case["N"]
    assert flipped >= 1 and np.isinf(r["margin"]["side"])          # no hop ever chose a direction


def test_fully_polarised_starts_read_the_last_cell_of_the_table():
    """m = +1 (-1) exactly at the first event, with the local and with the global field: channels() clamps i to flip_n - 1 (0)."""
    seen = set()
    for tag in ("all_plus_table_local", "all_plus_table_global", "all_minus_table_global"):
        p = X.prepared(X.by_tag(tag))
        orc, L = p["orc"], p["orc"].par.L
        cp, cm = np.bincount(p["pos0"][p["sigma0"] == 1], minlength=L), np.bincount(p["pos0"][p["sigma0"] == -1], minlength=L)
        m = orc.mean_field(cp, cm)[p["pos0"]]
        assert np.all(np.abs(m) == 1.0) and len(set(m.tolist())) == 1
        tab, n = p["flip_table"], p["flip_table"].shape[1] - 1
        got = orc.flip_rate_fn(p["sigma0"], m)
        assert np.array_equal(got, np.full(len(m), tab[0 if p["sigma0"][0] > 0 else 1, n if m[0] > 0 else 0]))
        seen.add((float(m[0]), orc.par.sigma_kernel > 0))
    assert seen == {(1.0, True), (1.0, False), (-1.0, False)}


def test_census():
    count = collections.Counter()
    for c in CASES:
        count.update(X.features(c))
    print(sorted(count.items()))
    wanted = ["ring", "walls", "field_global", "field_narrow", "field_half", "field_over", "K=1", "K=2", "K=3", "K=4", "K=5", "K>3", "L<=3",
              "one_particle", "full", "beta=0", "rate_diffusion=0", "rate_active=0", "k_on=0", "k_off=0", "k_exit=0", "anchors",
              "anchor_at_0", "anchor_at_L-1", "bound0", "bound0_plus", "bound0_off_anchor", "table", "polarised", "flip_n=1", "flip_n=8",
              "flip_n=64", "flip_n=65536"]
    short = {k: count[k] for k in wanted if count[k] < 3}
    assert not short, short
    assert count["four_wavefronts"] >= 1                            # the other cases reach that kernel through n_cap = 1030
    for flag in X.FLAGS:
        for value in (False, True):
            mine = [c for c in CASES if c["kw"][flag] is value]
            assert len(mine) >= 3, (flag, value)
            assert any(c["table"] is not None for c in mine), (flag, value, "with a table")
    # the flags matter only where something can bind: each value also among the cases with anchors and a binding rate
    for flag in ("minus_anchor", "immobilize_when_anchored", "suppress_flip_when_bound"):
        for value in (False, True):
            assert any(c["kw"][flag] is value and "anchors" in X.features(c) and c["kw"]["k_on"] > 0 for c in CASES), (flag, value)
    exits = sum(len(X.oracle_run(c)["exits"][0]) > 0 for c in CASES)
    assert exits >= 3, exits


@pytest.mark.parametrize("shape", sorted(X.FLIP_SHAPES))
@pytest.mark.parametrize("n", [1, 8, 64, 65536])
def test_table_callable_is_the_piecewise_linear_reading(shape, n):
    fn, d2 = X.FLIP_SHAPES[shape]
    tab = X.flip_table(shape, n)
    read = X.table_callable(tab)
    m = np.concatenate([np.linspace(-1.0, 1.0, 20001), -1.0 + 2.0 * np.arange(n + 1)[:: max(1, n // 64)] / n])
    for spin, row in ((1, 0), (-1, 1)):
        s = np.full(m.size, spin, np.int8)
        err = np.max(np.abs(read(s, m) - fn(s, m)))
        bound = d2 * (2.0 / n) ** 2 / 8.0                           # linear interpolation over cells of width 2 / n
        print(shape, n, spin, "error", err, "bound", bound)
        assert err <= bound + 2e-15, (shape, n, spin, err, bound)   # a few roundings of numbers below 2
        ends = read(np.array([spin, spin]), np.array([-1.0, 1.0]))
        # m = -1: f = 0, the first entry exactly.  m = +1: the clamp, f = 1 and a + 1 (b - a), which IS b whenever b - a is exact
        # (a / 2 <= b <= 2 a, Sterbenz) -- every table here but the two-entry tanh one, whose last cell spans 1.69 .. 0.31: there the
        # device's own arithmetic is one ulp of 1.69 off the entry, and the reading must be that arithmetic, not the entry
        a_, b_ = tab[row, n - 1], tab[row, n]
        assert ends[0] == tab[row, 0] and ends[1] == a_ + (b_ - a_) and abs(ends[1] - b_) <= np.spacing(max(a_, b_))
        if 0.5 * a_ <= b_ <= 2.0 * a_:
            assert ends[1] == b_
        else:
            assert (shape, n) == ("tanh", 1)
    if n == 8:                                                      # coarse enough that the reading is visibly not the function
        assert np.max(np.abs(read(np.ones(m.size), m) - fn(np.ones(m.size), m))) > 1e-3
