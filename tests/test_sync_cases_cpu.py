"""CPU suite: the case table of tests/sync_cases.py is what it claims to be.  Conditions on the INPUTS of
tests/test_gpu_sync_frames.py, asserted from the oracle alone (step(want_detail=True) gives the proposal and acceptance bytes of
every step; the runs are cached in that module): a case that exercises nothing proves nothing about a frame size.  A draw that
misses a condition is drawn again with another attempt number (sync_cases.ATTEMPT); no condition is relaxed for it.  The
conditions on binding, unbinding and exits bind a draw only where it has anchors with those rates positive, and the first attempt
that passes is rarely one of those: four of the 24 draws have anchors, one has k_exit > 0.  What the table guarantees about
anchors is therefore asserted on the named edges (anchors_exits_*, k1_bound_unbind_*, k1_exits_*), class by class."""
import collections
import zlib

import numpy as np
import pytest

import sync_cases as X
from oracle import sync_oracle as so

DRAWS, EDGES = X.draws(), X.edges()
TABLE_DIGEST = 2500655676    # the draws and edges are part of the file: another seed, range or order shows here and is a reviewed change


def _ids(c):
    return c["tag"]


def check_draw(case, rs):
    """The conditions every random draw meets at frame height rs."""
    r = X.oracle_run(case, rs)
    inst, st, kw = r["inst"], r["stats"], case["kw"]
    tag = (case["tag"], rs)
    p = st["proposed"]
    assert r["moved"] > 0, (tag, "nobody moved")
    assert p[X.EV_LEFT] > 0 and p[X.EV_RIGHT] + p[X.EV_FWD] > 0 and p[X.EV_FLIP] > 0, (tag, "proposals", p.tolist())
    if inst["N"] > 1 and kw["rate_diffusion"] > 0.0:
        assert st["refused"] > 0, (tag, "no hop was refused")
    if kw.get("anchor_positions") and kw["k_on"] > 0.0 and kw["k_off"] > 0.0:
        assert st["bound"] > 0 and st["unbound"] > 0, (tag, "binds, unbinds", st["bound"], st["unbound"])
    if kw.get("k_exit", 0.0) > 0.0:
        assert st["left_system"] > 0 and len(r["exits"]) == st["left_system"], (tag, "exits", st["left_system"])
    if r["n_tiles"] >= 3:
        assert st["cross_left"] > 0 and st["cross_right"] > 0, (tag, "tile boundary crossings", st["cross_left"], st["cross_right"])
        if not inst["periodic"]:
            assert st["near_left_wall"] > 0 and st["near_right_wall"] > 0, (tag, "deposits in reach of the walls", st["near_left_wall"], st["near_right_wall"])


def test_geometry_helpers_restate_the_library():
    assert [X.own(rs) for rs in X.RS_ALL] == [60, 124, 188, 252, 316, 380, 444, 508]
    assert X.tile_sites(60 * 6 + 2, 1) == 59 and X.tile_sites(60 * 7 + 5, 1) == 60      # (LOOP_CASES of tests/test_gpu_resident_loop.py)
    assert X.tile_sites(508 + 1, 8) == 506 and X.tile_sites(508 + 3, 8) == 508 and X.tile_sites(2, 1) == 60
    for rs in X.RS_ALL:
        for L in range(1, 5 * X.own(rs)):
            o = X.tile_sites(L, rs)
            last = L - (X.n_tiles(L, rs) - 1) * o
            assert 32 * rs <= o <= X.own(rs) and (last >= 3 or X.n_tiles(L, rs) == 1 or o == 32 * rs), (L, rs, o)


def test_the_table_is_complete():
    """No class and no RS without a case, no path without the cases the GPU test counts on: a later edit cannot drop a frame."""
    tags = [c["tag"] for c in X.all_cases() + X.site_range_cases() + X.window_cases()]
    assert len(set(tags)) == len(tags)
    table = collections.defaultdict(list)
    for c in X.all_cases():
        for rs in X.RS_ALL:
            table[(c["cls"], rs)].append(c)
    assert set(table) == {(cls, rs) for cls in X.CLASSES for rs in X.RS_ALL}
    for (cls, rs), cases in sorted(table.items()):
        assert sum(X.is_draw(c) for c in cases) == X.DRAWS_PER_CLASS >= 3, (cls, rs)
        assert sum(not X.is_draw(c) for c in cases) >= 2, (cls, rs)
        # the resident loop: every (class, RS) the rules admit has draws that are eligible, the others have none
        verdicts = [X.loop4_verdict(c, rs)[0] for c in cases if X.is_draw(c)]
        no_kernel = cls[2] == "f64" and (rs == 8 or (rs == 7 and cls[1] == "kn"))
        assert any(verdicts) != no_kernel and (not no_kernel or not any(verdicts)), (cls, rs, verdicts)
        if cls[1:] == ("k1", "f64") and rs >= 5:
            assert sum(X.loop8_admits(c, rs) for c in cases) >= 3, (cls, rs)
        if cls[2] == "f64" and rs >= 2:
            assert all(X.lattice_admits(c, rs) for c in cases)
    # anchors: the draws carry them where the redraws left them (few do), so the table's anchor coverage is the named edges' --
    # every kn class one with all three anchor rates positive and `immobilize` on, every k1 class one with particles bound from the
    # start that unbind and one (k1_exits_*, one per boundary condition) whose particles leave
    for cls in X.CLASSES:
        mine = [c for c in EDGES if c["cls"] == cls and c["kw"].get("anchor_positions")]
        if cls[1] == "kn":
            assert any(min(c["kw"]["k_on"], c["kw"]["k_off"], c["kw"]["k_exit"]) > 0.0 and c["kw"].get("immobilize_when_anchored", True) for c in mine), cls
        else:
            assert any(c["bound"] != "none" and c["kw"]["k_off"] > 0.0 and c["kw"]["k_exit"] == 0.0 for c in mine), cls
    assert {c["cls"][0] for c in EDGES if c["tag"].startswith("k1_exits")} == set(X.BCS)
    assert sorted(c["cls"][:2] for c in X.ensemble_cases()) == sorted((b, k) for b in X.BCS for k in X.KCS)
    assert sorted((c["cls"], c["K"]) for c in X.window_cases()) == sorted(((b, "k1" if K == 1 else "kn", f), K) for b in X.BCS for K in (1, 3) for f in X.FIELDS)
    assert [c["cls"][0] for c in X.site_range_cases()] == list(X.BCS) and all(c["K"] == 2 for c in X.site_range_cases())
    # the widths of the tables, across the draws, at RS 8: below one tile and above two
    for cls in X.CLASSES:
        reach = [len(X.oracle_run(c, 8)["table"]) - 1 for c in DRAWS if c["cls"] == cls]
        assert min(reach) < X.own(8), (cls, reach)
        assert max(reach) > 2 * X.own(8), (cls, reach)
    digest = zlib.crc32(repr([sorted((k, repr(v)) for k, v in c.items()) for c in X.all_cases()]).encode())
    print("digest of the case table", digest)
    assert digest == TABLE_DIGEST


@pytest.mark.parametrize("rs", X.RS_ALL)
@pytest.mark.parametrize("case", DRAWS, ids=_ids)
def test_draw_exercises_its_frame(case, rs):
    inst = X.instance(case, rs)
    whole = 6 if case["L"][0] == 6 else 3                     # three tiles (six on the long ring of the wide torus draws) and a ragged last one of five sites
    assert (whole == 6) == (case["cls"][0] == "torus" and case["tag"].endswith("_1"))
    assert inst["L"] == whole * X.own(rs) + 5 and X.n_tiles(inst["L"], rs) == whole + 1 and X.tile_sites(inst["L"], rs) == X.own(rs)
    assert 1 <= inst["N"] <= inst["L"] * inst["K"] and np.bincount(inst["pos"], minlength=inst["L"]).max() <= inst["K"]
    if case["dead"]:
        assert (inst["alive"] == 0).any() or inst["N"] < 8
    if case["bound"] == "random":
        assert inst["bound"].any() or inst["N"] < 8
    check_draw(case, rs)


@pytest.mark.parametrize("rs", X.RS_ALL)
@pytest.mark.parametrize("case", EDGES, ids=_ids)
def test_edge_is_what_its_name_says(case, rs):
    r = X.oracle_run(case, rs)
    inst, st, tag = r["inst"], r["stats"], case["tag"]
    L, K, o = inst["L"], inst["K"], r["tile_sites"]
    last = L - (r["n_tiles"] - 1) * o
    reach = len(r["table"]) - 1
    if tag.startswith("single_tile"):
        assert r["n_tiles"] == 1 and L == X.own(rs) - 7
    elif tag.startswith("last_tile_of_three"):
        assert r["n_tiles"] == 2 and last == 3 and o == X.own(rs)
    elif tag.startswith("two_tiles_torus"):
        assert r["n_tiles"] == 2 and last == o == X.own(rs) and inst["periodic"]
    else:
        assert r["n_tiles"] == 4 and last in (5, 6)
    if tag.startswith("image_list"):                          # loop_prepare's own condition for the instance with the image list
        assert not inst["periodic"] and not (2 * reach + 64 * rs + o + 4 < L)
    if tag.startswith("ring_wide"):
        assert inst["periodic"] and reach == L // 2
        assert "even" not in tag or L % 2 == 0
        assert "odd" not in tag or L % 2 == 1
    if tag.startswith("full_") or tag.startswith("all_plus_full"):
        hops = st["proposed"][[X.EV_LEFT, X.EV_RIGHT, X.EV_FWD]].sum()
        assert inst["N"] == L * K and r["moved"] == 0 and st["flipped"] > 0
        assert hops == 0 or st["refused"] == hops                # a full site offers no hop; one that is proposed is refused
        for s in r["snaps"]:
            assert np.array_equal(s.field_sites()[0] + s.field_sites()[1], np.full(L, K))
    if tag.startswith("all_plus_full"):
        assert (inst["spin"] == 1).all()
        start = X.make_oracle(inst)
        start.field_sites()
        S, W = start.last_site_sums
        assert np.array_equal(S, W) and W.max() > 0
        if inst["fp32"]:                                      # every site full, every spin +1: no state gives a larger sum, and the 32-bit grid
            top = W.max() * 2.0 ** r["q"]                      # (sum_bits = 29: the table's q comes from a bound on this very sum) holds it
            assert top == np.rint(top) and K * 2.0 ** r["q"] <= top < 2.0 ** 29, (tag, rs, top)
    if tag.startswith("one_particle"):
        assert inst["N"] == 1 and r["moved"] == 1
    if tag.startswith("dense"):
        n = st["max_class_deposits"]
        print(tag, "rs", rs, "most deposits of one class in one tile and step:", n)
        if rs >= 5:
            assert n > 128, f"{tag}: {n} deposits of one class in the busiest tile at RS {rs}"
    if tag.startswith("global_field"):
        assert inst["par"].sigma_kernel == 0 and r["moved"] > 0
    if tag.startswith("flip_table"):
        plain = X.oracle_run(case, rs, flip_table=False)
        a, b = r["snaps"][-1], plain["snaps"][-1]
        assert not (np.array_equal(a.pos, b.pos) and np.array_equal(a.spin, b.spin)), tag
    if tag.startswith("half_full"):
        n = st["max_class_deposits"]
        print(tag, "rs", rs, "most deposits of one class in reach of one tile in one step:", n)
        if rs >= 2:
            assert n > 1040, f"{tag}: {n} deposits of one class in reach of the busiest tile at RS {rs}"
    if tag.startswith("anchors_exits"):                       # binds, unbinds and leaves, in every call long enough for the loop
        kw = case["kw"]
        assert K > 1 and min(kw["k_on"], kw["k_off"], kw["k_exit"]) > 0.0 and kw.get("immobilize_when_anchored", True)
        assert st["bound"] > 0 and st["unbound"] > 0 and st["left_system"] >= 10 and len(r["exits"]) == st["left_system"], (tag, rs, st)
        steps, t = np.cumsum((0,) + X.CALLS), r["exits"][:, 0] / inst["dt"]
        for n, lo, hi in zip(X.CALLS, steps[:-1], steps[1:]):
            if n >= 33:
                assert ((t > lo - 0.5) & (t < hi - 0.5)).any(), (tag, rs, "no exit in the call of", n)
        assert X.loop4_verdict(case, rs)[0] == (not (inst["fp32"] is False and (rs == 8 or rs == 7)))
    if tag.startswith("k1_bound_unbind"):
        assert K == 1 and inst["bound"].any() and st["unbound"] > 0 and st["bound"] == 0 and st["left_system"] == 0, (tag, rs, st)
        assert X.loop4_verdict(case, rs)[0] == (inst["fp32"] or rs < 8)
    if tag.startswith("k1_exits"):
        assert K == 1 and inst["bound"].any() and st["left_system"] > 0 and not X.loop4_verdict(case, rs)[0]
    if not (tag.startswith("full_") or tag.startswith("all_plus_full")):
        assert r["moved"] > 0, tag


@pytest.mark.parametrize("case", X.window_cases(), ids=_ids)
def test_windowed_table_cases_lie_beyond_lds(case):
    """The tables are the smallest beyond LDS: more than 160 KB at the field's word size whatever the frame."""
    inst = X.instance(case, 1)
    L, fp32 = inst["L"], inst["fp32"]
    tab, q = so.build_table(inst["par"].sigma_grid, L, inst["K"], inst["periodic"], 29 if fp32 else 51)
    assert all(X.lattice_sites(case, rs) == L for rs in X.RS_ALL) and inst["N"] == 3000
    if inst["periodic"]:
        assert len(tab) == L // 2 + 1
    else:
        if inst["K"] == 1 or not fp32:                        # (the 32-bit grid is coarser with three cells per site: a shorter table)
            assert len(tab) == (48001 if fp32 else 24001) and (q == 12 or not fp32)
    assert len(tab) * (4 if fp32 else 8) > 160 * 1024


@pytest.mark.parametrize("rs", X.SITE_RANGE_RS)
@pytest.mark.parametrize("case", X.site_range_cases(), ids=_ids)
def test_site_range_cases_have_room_for_three_ranks(case, rs):
    r = X.oracle_run(case, rs)
    o, last = r["tile_sites"], r["inst"]["L"] % r["tile_sites"]
    assert last == 7 < len(r["table"])                        # a ragged last tile, shorter than the table
    # tiles beyond a tile with a site in reach of its frame (tlen + 2 sites): across the seam of a ring the last tile counts for `last` sites only
    reach_tiles = (len(r["table"]) + 2 + (o - last if r["inst"]["periodic"] else 0) + o - 1) // o
    assert reach_tiles == (2 if r["inst"]["periodic"] else 1) and r["n_tiles"] >= 4 * 3 * reach_tiles
    assert case["K"] == 2 and r["stats"]["left_system"] > 10 and r["stats"]["cross_left"] > 0 and r["stats"]["cross_right"] > 0
