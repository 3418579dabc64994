"""GPU suite (-m gpu): the device observables of the fixed-dt stepper -- aps_observe, aps_mark_reference, aps_observe_scalars,
aps_observe_scalars_all, aps_observe_structure, aps_observe_bins -- against the plain restatements of
tests/observable_reference.py, evaluated on the state aps_get_state returns (never on a call's own result).

Bars.  Every integer output is `==`: the eleven scalars, the bins, n, sum count^2, the site counts of aps_observe.  The m_field
of aps_observe is bit-equal to the oracle's field of the same state (SyncOracle.field_sites).  Floating-point sums are held to
a bound derived from the kernel's summation shape, printed beside the measured error: a sum whose terms are added along a path
of at most d additions, in any order, is within d * 2^-53 * sum |term| of the exact sum.
  structure_dft    per lane ceil(Npad / 256) additions, 6 shuffle levels, 4 atomics into LDS: d = ceil(Npad / 256) + 6 + 4;
                   terms of magnitude <= 1, each carrying 2 ulp (2^-53 below 1) of sincospi.
  structure_sites  per lane ceil(L / (256 G)) additions, 6 shuffle levels, 4 G atomics taken as serial, G the launched grid
                   min(1024, ceil(L / 256)): d = ceil(L / (256 G)) + 6 + 4 G; terms m and m * m (the reference sums the same
                   binary64 products, correctly rounded).
Measured on an MI355X (largest over the cases; the tests print every figure): Fourier sums 3.5e-13 against a bound of 7.4e-9
at N = 140 000 and 1.2e-13 against 3.7e-12 at k_max = L = 997; sum m 9.7e-13 against 3.9e-8 at L = 262 400 and 1.4e-14
against 4.6e-13 at L = 997; sum m^2 4.5e-13 against 9.5e-11; added over the ranks at L = 6000: Fourier sums 2.8e-13 against 1.9e-11, sum m 4.5e-13 against 2.2e-11.

Site-sharded handles (test_site_sharded_observables_add_up): a number is right once added over the ranks, or the call refuses
it (include/aps.h lists which).

One-line faults tried on a copy of the kernels, and the cases that failed under each (all others passed):
  count_sites without its DEAD / AWAY test .... every case that uploads dead particles (blocked, sum count^2), 15 of 20
  the two halves of cnt_pm swapped in the block-table index .... every case with a random table, 11 of 20
  observe_scalars launched with a cap of 511 workgroups and no stride .... test_scalar_sums_beyond_one_pass_of_the_grid
  k * pos without the reduction mod L .... test_fourier_modes_up_to_the_lattice_length[997], test_empty_and_minimal_systems"""
import math
import os

import numpy as np
import pytest

from oracle import sync_oracle as so

import observable_reference as R
from test_gpu_parity import _merged_state, capi, make_handle, params, random_state  # noqa: F401  (capi is a fixture)

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
ANCHORS = dict(anchor_positions=[0.25, 0.5, 0.75], anchor_radius=0.02, k_on=2.0, k_off=1.0)


def npad(n, world=1):
    """Slots per ensemble of a handle (aps_create: whole 256-slot groups per rank)."""
    return max(256, -(-(-(-n // world)) // 256) * 256) * world


def dft_bound(n_slots, n_live):
    return ((-(-n_slots // 256) + 6 + 4) * EPS + 2 * EPS) * n_live


def sites_depth(L):
    G = min(1024, -(-L // 256))
    return -(-L // (256 * G)) + 6 + 4 * G


def tables(K, seed=5):
    rnd = np.random.default_rng(seed).integers(0, 2, (K + 1, K + 1)).astype(np.uint8)
    return {"any": None, "zero": np.zeros((K + 1, K + 1), np.uint8), "random": rnd}


def dead_mask(rng, n, frac=0.15):
    alive = (rng.random(n) >= frac).astype(np.uint8)
    assert 0 < alive.sum() < n
    return alive


def oracle_field(par, state, fp32=False):
    p, s, b, a = state
    orc = so.SyncOracle(par, dt=0.05, seed=1, **(dict(sum_bits=29) if fp32 else {}))
    orc.set_state(p, s, b, (a == 1).astype(np.uint8))
    return orc.field_sites()[2]


def check_scalars(h, state, ref, L, K, e=0, which=("any", "zero", "random"), ranges=None):
    """aps_observe_scalars of ensemble e for the block tables `which` against scalar_sums; returns the references by table."""
    p, s, b, a = state
    x_wall, lo, hi = (7 * L) // 10, L // 10, L // 3
    if ranges is not None:
        lo, hi = ranges
    want = {}
    for name in which:
        tab = tables(K)[name]
        got = h.observe_scalars(ensemble=e, x_wall=x_wall, range_lo=lo, range_hi=hi, block_table=tab)
        want[name] = R.scalar_sums(p, s, a, ref[0] if ref else None, ref[1] if ref else None, L, K, x_wall, lo, hi, tab)
        assert got == want[name], (name, e, got, want[name])
    return want


def check_bins(h, state, L, nbins, e=0):
    p, s, b, a = state
    plus, minus = h.observe_bins(nbins, ensemble=e)
    wp, wm = R.bin_sums(p, s, a, L, nbins)
    assert np.array_equal(plus, wp) and np.array_equal(minus, wm), nbins
    assert int(plus.sum() + minus.sum()) == int((a == 1).sum())
    return plus, minus


def check_observe(h, par, state, e=0, fp32=False, field="oracle"):
    """aps_observe: the counts ==, the field bit-equal to the oracle's (field = "oracle"); returns the field."""
    p, s, b, a = state
    cp, cm, m = h.observe(ensemble=e)
    wp, wm = R.site_counts(p, s, a, par.L)
    assert np.array_equal(cp, wp) and np.array_equal(cm, wm)
    assert np.all(np.isfinite(m)) and np.all(np.abs(m) <= 1.0)
    if field == "oracle":
        assert np.array_equal(m, oracle_field(par, state, fp32))
    return m


def check_structure(h, state, m, L, n_slots, k_max, e=0, tag=""):
    """aps_observe_structure against structure_sums on the field m (aps_observe's, which check_observe pins to the oracle)."""
    p, s, b, a = state
    n, c2, m1, m2, F = h.observe_structure(ensemble=e, k_max=k_max)
    wn, wc2, wm1, wm2, wF = R.structure_sums(p, a, L, k_max, m)
    assert n == wn and c2 == wc2 and F.shape == (k_max, 2) and np.all(np.isfinite(F)) and math.isfinite(m1) and math.isfinite(m2)
    err_f = float(np.max(np.abs(F.astype(np.longdouble) - wF)))
    d = sites_depth(L)
    b_f, b_m1, b_m2 = dft_bound(n_slots, wn), d * EPS * math.fsum(np.abs(m)), d * EPS * wm2
    print(f"{tag} L={L} k_max={k_max} n={wn}: Fourier error {err_f:.3e} (bound {b_f:.3e}), sum m error {abs(m1 - wm1):.3e} "
          f"(bound {b_m1:.3e}), sum m^2 error {abs(m2 - wm2):.3e} (bound {b_m2:.3e})")
    assert err_f <= b_f and abs(m1 - wm1) <= b_m1 and abs(m2 - wm2) <= b_m2
    return wn, wc2, wm1, wm2, wF


def check_all(h, par, state, ref, n_cap, e=0, fp32=False, k_max=25, nbins=7, tag=""):
    want = check_scalars(h, state, ref, par.L, par.K, e)
    check_bins(h, state, par.L, nbins, e)
    m = check_observe(h, par, state, e, fp32)
    check_structure(h, state, m, par.L, npad(n_cap), k_max, e, tag)
    return want


def refused(capi, call, entry_point):
    """The call fails with APS_ERR_STATE and a text naming the entry point."""
    with pytest.raises(capi.ApsError, match=entry_point + ":") as err:
        call()
    assert err.value.code == -3, err.value


def stepped(capi, par, N, method="tiles", steps=40, seed=3, dt=0.05, mark=True, dead=0.15, **kw):
    """A handle with some particles uploaded dead and a reference marked, `steps` steps later: (handle, initial pos, alive)."""
    rng = np.random.default_rng(seed)
    pos, spin = random_state(rng, par.L, N, par.K)
    alive = dead_mask(rng, N, dead)
    h = make_handle(capi, par, N, dt=dt, seed=seed, method=method, **kw)
    try:
        h.set_state(pos, spin, alive=alive)
        if mark:
            h.mark_reference()
        h.step(steps)
    except Exception:
        h.close()
        raise
    return h, pos, alive


@pytest.mark.parametrize("method", ["pairs", "lattice", "tiles"])
def test_every_entry_point_in_the_three_formulations(capi, method):
    """L = 997, K = 3, walls, anchors with exits: particles uploaded dead, more dying after the mark."""
    par = params(L=997, K=3, sigma=0.02, k_exit=1.5, **ANCHORS)
    h, pos, alive = stepped(capi, par, 2000, method)
    try:
        h.resort()                                            # (the reference follows the particles into the new slot order)
        state = h.get_state()
        want = check_all(h, par, state, (pos, alive), 2000, tag=method)["any"]
        died = int(((alive == 1) & (state[3] == 0)).sum())
        assert died > 0 and want["n_d"] == int(alive.sum()) - died and 0 < want["blocked"] < want["attempts"]
        assert want["sum_d"] != 0 and want["n_wall"] > 0 and want["n_range"] > 0
    finally:
        h.close()


def test_torus_displacements_are_not_unwrapped(capi):
    par = params(L=1000, K=2, sigma=0.02, periodic=True, rate_diffusion=5.0, rate_active=2.0)
    h, pos, alive = stepped(capi, par, 1500, dt=0.04)
    try:
        state = h.get_state()
        want = check_all(h, par, state, (pos, alive), 1500, tag="torus")["any"]
        wrapped = np.abs(state[0].astype(np.int64) - pos)[(alive == 1) & (state[3] == 1)] > par.L // 2
        assert wrapped.sum() >= 1 and want["sum_d2"] >= int(wrapped.sum()) * (par.L // 2) ** 2
    finally:
        h.close()


def test_32bit_field(capi):
    par = params(L=3000, K=1, sigma=0.02)
    h, pos, alive = stepped(capi, par, 2000, fp32=True)
    try:
        state = h.get_state()
        check_all(h, par, state, (pos, alive), 2000, fp32=True, tag="i32")
        assert not np.array_equal(state[0], pos)
        assert not np.array_equal(oracle_field(par, state), oracle_field(par, state, fp32=True))     # the coarser grid is another field
    finally:
        h.close()


def test_ensembles_and_observe_scalars_all(capi):
    """Three betas in one handle; only ensemble 1 gets a reference; each ensemble its own range, one of them empty."""
    par = params(L=997, K=2, sigma=0.02)
    N, L, K = 1200, par.L, par.K
    rng = np.random.default_rng(12)
    h = make_handle(capi, par, N, seed=6, method="tiles", beta=[0.3, 1.1, 2.4])
    try:
        first = []
        for e in range(3):
            pos, spin = random_state(rng, L, N - 100 * e, K)
            alive = dead_mask(rng, len(pos))
            h.set_state(pos, spin, alive=alive, ensemble=e)
            first.append((pos, alive))
        h.mark_reference(ensemble=1)
        h.step(30)
        ranges = [(L // 10, L // 3), (0, -1), (5, L - 1)]
        rows = {name: h.observe_scalars_all(x_wall=(7 * L) // 10, ranges=ranges, block_table=tab) for name, tab in tables(K).items()}
        for e in range(3):
            state = h.get_state(ensemble=e)
            assert len(state[0]) == N - 100 * e and not np.array_equal(state[0], first[e][0])
            want = check_scalars(h, state, first[e] if e == 1 else None, L, K, e, ranges=ranges[e])
            for name in want:
                assert rows[name][e] == want[name], (name, e)
            assert (want["any"]["n_d"] > 0) == (e == 1) and (want["any"]["n_range"] > 0) == (e != 1)
            check_bins(h, state, L, 7, e)
            m = check_observe(h, par, state, e)
            check_structure(h, state, m, L, npad(N), 25, e, tag=f"ensemble {e}")
        assert len({rows["any"][e]["sum_pos"] for e in range(3)}) == 3
    finally:
        h.close()


def test_after_the_resident_loop(capi):
    """sync_slots after a call that ran inside the resident loop, after a per-step call, and after an odd / even buffer swap."""
    par = params(L=3000, K=1, sigma=0.01)
    os.environ["APS_LOOP_MIN"] = "3"
    try:
        h, pos, alive = stepped(capi, par, 1500, steps=7)
        try:
            for n in (0, 2, 33):
                if n:
                    h.step(n)
                taken, loop_state, why = h.loop_info()
                assert loop_state == 1 and taken == (0 if n == 2 else n or 7), (n, taken, why)
                state = h.get_state()
                check_all(h, par, state, (pos, alive), 1500, tag=f"loop +{n}")
            assert h.time()[1] == 42 and not np.array_equal(state[0], pos)
        finally:
            h.close()
    finally:
        del os.environ["APS_LOOP_MIN"]


def test_scalar_sums_beyond_one_pass_of_the_grid(capi):
    """N = 140 000 on L = 150 000: 547 groups of 256 slots against a grid capped at 512 workgroups, so the first 35 workgroups
    of observe_scalars take a second turn of their loop.  Only 2 % are uploaded dead: wherever the library puts its dead and
    padding slots, more particles are alive than one pass of the grid reads (asserted), so a pass alone must lose some."""
    N = 140000
    par = params(L=150000, K=1, sigma=0.002)
    assert npad(N) // 256 > 512
    h, pos, alive = stepped(capi, par, N, steps=5, dead=0.02)
    try:
        state = h.get_state()
        want = check_all(h, par, state, (pos, alive), N, k_max=2, tag="scalar stride")["any"]
        assert want["n"] == int(alive.sum()) > 512 * 256       # (nobody leaves)
        assert want["sum_d2"] > 0 and 0 < want["blocked"] < want["attempts"]
    finally:
        h.close()


def test_site_sums_beyond_one_pass_of_the_grid(capi):
    """L = 262 400: 1025 groups of 256 sites against a grid capped at 1024 workgroups, so workgroup 0 of structure_sites takes a
    second turn of its loop, over the last 256 sites.  The oracle's field is slow at this length, so only the REDUCTION is held
    here: the sums over sites against math.fsum of the m_field aps_observe returns (the field itself is pinned to the oracle at
    the small shapes above).  Everything integer is exact as everywhere."""
    L, N, tail = 262400, 3000, 40
    par = params(L=L, K=1, sigma=5.0 / L)
    rng = np.random.default_rng(21)
    pos = np.concatenate([rng.choice(262144, N - tail, replace=False), 262144 + rng.choice(256, tail, replace=False)]).astype(np.int32)
    spin = rng.choice(np.array([1, -1], np.int8), size=N)
    spin[-tail:] = np.where(np.arange(tail) % 4 == 0, -1, 1)  # (a tail that is magnetised)
    alive = dead_mask(rng, N)
    h = make_handle(capi, par, N, seed=8, method="tiles")
    try:
        h.set_state(pos, spin, alive=alive)
        h.mark_reference()
        h.step(3)
        state = h.get_state()
        check_scalars(h, state, (pos, alive), L, 1)
        check_bins(h, state, L, 7)
        m = check_observe(h, par, state, field=None)
        wn, wc2, wm1, wm2, _ = check_structure(h, state, m, L, npad(N), 8, tag="site stride")
        last = (state[3] == 1) & (state[0] >= 262144)
        assert last.sum() >= 10 and abs(math.fsum(m[262144:])) > 1.0 and math.fsum(m[262144:] ** 2) > 1.0
        assert abs(math.fsum(m[262144:])) > sites_depth(L) * EPS * math.fsum(np.abs(m))    # dropping the second turn would show
    finally:
        h.close()


def test_empty_and_minimal_systems(capi):
    par = params(L=997, K=2, sigma=0.02)
    rng = np.random.default_rng(2)
    pos, spin = random_state(rng, par.L, 300, par.K)
    h = make_handle(capi, par, 300, method="tiles")
    try:                                                      # every particle dead
        h.set_state(pos, spin, alive=np.zeros(300, np.uint8))
        h.mark_reference()
        h.step(5)
        state = h.get_state()
        assert not state[3].any()
        want = check_all(h, par, state, (pos, np.zeros(300, np.uint8)), 300, tag="all dead")
        assert all(w == dict(dict.fromkeys(R.SCALARS, 0), max_pos=-1) for w in want.values())
        n, c2, m1, m2, F = h.observe_structure(k_max=25)
        assert (n, c2, m1, m2) == (0, 0.0, 0.0, 0.0) and not F.any()
        assert not h.observe()[2].any() and not h.observe_bins(7)[0].any()
    finally:
        h.close()
    one = make_handle(capi, par, 1, method="tiles")
    try:                                                      # one live plus particle on the last site: nothing to attempt
        one.set_state(np.array([par.L - 1], np.int32), np.array([1], np.int8))
        one.mark_reference()
        state = one.get_state()
        want = check_all(one, par, state, (state[0].copy(), np.ones(1, np.uint8)), 1, tag="one particle")["any"]
        assert want == dict(n=1, sum_sigma=1, sum_pos=par.L - 1, n_wall=1, max_pos=par.L - 1, n_range=0, attempts=0, blocked=0,
                            sum_d=0, sum_d2=0, n_d=1)
        one.step(25)
        state = one.get_state()
        check_all(one, par, state, (np.array([par.L - 1]), np.ones(1, np.uint8)), 1, tag="one particle, later")
    finally:
        one.close()


@pytest.mark.parametrize("nbins", [1, 7, 997, 996, 64])
def test_bins(capi, nbins):
    """L = 997: one bin, a non-dividing width (7 x 143 = 1001), one site per bin, and widths that leave bins without any site
    (996 bins of 2 sites: 499 hold sites; 64 bins of 16: the last holds none, the one before it five)."""
    par = params(L=997, K=3, sigma=0.02, k_exit=1.5, **ANCHORS)
    h, pos, alive = stepped(capi, par, 2000, steps=25)
    try:
        state = h.get_state()
        plus, minus = check_bins(h, state, par.L, nbins)
        width = -(-par.L // nbins)
        held = -(-par.L // width)                             # bins that hold at least one site
        assert (nbins, width, held) in {(1, 997, 1), (7, 143, 7), (997, 1, 997), (996, 2, 499), (64, 16, 63)}
        assert not plus[held:].any() and not minus[held:].any()
        assert int(((state[3] == 1) & (state[0] >= (held - 1) * width)).sum()) == plus[held - 1] + minus[held - 1]
    finally:
        h.close()


@pytest.mark.parametrize("L,K,method", [(997, 3, "tiles"), (64, 32, "pairs")], ids=["K3", "K32"])
def test_block_tables(capi, L, K, method):
    """None, all-zero and a random table; K = 32 (a 33 x 33 table, site counts up to 32 in either 16-bit half of cnt_pm)."""
    par = params(L=L, K=K, sigma=0.05)
    N = (2 * L * K) // 3
    h, pos, alive = stepped(capi, par, N, method, steps=25)
    try:
        state = h.get_state()
        want = check_scalars(h, state, (pos, alive), L, K)
        assert want["zero"]["blocked"] == 0 < want["random"]["blocked"] != want["any"]["blocked"] and 0 < want["any"]["blocked"] <= want["any"]["attempts"]
        tab = tables(K)["random"]
        swapped = R.scalar_sums(state[0], state[1], state[3], None, None, L, K, 0, 0, -1, tab.T)
        assert swapped["blocked"] != want["random"]["blocked"]                     # (plus, minus) the other way round would show
        cp, cm = R.site_counts(state[0], state[1], state[3], L)
        assert max(cp.max(), cm.max()) >= min(K, 12)
    finally:
        h.close()


@pytest.mark.parametrize("k_max", [1, 25, 997])
def test_fourier_modes_up_to_the_lattice_length(capi, k_max):
    """k * pos reaches 996 * 996: beyond one turn for almost every mode, reduced mod L exactly before the trigonometry."""
    par = params(L=997, K=3, sigma=0.02, k_exit=1.5, **ANCHORS)
    h, pos, alive = stepped(capi, par, 2000, steps=25)
    try:
        state = h.get_state()
        m = check_observe(h, par, state)
        wn, _, _, _, wF = check_structure(h, state, m, par.L, npad(2000), k_max, tag="modes")
        assert wF[0, 0] == wn and wF[0, 1] == 0
        if k_max == par.L:                                    # a real histogram: mode L - k is the conjugate of mode k
            assert float(np.max(np.abs(wF[1:, 0] - wF[:0:-1, 0]))) < 1e-12 and float(np.max(np.abs(wF[1:, 1] + wF[:0:-1, 1]))) < 1e-12
            assert float(np.max(np.abs(wF[1:]))) > 10.0
    finally:
        h.close()


SUMMED = ("n", "sum_sigma", "sum_pos", "n_wall", "n_range", "attempts", "blocked", "sum_d", "sum_d2", "n_d")


@pytest.mark.parametrize("world,periodic,interval", [(2, False, 1), (3, False, 0), (2, True, 3)])
def test_site_sharded_observables_add_up(capi, world, periodic, interval):
    """Site-range shards driven as in test_site_sharded_tiles_equal_single_handle (propose, halo_from, commit; L = 6000, K = 2,
    N = 5200, anchors with exits; the active rate is 14 so that enough particles change ranks).  The single handle marks its
    reference after 20 steps; every 20 further steps, four times, so that observations also fall between two exchanges:
      bins, site counts, n, sum count^2, Fourier sums, sum m, sum m^2 ... added over the ranks == the single handle / the reference
      m_field of a rank ... the single handle's bits on the own sites, 0 elsewhere
      scalars ... added over the ranks (max for max_pos) whenever the halo is current (age 0: after EVERY step here, so that the
                  boundary pairs are met); between two exchanges a rank with a right neighbour refuses, the last rank answers
      aps_mark_reference ... refused on a rank, so the three displacement sums of a rank are 0
      exit log ... merged over the ranks == the single handle's."""
    par = params(L=6000, K=2, sigma=0.002, periodic=periodic, k_exit=0.7, rate_diffusion=3.0, rate_active=14.0, **ANCHORS)
    L, K, N, dt, seed = par.L, par.K, 5200, 0.04, 31
    pos, spin = random_state(np.random.default_rng(77), L, N, K)
    orc = so.SyncOracle(par, dt=dt, seed=seed)
    orc.set_state(pos, spin)
    ranks = [make_handle(capi, par, N, dt=dt, seed=seed, rank=r, world=world, method="tiles", halo_interval=interval) for r in range(world)]
    single = make_handle(capi, par, N, dt=dt, seed=seed, method="tiles")
    x_wall, lo, hi = (7 * L) // 10, L // 10, L // 3
    hits = {"boundary": 0, "summed": 0, "refused": 0}

    def scalars_over_ranks(age, both_tables=False):
        st = (orc.pos, orc.spin, orc.bound, orc.alive)
        live = orc.alive == 1
        occ = np.bincount(orc.pos[live], minlength=L + 1)
        for name in ("any", "random") if both_tables else ("any",):
            tab, parts = tables(K)[name], []
            for h, (b0, b1) in zip(ranks, bounds):
                if age != 0 and b1 < L:
                    refused(capi, lambda: h.observe_scalars(x_wall=x_wall, range_lo=lo, range_hi=hi, block_table=tab), "aps_observe_scalars")
                    refused(capi, lambda: h.observe_scalars_all(x_wall=x_wall, block_table=tab), "aps_observe_scalars_all")
                    hits["refused"] += 1
                else:
                    parts.append(h.observe_scalars(x_wall=x_wall, range_lo=lo, range_hi=hi, block_table=tab))
                    assert parts[-1] == h.observe_scalars_all(x_wall=x_wall, ranges=[(lo, hi)], block_table=tab)[0]
                    own = (orc.pos >= b0) & (orc.pos < b1)
                    assert parts[-1]["n"] == int((live & own).sum()) and parts[-1]["n_d"] == 0
            if age == 0:
                got = {k: sum(p[k] for p in parts) for k in SUMMED}
                got["max_pos"] = max(p["max_pos"] for p in parts)
                assert got == R.scalar_sums(*st[:2], st[3], None, None, L, K, x_wall, lo, hi, tab), name
                hits["summed"] += 1
        if age == 0:
            hits["boundary"] += sum(bool((live & (orc.spin > 0) & (orc.pos == b1 - 1)).any() and occ[b1] > 0) for _, b1 in bounds if b1 < L)

    def advance(nsteps, observe):
        for _ in range(nsteps):
            for h in ranks:
                h.propose()
            due = ranks[0].halo_info()[2]
            for r, h in enumerate(ranks):
                nb = {(r - 1) % world, (r + 1) % world} if periodic else {q for q in (r - 1, r + 1) if 0 <= q < world}
                for q in sorted(nb) if due else []:
                    h.halo_from(ranks[q])
            for h in ranks:
                h.commit()
            orc.run(1)
            if observe and ranks[0].halo_info()[1] == 0:
                scalars_over_ranks(0)
        single.step(nsteps)

    try:
        bounds = [h.owned_sites() for h in ranks]
        for h in ranks + [single]:
            h.set_state(pos, spin)
        scalars_over_ranks(0, True)                           # straight after the upload every rank holds every cell
        advance(20, False)
        single.mark_reference()
        for h in ranks:
            refused(capi, h.mark_reference, "aps_mark_reference")
        ref = (orc.pos.copy(), orc.alive.copy())
        owner = lambda p: np.searchsorted([b[1] for b in bounds], p, side="right")
        moved = 0
        for block in range(4):
            advance(20, True)
            p, s, b, a, seen = _merged_state(ranks, N)
            assert np.array_equal(seen, np.ones(N, int)), block
            for x, y in zip((p, s, b, a), single.get_state()):
                assert np.array_equal(x, y), block
            assert np.array_equal(p, orc.pos) and np.array_equal(s, orc.spin) and np.array_equal(a, orc.alive)
            state = (p, s, b, a)
            age = ranks[0].halo_info()[1]
            scalars_over_ranks(age, True)
            assert single.observe_scalars(x_wall=x_wall, range_lo=lo, range_hi=hi) == R.scalar_sums(p, s, a, ref[0], ref[1], L, K, x_wall, lo, hi)
            both = (a == 1) & (ref[1] == 1)
            moved = max(moved, int((owner(p[both]) != owner(ref[0][both])).sum()))
            for nbins in (7, 64):                             # bins
                parts = [h.observe_bins(nbins) for h in ranks]
                want = R.bin_sums(p, s, a, L, nbins)
                assert np.array_equal(sum(x[0] for x in parts), want[0]) and np.array_equal(sum(x[1] for x in parts), want[1])
            cps, cms, ms = single.observe()                   # aps_observe
            assert np.array_equal(ms, orc.field_sites()[2])
            parts = [h.observe() for h in ranks]
            assert np.array_equal(sum(x[0] for x in parts), cps) and np.array_equal(sum(x[1] for x in parts), cms)
            for (b0, b1), (_, _, m) in zip(bounds, parts):
                assert np.array_equal(m[b0:b1], ms[b0:b1]) and not m[:b0].any() and not m[b1:].any()
            k_max = 8                                         # aps_observe_structure
            parts = [h.observe_structure(k_max=k_max) for h in ranks]
            wn, wc2, wm1, wm2, wF = R.structure_sums(p, a, L, k_max, ms)
            assert sum(x[0] for x in parts) == wn and sum(x[1] for x in parts) == wc2
            F = sum(x[4].astype(np.longdouble) for x in parts)
            m1, m2, d = math.fsum(x[2] for x in parts), math.fsum(x[3] for x in parts), sites_depth(L) + 1   # (+ 1: the sum over ranks)
            err_f, b_f = float(np.max(np.abs(F - wF))), dft_bound(npad(N, world), wn)
            print(f"world {world} block {block} age {age}: Fourier error {err_f:.3e} (bound {b_f:.3e}), sum m error {abs(m1 - wm1):.3e} "
                  f"(bound {d * EPS * math.fsum(np.abs(ms)):.3e}), sum m^2 error {abs(m2 - wm2):.3e} (bound {d * EPS * wm2:.3e})")
            assert err_f <= b_f and abs(m1 - wm1) <= d * EPS * math.fsum(np.abs(ms)) and abs(m2 - wm2) <= d * EPS * wm2
            assert single.observe_structure(k_max=k_max)[:2] == (wn, wc2)
        ex = np.concatenate([h.exits() for h in ranks])
        ex = ex[np.lexsort((ex[:, 2], ex[:, 0]))]
        assert len(ex) > 0 and np.array_equal(ex, single.exits())
        k = ranks[0].halo_info()[0]
        print(f"world {world} interval {k}: {hits}, {moved} particles on another rank than at the mark")
        assert hits["boundary"] >= 1 and hits["summed"] >= 4 and moved >= 10 and (k == 1 or hits["refused"] >= 1)
    finally:
        for h in ranks + [single]:
            h.close()
