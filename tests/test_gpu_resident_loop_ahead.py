"""GPU suite (-m gpu): the eight-wave resident loop's wait for the records (csrc/tile_loop.hpp) and the shapes at which a change of
the order between barrier E and barrier S can go wrong.  The kernel spaces its re-polls of a record that is not there yet
(TL_REPOLL_SLEEP); the order of an iteration is the one of tests/test_gpu_resident_loop_chain.py.  The plan this file was written
for -- barrier F taken away, the particle list read behind barrier S, the owned particles' random numbers drawn one step ahead
into an LDS array keyed by frame position, a source offset in the list entry -- passed every case below and was not kept: it
was no faster.  The cases stay as the bar for the next attempt on that chain, and they hold the spaced polls:
three-step calls, the give-up path with a wait that runs out between two spaced polls, config 2's own instance at small size.

Replaces the loop of ParticleSystem.run (PARTICLE_solver_CLASS.py:511-516) like aps_step itself.  The bar is the one of
tests/test_gpu_resident_loop_chain.py -- integer state and {W, S, occupancy} identical to the CPU oracle's after every call --
and after every call the eight-wave kernel is also held against the four-wave kernel and against one launch per step, bit for
bit.  Frames are forced (APS_TS_R, APS_TS_OWN); the shapes are the smallest at which each piece can go wrong, and what makes a
shape bite is asserted from the oracle's states."""
import contextlib
import importlib
import os

import numpy as np
import pytest

from oracle import sync_oracle as so
from test_gpu_parity import check_lattice, make_handle, params, random_state

pytestmark = pytest.mark.gpu
PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"
CALLS = (7, 4, 1, 33, 2, 50, 3)                      # odd and even calls, calls too short for the loop, and the shortest loop last
ANCHORS = dict(anchor_positions=[0.3, 0.7], anchor_radius=0.08, k_on=3.0, k_off=1.0, k_exit=0.0)


@pytest.fixture(scope="module")
def capi():
    mod = importlib.import_module(PKG + ".capi")
    assert mod.device_count() >= 1, "no GPU visible"
    return mod


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def same_state(h, orc, tag=""):
    p, sg, bd, al = h.get_state()
    assert np.array_equal(al, orc.alive), tag
    assert np.array_equal(p, orc.pos), tag
    assert np.array_equal(sg, orc.spin), tag
    assert np.array_equal(bd, orc.bound), tag


def same_bits(a, b, tag="", ensembles=1):
    for e in range(ensembles):
        for x, y in zip(a.get_state(ensemble=e), b.get_state(ensemble=e)):
            assert np.array_equal(x, y), (tag, e)
        for x, y in zip(a.get_lattice(e), b.get_lattice(e)):
            assert np.array_equal(x, y), (tag, e)


def frame_counts(pos, alive, L, own):
    """Particles on the frame of every tile (its owned sites and two either side, clipped at the walls)."""
    occ = np.bincount(pos[alive != 0], minlength=L)
    csum = np.concatenate(([0], np.cumsum(occ)))
    ntile = (L + own - 1) // own
    lo = np.maximum(np.arange(ntile) * own - 2, 0)
    hi = np.minimum(np.minimum((np.arange(ntile) + 1) * own, L) + 2, L)
    return csum[hi] - csum[lo]


# rs: rows of the forced frame; own: forced owned sites per tile (default 64 rs - 4); frac: density
WAIT_CASES = [
    # 18 tiles of 160 sites, fast diffusion: in most steps an owned site's particle came from the halo (either side) and a halo
    # particle came from an owned site -- the list of a step is built from cells that moved across the owned/halo edge
    dict(tag="boundary_traffic", rs=5, own=160, L=2880, K=1, sigma=0.01, frac=0.6, rate_diffusion=6.0, rate_active=16.0),
    # refused hops (a rival wins the target); every interior frame above 256 particles: both halves of the workgroup hold particles
    dict(tag="crowded", rs=5, L=316 * 4, K=1, sigma=0.01, frac=0.9, rate_diffusion=6.0),
    # frames holding about 256 particles: the count crosses the half of the workgroup between steps
    dict(tag="crossing_half", rs=5, L=316 * 4, K=1, sigma=0.01, frac=0.8, rate_diffusion=6.0, rate_active=10.0),
    # a tile that is its own neighbour, and one that is its neighbour's neighbour on both sides
    dict(tag="one_tile_torus", rs=5, L=300, K=1, sigma=0.02, periodic=True, frac=0.5),
    dict(tag="two_tiles_torus", rs=5, L=632, K=1, sigma=0.01, periodic=True, frac=0.5),
    # the shortest owned ranges: the last tile owns exactly 3 sites, or 5
    dict(tag="ragged_last_tile_3", rs=5, L=316 * 3 + 3, K=1, sigma=0.01, frac=0.5),
    dict(tag="ragged_last_tile_5", rs=5, L=316 * 3 + 5, K=1, sigma=0.01, frac=0.5),
    # a box comparable to the reach: the instance that carries the image list
    dict(tag="small_box_images", rs=5, L=600, K=1, sigma=0.3, frac=0.6),
    # unbinding changes the cell word of a particle but not its id; the particles on anchor sites start bound
    dict(tag="anchors", rs=5, L=900, K=1, sigma=0.02, frac=0.5, **ANCHORS),
    # config 2's own instance (frames of 7 rows, walls) and the widest one, three tiles each
    dict(tag="seven_rows", rs=7, L=3 * (64 * 7 - 4), K=1, sigma=0.01, frac=0.5),
    dict(tag="eight_rows", rs=8, L=3 * (64 * 8 - 4), K=1, sigma=0.01, frac=0.5),
]


def build(capi, case, dt=0.04, seed=20260202, betas=None, nhandles=3):
    """Oracle(s) and handles on the same initial state: eight waves, four waves, one launch per step."""
    case = dict(case)
    tag, frac, rs = case.pop("tag"), case.pop("frac"), case.pop("rs")
    own = case.pop("own", None)
    par = params(**case)
    rng = np.random.default_rng(11)
    N = max(1, int(frac * par.L * par.K))
    nens = len(betas) if betas else 1
    states = [random_state(rng, par.L, N, par.K) for _ in range(nens)]
    states = [(pos, spin, np.ascontiguousarray(par.is_anchor_site[pos] != 0, dtype=np.uint8)) for pos, spin in states]
    orcs = []
    for e, (pos, spin, bound) in enumerate(states):
        pe = params(**dict(case, beta=betas[e])) if betas else par
        orc = so.SyncOracle(pe, dt=dt, seed=seed, **(dict(ensemble=e) if betas else {}))
        orc.set_state(pos, spin, bound=bound)
        orcs.append(orc)
    geometry = dict(APS_TS_R=rs, **(dict(APS_TS_OWN=own) if own else {}))
    with env(**geometry):                                # (read when the handle is made)
        handles = [make_handle(capi, par, N, dt=dt, seed=seed, method="tiles", **(dict(beta=betas) if betas else {})) for _ in range(nhandles)]
    if nhandles == 3:
        handles[2].set_resident_loop(False)
    for h in handles:
        for e, (pos, spin, bound) in enumerate(states):
            h.set_state(pos, spin, bound=bound, ensemble=e)
        assert h.tiles_info()["frame_sites"] == 64 * rs, (tag, h.tiles_info())
    return tag, par, states, orcs, handles


def run_calls(tag, par, states, orcs, handles, watch=None, four_wave_kernel=True):
    """The call pattern on all three handles and the oracle(s); after every call the three comparisons.  watch(orc) is called
    on ensemble 0's oracle after every single step.  four_wave_kernel=False: binary64 frames of 8 rows have no kernel of four
    waves (it would need more than 256 VGPRs), the handle that is refused eight waves steps with one launch per step."""
    wide, narrow, per_step = handles
    total = 0
    for n in CALLS:
        with env(APS_LOOP_MIN=3, APS_LOOP_WAVES=8):
            wide.step(n)
        with env(APS_LOOP_MIN=3, APS_LOOP_WAVES=4):
            narrow.step(n)
        per_step.step(n)
        for _ in range(n):
            for orc in orcs:
                orc.run(1)
            if watch:
                watch(orcs[0])
        total += n
        taken, state, why = wide.loop_info()
        assert state == 1, (tag, why)
        assert taken == (0 if n < 3 else n), (tag, n, taken)
        assert wide.loop_waves() == 8, tag
        if not four_wave_kernel:
            assert narrow.loop_info()[0] == 0 and narrow.loop_waves() == 0, (tag, n, narrow.loop_waves(), narrow.loop_info())
        elif n >= 3:                                         # the four-wave handle took the loop too, with four waves
            assert narrow.loop_waves() == 4 and narrow.loop_info()[0] == n, (tag, n, narrow.loop_waves(), narrow.loop_info())
        else:
            assert narrow.loop_waves() in (0, 4), tag
        assert per_step.loop_info()[0] == 0, tag
        if len(orcs) == 1:
            same_state(wide, orcs[0], (tag, total))
            check_lattice(wide, orcs[0])
        else:
            for e, orc in enumerate(orcs):
                got = wide.get_state(ensemble=e)
                assert np.array_equal(got[0], orc.pos) and np.array_equal(got[1], orc.spin), (tag, total, e)
                check_lattice(wide, orc, ensemble=e)
        same_bits(wide, narrow, (tag, total, "four waves"), len(orcs))
        same_bits(wide, per_step, (tag, total, "one launch per step"), len(orcs))
    assert CALLS[-1] == 3 and wide.loop_info()[0] == 3, tag      # the shortest loop: a first iteration, one in the middle, a last one
    assert wide.time()[1] == total
    assert not np.array_equal(wide.get_state()[0], states[0][0])


@pytest.mark.parametrize("case", WAIT_CASES, ids=lambda c: c["tag"])
def test_wait_equals_oracle_four_waves_and_one_launch_per_step(capi, case):
    tag, par, states, orcs, handles = build(capi, case)
    info = handles[0].tiles_info()
    own, ntile = info["owned_sites"], info["n_tiles"]
    pos0 = states[0][0]
    moved_tile = np.zeros(len(pos0), bool)
    counts = []
    prev = [pos0.copy()]
    crossed = dict(from_left=0, from_right=0, left=0)

    def watch(orc):
        moved_tile[:] |= (orc.pos // own) != (pos0 // own)
        counts.append(frame_counts(orc.pos, orc.alive, par.L, own))
        dt_ = orc.pos // own - prev[0] // own                # (walls in the cases that look at this: no wrap)
        crossed["from_left"] += int((dt_ == 1).sum())        # entered the owned range of the tile to the right, from its left side
        crossed["from_right"] += int((dt_ == -1).sum())
        crossed["left"] += int((dt_ != 0).sum())
        prev[0] = orc.pos.copy()

    try:
        if tag.startswith("ragged_last_tile"):
            assert par.L - (ntile - 1) * own == int(tag[-1]), (tag, own, ntile)
        if tag == "two_tiles_torus":
            assert ntile == 2
        if tag == "one_tile_torus":
            assert ntile == 1
        if tag in ("seven_rows", "eight_rows"):
            assert ntile == 3 and own == info["frame_sites"] - 4, (tag, info)
        run_calls(tag, par, states, orcs, handles, watch, four_wave_kernel=tag != "eight_rows")
        c = np.array(counts)                                 # [step][tile]
        if tag == "boundary_traffic":
            assert ntile >= 5 and int(moved_tile.sum()) >= 50, (tag, ntile, int(moved_tile.sum()))
            # a particle entered an owned range from each side, and one left its owned range
            assert crossed["from_left"] > 0 and crossed["from_right"] > 0 and crossed["left"] > 0, (tag, crossed)
        if tag == "crossing_half":                           # some tile's frame above 256 particles in one step, at or below in another
            assert ((c > 256).any(axis=0) & (c <= 256).any(axis=0)).any(), (tag, c.min(axis=0), c.max(axis=0))
        if tag == "anchors":                                 # bound particles let go
            assert int(orcs[0].bound.sum()) <= int(states[0][2].sum()) - 10, (tag, int(orcs[0].bound.sum()), int(states[0][2].sum()))
        if tag == "crowded":                                 # every interior tile above 256 throughout
            assert ntile >= 3 and (c[:, 1:-1] > 256).all(), (tag, c.min(axis=0))
    finally:
        for h in handles:
            h.close()


def test_wait_two_ensembles(capi):
    """Two values of beta in one launch: the ensemble word of the Philox counter, and two ensembles' records polled side by side."""
    case = dict(tag="two_ensembles", rs=5, L=316 * 3, K=1, sigma=0.01, frac=0.6, rate_diffusion=6.0)
    tag, par, states, orcs, handles = build(capi, case, seed=77, betas=[0.3, 2.0])
    try:
        run_calls(tag, par, states, orcs, handles)
        assert not np.array_equal(orcs[0].pos - states[0][0], orcs[1].pos - states[1][0])
    finally:
        for h in handles:
            h.close()


@pytest.mark.parametrize("n", [10, 11], ids=["even_call", "odd_call"])
def test_wait_give_up_mid_loop(capi, n):
    """The bounded-wait exit with spaced polls: tile 3 leaves at the top of iteration 2 without its record, its neighbours' waits
    run out after 2 ms (the clock is read every 64 polls, each now 16 sleeps apart), every workgroup leaves through the exit
    behind barrier S, and the call is repeated with one launch per step from the intact inputs -- after an even and after an
    odd number of steps (the buffer sets trade places or not)."""
    tag, par, states, orcs, handles = build(capi, WAIT_CASES[0], seed=31, nhandles=1)
    wide, orc = handles[0], orcs[0]
    try:
        with env(APS_LOOP_MIN=3, APS_LOOP_WAVES=8):
            wide.step(5)
            orc.run(5)
            assert wide.loop_info()[:2] == (5, 1) and wide.loop_waves() == 8
            same_state(wide, orc)
            with env(APS_LOOP_TEST_STALL="3:2", APS_LOOP_TIMEOUT_MS=2):
                wide.step(n)
            orc.run(n)
            taken, state, why = wide.loop_info()
            assert (taken, state) == (0, -1) and "ran out" in why, (taken, state, why)
            assert wide.time()[1] == 5 + n
            same_state(wide, orc)
            check_lattice(wide, orc)
            wide.step(20)
            orc.run(20)
            assert wide.loop_info()[:2] == (0, -1)
            same_state(wide, orc)
            check_lattice(wide, orc)
    finally:
        wide.close()
