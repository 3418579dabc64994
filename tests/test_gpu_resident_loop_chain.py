"""GPU suite (-m gpu): the eight-wave resident loop's chain from exclusion to the next sweep (csrc/tile_loop.hpp).  The halo
particles' random numbers are drawn behind barrier S by the wave that appended them to the list and picked up from LDS in the
proposals phase; a boundary cell is published by its thread in the exclusion phase, the record's tail first thing after
barrier E.

Replaces the loop of ParticleSystem.run (PARTICLE_solver_CLASS.py:511-516) like aps_step itself.  The bar is the one of
tests/test_gpu_resident_loop_wide.py -- integer state and {W, S, occupancy} identical to the CPU oracle's after every call --
and after every call the eight-wave kernel is also held against the four-wave kernel and against one launch per step, bit for
bit.  Frames are forced (APS_TS_R, APS_TS_OWN); the shapes are the smallest at which each piece can go wrong, and what makes a
shape bite (particles that change tile, frames around and above 256 particles) is asserted from the oracle's states."""
import contextlib
import importlib
import os

import numpy as np
import pytest

from oracle import sync_oracle as so
from test_gpu_parity import check_lattice, make_handle, params, random_state

pytestmark = pytest.mark.gpu
PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"
CALLS = (7, 4, 1, 33, 2, 50, 3)                      # odd and even calls, calls too short for the loop, observations in between
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
CHAIN_CASES = [
    # 18 tiles of 160 sites, fast diffusion: particles cross tile boundaries in most steps -- an owned site's particle that came
    # from the halo, a halo particle that came from an owned site
    dict(tag="boundary_traffic", rs=5, own=160, L=2880, K=1, sigma=0.01, frac=0.6, rate_diffusion=6.0, rate_active=16.0),
    # a tile that is its neighbour's neighbour on both sides, and one that is its own neighbour
    dict(tag="two_tiles_torus", rs=5, L=632, K=1, sigma=0.01, periodic=True, frac=0.5),
    dict(tag="one_tile_torus", rs=5, L=300, K=1, sigma=0.02, periodic=True, frac=0.5),
    # frames of 320 sites holding about 256 particles: the halo particles' lanes lie in wave 3 in some steps and in wave 4 in others
    dict(tag="crossing_half", rs=5, L=316 * 4, K=1, sigma=0.01, frac=0.8, rate_diffusion=6.0, rate_active=10.0),
    # always more than 256: the waves of the upper quad hold particles of their own, the halo particles among them
    dict(tag="crowded", rs=5, L=316 * 4, K=1, sigma=0.01, frac=0.9, rate_diffusion=6.0),
    # halo positions next to a very short owned range: the last tile owns 5 sites, or exactly 3
    dict(tag="ragged_last_tile_5", rs=5, L=316 * 3 + 5, K=1, sigma=0.01, frac=0.5),
    dict(tag="ragged_last_tile_3", rs=5, L=316 * 3 + 3, K=1, sigma=0.01, frac=0.5),
    # a box comparable to the reach: the instance that carries the image list
    dict(tag="small_box_images", rs=5, L=600, K=1, sigma=0.3, frac=0.6),
    # unbinding changes the cell word of a particle but not its id (the anchor shape of test_gpu_resident_loop.py with one cell per
    # site; nothing binds there -- a particle binds into free capacity of its own site -- so the particles on anchor sites start bound)
    dict(tag="anchors", rs=5, L=900, K=1, sigma=0.02, frac=0.5, **ANCHORS),
]


def build(capi, case, dt=0.04, seed=20260202, betas=None):
    """Oracle(s) and three handles on the same initial state: eight waves, four waves, one launch per step."""
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
        handles = [make_handle(capi, par, N, dt=dt, seed=seed, method="tiles", **(dict(beta=betas) if betas else {})) for _ in range(3)]
    handles[2].set_resident_loop(False)
    for h in handles:
        for e, (pos, spin, bound) in enumerate(states):
            h.set_state(pos, spin, bound=bound, ensemble=e)
        assert h.tiles_info()["frame_sites"] == 64 * rs, (tag, h.tiles_info())
    return tag, par, states, orcs, handles


def run_calls(tag, par, states, orcs, handles, watch=None):
    """The call pattern on all three handles and the oracle(s); after every call the three comparisons.  watch(orc) is called
    on ensemble 0's oracle after every single step."""
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
        if n >= 3:                                           # the four-wave handle took the loop too, with four waves
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
    assert wide.time()[1] == total
    assert not np.array_equal(wide.get_state()[0], states[0][0])


@pytest.mark.parametrize("case", CHAIN_CASES, ids=lambda c: c["tag"])
def test_chain_equals_oracle_four_waves_and_one_launch_per_step(capi, case):
    tag, par, states, orcs, handles = build(capi, case)
    own, ntile = handles[0].tiles_info()["owned_sites"], handles[0].tiles_info()["n_tiles"]
    pos0 = states[0][0]
    moved_tile = np.zeros(len(pos0), bool)
    counts = []

    def watch(orc):
        moved_tile[:] |= (orc.pos // own) != (pos0 // own)
        counts.append(frame_counts(orc.pos, orc.alive, par.L, own))

    try:
        if tag.startswith("ragged_last_tile"):
            assert par.L - (ntile - 1) * own == int(tag[-1]), (tag, own, ntile)
        if tag == "two_tiles_torus":
            assert ntile == 2
        if tag == "one_tile_torus":
            assert ntile == 1
        run_calls(tag, par, states, orcs, handles, watch)
        c = np.array(counts)                                 # [step][tile]
        if tag == "boundary_traffic":
            assert ntile >= 5 and int(moved_tile.sum()) >= 50, (tag, ntile, int(moved_tile.sum()))
        if tag == "crossing_half":                           # some tile's frame above 256 particles in one step, at or below in another
            assert ((c > 256).any(axis=0) & (c <= 256).any(axis=0)).any(), (tag, c.min(axis=0), c.max(axis=0))
        if tag == "anchors":                                 # bound particles let go
            assert int(orcs[0].bound.sum()) <= int(states[0][2].sum()) - 10, (tag, int(orcs[0].bound.sum()), int(states[0][2].sum()))
        if tag == "crowded":                                 # every interior tile above 256 throughout
            assert ntile >= 3 and (c[:, 1:-1] > 256).all(), (tag, c.min(axis=0))
    finally:
        for h in handles:
            h.close()


def test_chain_two_ensembles(capi):
    """Two values of beta in one launch: the ensemble word of the Philox counter, for the halo particles' numbers too."""
    case = dict(tag="two_ensembles", rs=5, L=316 * 3, K=1, sigma=0.01, frac=0.6, rate_diffusion=6.0)
    tag, par, states, orcs, handles = build(capi, case, seed=77, betas=[0.3, 2.0])
    try:
        run_calls(tag, par, states, orcs, handles)
        assert not np.array_equal(orcs[0].pos - states[0][0], orcs[1].pos - states[1][0])
    finally:
        for h in handles:
            h.close()
