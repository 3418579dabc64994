"""GPU suite (-m gpu): the model record as the eight-wave resident loop reads it (csrc/tile_loop.hpp, tl_load_model).  Behind
barrier B every iteration reads the record of rates, switches, seeds and the flip table's address; the eight-wave kernel does so
with scalar loads through the constant address space, word by word, the four-wave kernel and tile_step through a plain pointer.
A word that lands in the wrong field changes a rate or a switch, so every case below sets fields away from their defaults at
both ends of the record and holds the eight-wave kernel -- after every call -- against the CPU oracle (integer state, {W, S},
occupancy), against the four-wave kernel and against one launch per step, bit for bit.  That a field matters in its case is
asserted from a second oracle that runs without it.

Replaces the loop of ParticleSystem.run (PARTICLE_solver_CLASS.py:511-516) like aps_step itself."""
import numpy as np
import pytest

from oracle import sync_oracle as so
from test_gpu_parity import check_lattice, make_handle, params, random_state
from test_gpu_resident_loop_ahead import ANCHORS, capi, env, same_bits, same_state  # noqa: F401  (capi: the fixture)

pytestmark = pytest.mark.gpu
CALLS = (7, 2, 12, 3)                                    # odd and even loops, a call too short for the loop, the shortest loop last


def tanh_table(n=16):
    """[2][n + 1]: a caller's flip rate 1 - 0.8 sigma tanh(2 m) tabulated at m = -1 + 2 i / n (aps_set_flip_table's layout)."""
    m = -1.0 + 2.0 * np.arange(n + 1) / n
    return np.ascontiguousarray(np.stack([1.0 - 0.8 * np.tanh(2.0 * m), 1.0 + 0.8 * np.tanh(2.0 * m)]))


# rs: rows of the forced frame; plain: the same case with the fields under test at their defaults (a second oracle)
MODEL_CASES = [
    # the last two fields of the record: the table's length and its address
    dict(tag="flip_table", rs=5, L=316 * 3, sigma=0.01, frac=0.5, table=True),
    dict(tag="flip_table_seven_rows_torus", rs=7, L=2 * (64 * 7 - 4), sigma=0.01, frac=0.5, periodic=True, table=True),
    # the switches at the record's head, all away from their defaults, with the binding rates behind them
    dict(tag="switches", rs=5, L=900, sigma=0.02, frac=0.5, minus_anchor=False, immobilize_when_anchored=False,
         suppress_flip_when_bound=False, **ANCHORS),
    # the two rates in the middle (the crowding switch next to them decides nothing with one cell per site: no case for it)
    dict(tag="rates", rs=5, L=316 * 3, sigma=0.01, frac=0.8, rate_diffusion=6.0, rate_active=16.0),
    # the ensemble word of the Philox counter, between the seeds and the table
    dict(tag="ensemble_base", rs=5, L=316 * 3, sigma=0.01, frac=0.5, ens_base=5),
]
DEFAULTS = dict(minus_anchor=True, immobilize_when_anchored=True, suppress_flip_when_bound=True, rate_diffusion=0.6, rate_active=4.0)


@pytest.mark.parametrize("case", MODEL_CASES, ids=lambda c: c["tag"])
def test_model_fields_equal_oracle_four_waves_and_one_launch_per_step(capi, case):
    case = dict(case)
    tag, rs, frac = case.pop("tag"), case.pop("rs"), case.pop("frac")
    table = tanh_table() if case.pop("table", False) else None
    ens_base = case.pop("ens_base", 0)
    dt, seed = 0.04, 20261020
    par = params(K=1, **case)
    plain = params(K=1, **{k: DEFAULTS.get(k, v) for k, v in case.items()})
    rng = np.random.default_rng(5)
    N = int(frac * par.L)
    pos, spin = random_state(rng, par.L, N, 1)
    bound = np.ascontiguousarray(par.is_anchor_site[pos] != 0, dtype=np.uint8)
    orc = so.SyncOracle(par, dt=dt, seed=seed, ensemble=ens_base, flip_table=table)
    other = so.SyncOracle(plain, dt=dt, seed=seed)        # the same run without the fields under test
    for o in (orc, other):
        o.set_state(pos, spin, bound=bound)
    with env(APS_TS_R=rs):                                # (read when the handle is made)
        handles = [make_handle(capi, par, N, dt=dt, seed=seed, method="tiles", beta=[par.beta], ensemble_base=ens_base) for _ in range(3)]
    wide, narrow, per_step = handles
    try:
        per_step.set_resident_loop(False)
        for h in handles:
            if table is not None:
                h.set_flip_table(table)
            h.set_state(pos, spin, bound=bound)
            assert h.tiles_info()["frame_sites"] == 64 * rs, (tag, h.tiles_info())
        total = 0
        for n in CALLS:
            with env(APS_LOOP_MIN=3, APS_LOOP_WAVES=8):
                wide.step(n)
            with env(APS_LOOP_MIN=3, APS_LOOP_WAVES=4):
                narrow.step(n)
            per_step.step(n)
            orc.run(n)
            other.run(n)
            total += n
            taken, state, why = wide.loop_info()
            assert state == 1 and taken == (0 if n < 3 else n) and wide.loop_waves() == 8, (tag, n, taken, state, why)
            if n >= 3:
                assert narrow.loop_waves() == 4 and narrow.loop_info()[0] == n, (tag, n, narrow.loop_info())
            assert per_step.loop_info()[0] == 0, tag
            same_state(wide, orc, (tag, total))
            check_lattice(wide, orc)
            same_bits(wide, narrow, (tag, total, "four waves"))
            same_bits(wide, per_step, (tag, total, "one launch per step"))
        assert wide.time()[1] == total
        # the fields under test decided something: without them the run ends elsewhere
        assert not (np.array_equal(orc.pos, other.pos) and np.array_equal(orc.spin, other.spin) and np.array_equal(orc.bound, other.bound)), tag
    finally:
        for h in handles:
            h.close()
