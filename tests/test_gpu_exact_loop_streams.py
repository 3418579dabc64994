"""GPU suite (-m gpu): the random streams of the device-resident exact event loop, pinned to a CPU Philox.

Every entry point of the exact loop draws its four numbers per event from Philox4x32-10 on the device unless the caller hands
it a table (`uniforms`).  The other modules feed tables (which bypasses the Philox branch), compare seeded runs with seeded runs,
or look at ensemble means; none of that sees a batch whose members share a stream.  Here each entry point gets the same pin:

(a) run seeded; build the table the headers promise for that key and stream with oracle/philox_streams.py (plain NumPy,
    held to the Random123 known answers by tests/test_philox_streams_cpu.py); run again with `uniforms=` that table.  Both runs
    execute the same arithmetic on the same numbers, so every output must be equal bit for bit, t_final included.  The table has
    two draw blocks of rows more than the seeded run fired events, and the seeded run must have stopped at least one block short
    of the table's end: it ended on T, not on the row count, and every block of draws it took lies inside the table.
(b) for the one-wavefront batch kernel and the large kernel, the CPU restatement of the reference (oracle/gillespie_numpy.py)
    is driven with the same table through TableRng and the event loop of tests/test_gpu_gillespie.py: integers exact, times to
    rtol 1e-12 (that module's bar and caveat: a draw within 1e-10 of a threshold could split the two sides; the seeds here are
    fixed and none lands there).

Every key has a non-zero high word.  Every batch holds at least three systems with identical initial states and beta: they differ
through the stream alone, and must differ pairwise.

Key and stream per entry point (include/gillespie.h, gillespie_many.h, gillespie_mixed.h):
    gil_run_batch (run_raw)              key seed,                 stream s
    gil_run_large (run_large_raw)        key seed,                 stream 0
    gilm_run (run_many_large_raw)        key (seed + s) mod 2^64,  stream 0
    gilx_run (run_mixed_raw)             key seeds[s],             stream streams[s]

The structure, capture, profile and mixed-structure entry points instantiate the same kernels, hence the same draw code; that each
leaves the seeded trajectory of run_raw / run_many_large_raw / run_mixed_raw untouched is shown by
    test_gpu_gillespie_structure.py::test_recording_changes_nothing
    test_gpu_gillespie_capture.py::test_philox_batches_repeat_and_leave_the_trajectory_alone
    test_gpu_gillespie_profile.py::test_recording_changes_nothing_else
    test_gpu_gillespie_mixed_structure.py::test_mixed_launch_equals_the_structure_launches_it_replaces
so the pin is not repeated per instantiation.

Events fired per system at the shapes below (the asserted floors are the issue's, several draw blocks each):
    batch, one wavefront   L=120  N=70   K=3         T=2.5   floor 3 x 64
    batch, 256 threads     L=600  N=1030 K=2         T=0.5   floor 2 x 256
    large                  L=1500 N=900  K=1 global  T=1.3   floor 2 x 1024, at most 3000 (the oracle leg)
    many large             L=400  N=300  n_cap=2049  T=1.6   floor 1024
    mixed, one wavefront   L=200  N=110  K=2         T=1.2   floor 3 x 64
    mixed, 256 threads     L=600  N=1030 / 400, K=2  T=0.8   floor 2 x 256
"""
import importlib

import numpy as np
import pytest

from oracle import philox_streams as ps
from oracle.gillespie_numpy import GillespieOracle
from test_gpu_gillespie import TableRng, oracle_event_loop      # noqa: F401  (TableRng is what oracle_event_loop drives)

pytestmark = pytest.mark.gpu
PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"
TRAJECTORY_KEYS = ("pos", "sigma", "flags", "scalars", "n_recorded", "n_events", "t_final", "exits", "n_exits")
KEY = 0x9E3779B97F4A7C15


@pytest.fixture(scope="module")
def gil():
    assert importlib.import_module(PKG + ".capi").device_count() >= 1
    return importlib.import_module(PKG + ".gillespie")


def _oracle(N, rng_seed=17, **case):
    kw = dict(xlim=1.0, scale_rates=False, k_on=0.0, k_off=0.0, k_exit=0.0)
    kw.update(case)
    orc = GillespieOracle(init="fixed", N=N, rng=np.random.default_rng(rng_seed), **kw)
    pos0, sigma0 = orc.init_particles()
    return orc, pos0, sigma0


def _raw(orc, sigma=True):
    P = orc.par
    kw = dict(L=P.L, K=P.K, periodic=P.periodic, rate_diffusion=P.rate_diffusion, rate_active=P.rate_active,
              minus_anchor=P.minus_anchor, immobilize=P.immobilize_when_anchored, suppress_flip=P.suppress_flip_when_bound,
              crowding=P.crowding_suppresses_rates, k_on=P.k_on, k_off=P.k_off, k_exit=P.k_exit, anchor_mask=P.is_anchor_site)
    if sigma:
        kw["sigma_grid"] = P.sigma_grid if P.sigma_kernel > 0 else 0.0
    return kw


def _tables(keys_and_streams, n_events, block):
    """[systems][rows][4] from the CPU Philox: rows = the most events any system fired + two draw blocks."""
    rows = int(np.max(n_events)) + 2 * block
    return np.stack([ps.exact_loop_uniforms(key, stream, rows) for key, stream in keys_and_streams])


def _pin(seeded, tabled, tables, block, floor, what):
    """(a): the seeded run and the run fed the CPU-built table, bit for bit."""
    rows = tables.shape[-2]
    n_events = np.atleast_1d(seeded["n_events"])
    print(what, "events", n_events.tolist(), "rows", rows)
    assert np.all(n_events > floor), (what, n_events, floor)
    assert np.all(n_events <= rows - block), (what, n_events, rows)              # stopped on T, not on the row count
    for key in TRAJECTORY_KEYS:
        if key in seeded:
            assert np.array_equal(np.asarray(seeded[key]), np.asarray(tabled[key])), (what, key)


def _differ_pairwise(r, systems, what):
    for i, a in enumerate(systems):
        for b in systems[i + 1:]:
            assert r["t_final"][a] != r["t_final"][b], (what, a, b)
            assert not np.array_equal(r["pos"][a, 1:], r["pos"][b, 1:]), (what, a, b)


def _against_oracle(orc, pos0, sigma0, table, T, times, r, what):
    """(b): one system's outputs `r` (no system axis) against the oracle driven with the same table."""
    N = len(pos0)
    snaps, exits, t, ev = oracle_event_loop(orc, pos0, sigma0, table, T, times, len(table))
    assert int(r["n_events"]) == ev and int(r["n_recorded"]) == len(snaps), (what, int(r["n_events"]), ev)
    np.testing.assert_allclose(r["t_final"], t, rtol=1e-12)
    for kk, (p, s, b) in enumerate(snaps):
        live = (r["flags"][kk, :N] & 2) != 0
        assert np.array_equal(r["pos"][kk, :N][live], p), (what, kk)
        assert np.array_equal(r["sigma"][kk, :N][live], s), (what, kk)
        assert np.array_equal((r["flags"][kk, :N][live] & 1).astype(bool), b), (what, kk)
    nx = int(r["n_exits"])
    assert nx == len(exits[0])
    np.testing.assert_allclose(r["exits"][:nx, 0], exits[0], rtol=1e-12)
    assert np.array_equal(r["exits"][:nx, 1].astype(int), np.array(exits[1], dtype=int))


def _system_of(r, s):
    return {k: r[k][s] for k in TRAJECTORY_KEYS}


def test_batch_kernel_one_wavefront(gil):
    orc, pos0, sigma0 = _oracle(70, L=120, site_capacity=3, local_kernel_sigma=0.02, rate_diffusion=0.3, rate_active=5.0, beta=2.0)
    T = 2.5
    times = np.arange(0.0, T, 0.05)
    kw = dict(betas=[orc.par.beta] * 3, states=[(pos0, sigma0)] * 3, times_obs=times, T=T, **_raw(orc))
    assert len(pos0) <= 1024                                                     # one wavefront per system
    seeded = gil.run_raw(seed=KEY, **kw)
    tables = _tables([ps.batch_stream(KEY, s) for s in range(3)], seeded["n_events"], 64)
    _pin(seeded, gil.run_raw(uniforms=tables, **kw), tables, 64, 3 * 64, "batch64")
    _differ_pairwise(seeded, [0, 1, 2], "batch64")
    for s in range(3):
        _against_oracle(orc, pos0, sigma0, tables[s], T, times, _system_of(seeded, s), ("batch64", s))


def test_batch_kernel_256_threads(gil):
    orc, pos0, sigma0 = _oracle(1030, L=600, site_capacity=2, local_kernel_sigma=0.02, rate_diffusion=0.5, rate_active=4.0, beta=0.8)
    T = 0.5
    kw = dict(betas=[orc.par.beta] * 3, states=[(pos0, sigma0)] * 3, times_obs=np.arange(0.0, T, 0.05), T=T, **_raw(orc))
    assert len(pos0) > 1024                                                      # n_cap > 1024: four wavefronts per system
    seeded = gil.run_raw(seed=KEY, **kw)
    tables = _tables([ps.batch_stream(KEY, s) for s in range(3)], seeded["n_events"], 256)
    _pin(seeded, gil.run_raw(uniforms=tables, **kw), tables, 256, 2 * 256, "batch256")
    _differ_pairwise(seeded, [0, 1, 2], "batch256")


def test_large_kernel(gil):
    orc, pos0, sigma0 = _oracle(900, rng_seed=5, L=1500, site_capacity=1, local_kernel_sigma=0.0, rate_diffusion=1.0, rate_active=2.0,
                                beta=1.5)
    T = 1.3
    times = np.arange(0.0, T, 0.05)
    kw = dict(beta=orc.par.beta, state=(pos0, sigma0), times_obs=times, T=T, **_raw(orc))
    seeded = gil.run_large_raw(seed=KEY, **kw)
    table = _tables([ps.large_stream(KEY)], seeded["n_events"], 1024)[0]
    _pin(seeded, gil.run_large_raw(uniforms=table, **kw), table, 1024, 2 * 1024, "large")
    assert seeded["n_events"] <= 3000                                            # what the oracle leg is given
    _against_oracle(orc, pos0, sigma0, table, T, times, seeded, "large")
    other = gil.run_large_raw(seed=KEY ^ (1 << 40), **kw)                        # one bit of the key's high word
    assert other["t_final"] != seeded["t_final"] and not np.array_equal(other["pos"][1:], seeded["pos"][1:])


@pytest.mark.parametrize("seed", [2 ** 32 - 2, 2 ** 64 - 2], ids=["carry_into_the_high_word", "wrap_to_zero"])
def test_many_large_kernel(gil, seed):
    orc, pos0, sigma0 = _oracle(300, L=400, site_capacity=2, local_kernel_sigma=0.02, rate_diffusion=0.5, rate_active=4.0, beta=0.8)
    T = 1.6
    kw = dict(betas=[orc.par.beta] * 3, states=[(pos0, sigma0)] * 3, times_obs=np.arange(0.0, T, 0.1), T=T, n_cap=2049, **_raw(orc))
    P = orc.par
    assert gil.plan_capture(L=P.L, K=P.K, periodic=P.periodic, sigma_grid=kw["sigma_grid"], n_systems=3, n_cap=2049,
                            n_obs=len(kw["times_obs"]))["shape"] == 1            # more slots than a workgroup's LDS holds
    seeded = gil.run_many_large_raw(seed=seed, **kw)
    streams = [ps.many_large_stream(seed, s) for s in range(3)]
    assert [k for k, _ in streams] == [(seed + s) % 2 ** 64 for s in range(3)] and all(st == 0 for _, st in streams)
    tables = _tables(streams, seeded["n_events"], 1024)
    _pin(seeded, gil.run_many_large_raw(uniforms=tables, **kw), tables, 1024, 1024, ("many", seed))
    _differ_pairwise(seeded, [0, 1, 2], ("many", seed))


MIXED_KEYS = [0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0xD6E8FEB86659FD93]
MIXED_STREAMS = [5, 0, 7, 7]                     # systems 2 and 3 share a stream number under different keys


def test_mixed_kernel_one_wavefront(gil):
    orc, pos0, sigma0 = _oracle(110, L=200, site_capacity=2, local_kernel_sigma=0.02, rate_diffusion=0.5, rate_active=4.0, beta=1.1)
    T = 1.2
    kw = dict(sigma_grids=[0.02 * 200, 0.1 * 200], variant_of_system=[0, 0, 1, 0], betas=[orc.par.beta] * 4,
              states=[(pos0, sigma0)] * 4, times_obs=np.arange(0.0, T, 0.05), T=T, seeds=MIXED_KEYS, streams=MIXED_STREAMS,
              **_raw(orc, sigma=False))
    assert gil.plan_mixed(L=200, K=2, periodic=False, sigma_grids=kw["sigma_grids"], n_systems=4, n_cap=110, n_obs=len(kw["times_obs"]),
                          variant_of_system=kw["variant_of_system"])["threads"] == 64
    seeded = gil.run_mixed_raw(seed=12345, **kw)                                 # the launch's seed is not used when seeds are given
    tables = _tables([ps.mixed_stream(MIXED_KEYS, MIXED_STREAMS, s) for s in range(4)], seeded["n_events"], 64)
    _pin(seeded, gil.run_mixed_raw(uniforms=tables, **kw), tables, 64, 3 * 64, "mixed64")
    _differ_pairwise(seeded, [0, 1, 3], "mixed64")                               # same variant, state and beta: the stream alone
    _differ_pairwise(seeded, [2, 3], "mixed64")                                  # stream 7 twice, under two keys


def test_mixed_kernel_256_threads(gil):
    """The mixed case with one system of 1030 slots (L = 600, K = 2 so that they fit): n_cap = 1030 puts every system of the launch
    on four wavefronts."""
    orc, big_pos, big_sigma = _oracle(1030, L=600, site_capacity=2, local_kernel_sigma=0.02, rate_diffusion=0.5, rate_active=4.0, beta=1.1)
    _, pos0, sigma0 = _oracle(400, L=600, site_capacity=2, local_kernel_sigma=0.02, rate_diffusion=0.5, rate_active=4.0, beta=1.1)
    T = 0.8
    kw = dict(sigma_grids=[0.02 * 600, 0.1 * 600], variant_of_system=[0, 0, 1, 0], betas=[orc.par.beta] * 4,
              states=[(pos0, sigma0), (pos0, sigma0), (big_pos, big_sigma), (pos0, sigma0)], times_obs=np.arange(0.0, T, 0.05), T=T,
              seeds=MIXED_KEYS, streams=MIXED_STREAMS, **_raw(orc, sigma=False))
    assert gil.plan_mixed(L=600, K=2, periodic=False, sigma_grids=kw["sigma_grids"], n_systems=4, n_cap=1030, n_obs=len(kw["times_obs"]),
                          variant_of_system=kw["variant_of_system"])["threads"] == 256
    seeded = gil.run_mixed_raw(**kw)
    tables = _tables([ps.mixed_stream(MIXED_KEYS, MIXED_STREAMS, s) for s in range(4)], seeded["n_events"], 256)
    _pin(seeded, gil.run_mixed_raw(uniforms=tables, **kw), tables, 256, 2 * 256, "mixed256")
    _differ_pairwise(seeded, [0, 1, 3], "mixed256")


# ---- the public face

PUBLIC = dict(L=300, xlim=1.0, rate_diffusion=0.4, rate_active=4.0, beta=1.0, init="fixed", N=140, scale_rates=False,
              local_kernel_sigma=0.02, site_capacity=2, k_on=0.0, k_off=0.0, k_exit=0.0, mode="gillespie_gpu")


def _public_raw(ps_):
    return dict(L=ps_.L, K=ps_.K, periodic=ps_.periodic, sigma_grid=ps_._sigma_grid, rate_diffusion=ps_.rate_diffusion,
                rate_active=ps_.rate_active, minus_anchor=ps_.minus_anchor, immobilize=ps_.immobilize_when_anchored,
                suppress_flip=ps_.suppress_flip_when_bound, crowding=ps_.crowding_suppresses_rates, k_on=ps_.k_on, k_off=ps_.k_off,
                k_exit=ps_.k_exit, anchor_mask=ps_.is_anchor_site, flip_table=ps_.flip_table())


def _same_pos_lists(out, r, s, n0):
    n_rec = int(r["n_recorded"][s])
    assert n_rec > 1 and all(p is None for p in out["pos_list"][n_rec:])
    for k in range(n_rec):
        live = (r["flags"][s, k, :n0] & 2) != 0
        assert np.array_equal(out["pos_list"][k], r["pos"][s, k, :n0][live].astype(np.int64)), (s, k)


def test_particle_system_run_draws_key_seed_stream_zero(gil):
    from PARTICLE_solver_CLASS import ParticleSystem
    T, obs_dt = 1.0, 0.1
    system = ParticleSystem(rng=np.random.default_rng(3), seed=KEY, **PUBLIC)
    out = system.run(T=T, obs_dt=obs_dt)
    twin = ParticleSystem(rng=np.random.default_rng(3), seed=KEY, **PUBLIC)      # the same seeded rng: the same initial state
    state = twin.init_particles()
    table = _tables([ps.batch_stream(KEY, 0)], [system.n_events], 64)
    assert 3 * 64 < system.n_events <= table.shape[1] - 64
    r = gil.run_raw(betas=[twin.beta], states=[state], times_obs=np.arange(0.0, T, obs_dt), T=T, uniforms=table, **_public_raw(twin))
    assert int(r["n_events"][0]) == system.n_events
    _same_pos_lists(out, r, 0, len(state[0]))


def test_run_batched_exact_draws_key_of_the_first_system_stream_j(gil):
    from PARTICLE_solver_CLASS import ParticleSystem
    T, obs_dt = 1.0, 0.1
    make = lambda: [ParticleSystem(rng=np.random.default_rng(3), seed=KEY if j == 0 else 1000 + j, **PUBLIC) for j in range(3)]   # noqa: E731
    systems = make()
    outs = gil.run_batched_exact(systems, T=T, obs_dt=obs_dt)
    states = [twin.init_particles() for twin in make()]
    assert all(np.array_equal(states[0][0], st[0]) and np.array_equal(states[0][1], st[1]) for st in states[1:])
    n_events = [s_.n_events for s_ in systems]
    tables = _tables([ps.batch_stream(KEY, j) for j in range(3)], n_events, 64)
    assert min(n_events) > 3 * 64 and max(n_events) <= tables.shape[1] - 64
    twin = make()[0]
    r = gil.run_raw(betas=[twin.beta] * 3, states=states, times_obs=np.arange(0.0, T, obs_dt), T=T, uniforms=tables, **_public_raw(twin))
    assert r["n_events"].tolist() == n_events
    for j in range(3):
        _same_pos_lists(outs[j], r, j, len(states[j][0]))
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert not np.array_equal(outs[a]["pos_list"][-1], outs[b]["pos_list"][-1])
