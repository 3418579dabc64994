"""CPU suite: oracle/philox_streams.py -- the NumPy restatement of the random streams the device's exact event loop and the PDE
tracers draw (layouts: include/gillespie.h, include/gillespie_many.h, include/gillespie_mixed.h, include/pde.h) -- against the
oracle's C Philox and the Random123 known answers, and the properties of the layout that no GPU run can look at: the ends of
the 53-bit conversion, which word feeds which number, the high half of the event index, the carry of seed + s."""
import numpy as np

from oracle import philox_streams as ps
from oracle import sync_oracle as so
from test_oracle_sync import PHILOX_KAT

KEY = 0x9E3779B97F4A7C15


def test_numpy_philox_equals_the_known_answers_and_the_c_oracle():
    for ctr, key, want in PHILOX_KAT:
        assert tuple(int(x) for x in ps.philox4x32_10(*ctr, *key)) == want
    rng = np.random.default_rng(2024)
    ctr = rng.integers(0, 2 ** 32, size=(300, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, size=(300, 2), dtype=np.uint64)
    ctr[:8], key[:8] = [[0, 0, 0, 0], [0xFFFFFFFF] * 4] * 4, [[0, 0xFFFFFFFF], [0xFFFFFFFF, 0]] * 4    # carries of the key schedule
    got = ps.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], key[:, 0], key[:, 1])
    assert got.shape == (300, 4) and got.dtype == np.uint32
    want = np.stack([so.philox4x32_10(c, k) for c, k in zip(ctr, key)])
    assert np.array_equal(got, want)
    # broadcasting: scalars against a vector
    one = ps.philox4x32_10(ctr[:, 0], 7, 9, ps.EXACT_LOOP_DOMAIN_A, 11, 13)
    assert np.array_equal(one[5], so.philox4x32_10([ctr[5, 0], 7, 9, ps.EXACT_LOOP_DOMAIN_A], [11, 13]))


def test_uniform53_ends_and_grid():
    top = float(ps.uniform53(0xFFFFFFFF, 0xFFFFFFFF))
    assert top < 1.0 and top == 1.0 - 2.0 ** -53
    assert np.isfinite(-np.log1p(-top)) and -np.log1p(-top) > 36.0          # the longest waiting time the loop can draw
    assert float(ps.uniform53(0, 0)) == 0.0 and -np.log1p(-0.0) == 0.0
    assert float(ps.uniform53(0, 1 << 6)) == 2.0 ** -53                      # one step of the grid: 53 bits, not 52
    assert float(ps.uniform53(1 << 5, 0)) == 2.0 ** -27
    assert float(ps.uniform53(31, 63)) == 0.0                                # the low 5 and 6 bits are dropped
    rng = np.random.default_rng(1)
    a, b = rng.integers(0, 2 ** 32, size=(2, 1000), dtype=np.uint64)
    u = ps.uniform53(a, b)
    assert np.array_equal(u * 2.0 ** 53, np.floor(u * 2.0 ** 53)) and u.min() >= 0.0 and u.max() < 1.0
    assert np.any((u * 2.0 ** 53) % 2 == 1)                                  # odd multiples of 2^-53 occur


def test_each_word_feeds_exactly_one_column():
    w = ps.exact_loop_words(KEY, 3, 50)
    assert w.shape == (50, 8) and w.dtype == np.uint32
    base = ps.uniforms_from_words(w)
    assert np.array_equal(base, ps.exact_loop_uniforms(KEY, 3, 50))
    for j in range(8):
        v = w.copy()
        v[:, j] ^= np.uint32(0x80000000)
        changed = ps.uniforms_from_words(v) != base
        assert changed[:, j // 2].all() and not np.delete(changed, j // 2, axis=1).any(), j
    # the two blocks of an event are the two domain constants on the same counter and key
    k0, k1 = ps.split_key(KEY)
    assert (k0, k1) == (0x7F4A7C15, 0x9E3779B9)
    assert np.array_equal(w[17, :4], so.philox4x32_10([17, 0, 3, 0x47494C31], [k0, k1]))
    assert np.array_equal(w[17, 4:], so.philox4x32_10([17, 0, 3, 0x47494C32], [k0, k1]))
    # no two of the four numbers of an event coincide, and systems on different streams or keys draw different tables
    assert all(len(set(row)) == 4 for row in base)
    assert not np.any(ps.exact_loop_uniforms(KEY, 4, 50) == base)
    assert not np.any(ps.exact_loop_uniforms(KEY & 0xFFFFFFFF, 3, 50) == base)       # the key's high word counts
    assert not np.any(ps.exact_loop_uniforms(KEY ^ 1, 3, 50) == base)


def test_event_index_carries_into_counter_word_one():
    k0, k1 = ps.split_key(KEY)
    w = ps.exact_loop_words(KEY, 2, 2, first_event=2 ** 32 - 1)
    assert np.array_equal(w[0, :4], so.philox4x32_10([0xFFFFFFFF, 0, 2, 0x47494C31], [k0, k1]))
    assert np.array_equal(w[1, :4], so.philox4x32_10([0, 1, 2, 0x47494C31], [k0, k1]))
    assert np.array_equal(w[1, 4:], so.philox4x32_10([0, 1, 2, 0x47494C32], [k0, k1]))
    assert not np.array_equal(w[1], ps.exact_loop_words(KEY, 2, 1)[0])        # event 2^32 is not event 0 again
    assert np.array_equal(ps.exact_loop_uniforms(KEY, 2, 3, first_event=2 ** 32 - 2)[1:], ps.uniforms_from_words(w))


def test_many_large_key_carries_and_wraps():
    got = [ps.many_large_stream(2 ** 32 - 2, s) for s in range(3)]
    assert got == [(0xFFFFFFFE, 0), (0xFFFFFFFF, 0), (0x100000000, 0)]
    assert [ps.split_key(k) for k, _ in got] == [(0xFFFFFFFE, 0), (0xFFFFFFFF, 0), (0, 1)]      # carry into the high word
    got = [ps.many_large_stream(2 ** 64 - 2, s) for s in range(3)]
    assert got == [(2 ** 64 - 2, 0), (2 ** 64 - 1, 0), (0, 0)]                                  # wrap to 0
    assert [ps.split_key(k) for k, _ in got] == [(0xFFFFFFFE, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF), (0, 0)]
    tables = [ps.exact_loop_uniforms(*ps.many_large_stream(2 ** 32 - 2, s), 20) for s in range(3)]
    assert not np.any(tables[2] == ps.exact_loop_uniforms(0, 0, 20))         # a dropped carry would give key 0
    assert not np.any(tables[0] == tables[1]) and not np.any(tables[1] == tables[2])
    assert ps.batch_stream(KEY, 5) == (KEY, 5) and ps.large_stream(KEY) == (KEY, 0)
    assert ps.mixed_stream([1, KEY, 3], [5, 0, 7], 1) == (KEY, 0)


def test_pde_tracer_noise_layout():
    k0, k1 = ps.split_key(KEY)
    u, g = ps.pde_tracer_noise(KEY, 1, 40, 70)
    assert u.shape == g.shape == (41, 70) and u.dtype == g.dtype == np.float64
    for n, i in ((0, 0), (40, 69), (13, 64)):
        x = so.philox4x32_10([n, i, 1, 0x7AC3], [k0, k1]).astype(np.float64)
        assert u[n, i] == float(ps.uniform53(int(x[0]), int(x[1])))
        want = np.sqrt(-2.0 * np.log((x[2] + 0.5) * 2.0 ** -32)) * np.cos(2.0 * np.pi * (x[3] + 0.5) * 2.0 ** -32)
        assert g[n, i] == want
    assert np.all(np.isfinite(g)) and u.min() >= 0.0 and u.max() < 1.0
    # x2 = 0 is the largest radius Box-Muller can give here; it is finite
    assert np.isfinite(np.sqrt(-2.0 * np.log(0.5 * 2.0 ** -32)))
    u2, g2 = ps.pde_tracer_noise(KEY, 0, 40, 70)
    assert not np.any(u2 == u) and not np.any(g2 == g)
