"""CPU suite: the restatements of tests/observable_reference.py are what they claim to be, on three tiny states (L = 7, 64, 97,
K up to 3, some particles dead, some away): structure_sums against np.fft.fft of the site histogram, scalar_sums and bin_sums
against loops over particles that share no code with them."""
import math

import numpy as np
import pytest

import observable_reference as R

CASES = [dict(L=7, K=1, N=5, seed=1), dict(L=64, K=3, N=120, seed=2), dict(L=97, K=2, N=150, seed=3)]


def state(case):
    rng = np.random.default_rng(case["seed"])
    L, K, N = case["L"], case["K"], case["N"]
    pos = rng.permutation(rng.choice(np.repeat(np.arange(L), K), size=N, replace=False)).astype(np.int32)
    spin = rng.choice(np.array([1, -1], np.int8), size=N)
    alive = rng.choice(np.array([1, 1, 1, 0, 2], np.uint8), size=N)
    ref_pos = rng.integers(0, L, size=N).astype(np.int32)
    ref_alive = rng.choice(np.array([1, 1, 0], np.uint8), size=N)
    assert (alive == 0).any() and (alive == 1).any() and (ref_alive == 0).any()
    return pos, spin, alive, ref_pos, ref_alive


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"L{c['L']}")
def test_structure_sums_against_fft(case):
    pos, spin, alive, _, _ = state(case)
    L = case["L"]
    m = np.random.default_rng(9).uniform(-1.0, 1.0, L)
    n, c2, m1, m2, F = R.structure_sums(pos, alive, L, L, m)
    count = np.bincount(pos[alive == 1], minlength=L)
    fft = np.fft.fft(count)
    err = max(np.max(np.abs(F[:, 0].astype(float) - fft.real)), np.max(np.abs(F[:, 1].astype(float) - fft.imag)))
    print("L", L, "largest difference from np.fft.fft", err)
    assert err <= 1e-12
    assert isinstance(n, int) and isinstance(c2, int) and n == int((alive == 1).sum()) and c2 == sum(int(c) ** 2 for c in count)
    assert m1 == math.fsum(m.tolist()) and m2 == math.fsum([x * x for x in m.tolist()])
    assert F[0, 0] == n and F[0, 1] == 0
    n0, c20, z1, z2, F0 = R.structure_sums(pos, np.zeros_like(alive), L, 3)          # nothing alive, no field
    assert (n0, c20, z1, z2) == (0, 0, 0.0, 0.0) and not F0.any()


@pytest.mark.parametrize("table", ["any", "zero", "random"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"L{c['L']}")
def test_scalar_sums_against_a_double_loop(case, table):
    pos, spin, alive, ref_pos, ref_alive = state(case)
    L, K, N = case["L"], case["K"], case["N"]
    tab = {"any": None, "zero": np.zeros((K + 1) ** 2, np.uint8),
           "random": np.random.default_rng(5).integers(0, 2, (K + 1) ** 2).astype(np.uint8)}[table]
    x_wall, lo, hi = L // 2, L // 5, L - 3
    want = dict.fromkeys(R.SCALARS, 0)
    want["max_pos"] = -1
    for i in range(N):
        if alive[i] != 1:
            continue
        p = int(pos[i])
        want["n"] += 1
        want["sum_sigma"] += int(spin[i])
        want["sum_pos"] += p
        want["n_wall"] += p >= x_wall
        want["max_pos"] = max(want["max_pos"], p)
        want["n_range"] += lo <= p <= hi
        if spin[i] > 0 and p < L - 1:
            plus = minus = 0
            for j in range(N):                                # the right neighbour site's occupancy, particle by particle
                if alive[j] == 1 and pos[j] == p + 1:
                    plus, minus = plus + (spin[j] > 0), minus + (spin[j] < 0)
            want["attempts"] += 1
            want["blocked"] += int(plus + minus >= 1) if tab is None else int(tab[plus * (K + 1) + minus])
        if ref_alive[i] == 1:
            d = p - int(ref_pos[i])
            want["sum_d"] += d
            want["sum_d2"] += d * d
            want["n_d"] += 1
    got = R.scalar_sums(pos, spin, alive, ref_pos, ref_alive, L, K, x_wall, lo, hi, tab)
    assert got == want and all(isinstance(v, int) for v in got.values())
    assert want["attempts"] > 0 and want["n_d"] > 0
    none = R.scalar_sums(pos, spin, alive, None, None, L, K, x_wall, lo, hi, tab)
    assert none == dict(want, sum_d=0, sum_d2=0, n_d=0)
    dead = R.scalar_sums(pos, spin, np.zeros_like(alive), ref_pos, ref_alive, L, K, x_wall, lo, hi, tab)
    assert dead == dict(dict.fromkeys(R.SCALARS, 0), max_pos=-1)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"L{c['L']}")
def test_bin_sums_against_a_loop(case):
    pos, spin, alive, _, _ = state(case)
    L = case["L"]
    for nbins in (1, 2, 5, L - 1, L):
        width = (L + nbins - 1) // nbins
        plus, minus = [0] * nbins, [0] * nbins
        for i in range(len(pos)):
            if alive[i] == 1:
                (plus if spin[i] > 0 else minus)[int(pos[i]) // width] += 1
        got = R.bin_sums(pos, spin, alive, L, nbins)
        assert got[0].tolist() == plus and got[1].tolist() == minus
        assert sum(plus) + sum(minus) == int((alive == 1).sum())
        if nbins * width - L >= width:                        # the rule leaves bins without a site: they stay 0
            empty = range(-(-L // width), nbins)
            assert len(empty) > 0 and all(plus[b] == 0 and minus[b] == 0 for b in empty)
    assert any((L + nb - 1) // nb * nb - L >= (L + nb - 1) // nb for nb in (1, 2, 5, L - 1, L))
