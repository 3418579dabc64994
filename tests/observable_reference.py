"""Plain restatements of the device observables of the fixed-dt stepper (include/aps.h: aps_observe_scalars, aps_observe_bins,
aps_observe_structure), for tests/test_gpu_observables.py; tests/test_observable_reference_cpu.py checks them on the CPU.
A helper module, not a test: NumPy and Python integers only, no device code, no import of the package.

Every function takes a state as aps_get_state returns it (`alive`: 1 live and own, 0 dead, 2 on another rank's sites; only 1
counts) and returns Python integers wherever the device sum is an integer, so nothing here can overflow or round."""
import math

import numpy as np

SCALARS = ("n", "sum_sigma", "sum_pos", "n_wall", "max_pos", "n_range", "attempts", "blocked", "sum_d", "sum_d2", "n_d")
_TWO_PI = np.longdouble(8) * np.arctan(np.longdouble(1))


def _live(alive):
    return np.asarray(alive) == 1


def site_counts(pos, spin, alive, L):
    """(plus, minus) live particles per site."""
    pos, spin, live = np.asarray(pos, np.int64), np.asarray(spin), _live(alive)
    return np.bincount(pos[live & (spin > 0)], minlength=L), np.bincount(pos[live & (spin < 0)], minlength=L)


def scalar_sums(pos, spin, alive, ref_pos, ref_alive, L, K, x_wall, lo, hi, block_table=None):
    """The eleven entries of out11, by name.  ref_pos = None: no reference marked (the three displacement sums are 0);
    else d = pos - ref_pos over the particles alive now AND at mark time, not unwrapped on a torus.
    block_table[(K + 1) * (K + 1)] is indexed [plus * (K + 1) + minus] of the right neighbour site; None: any particle blocks."""
    pos, spin, live = np.asarray(pos, np.int64), np.asarray(spin, np.int64), _live(alive)
    if block_table is None:
        table = np.array([[1 if cp + cm >= 1 else 0 for cm in range(K + 1)] for cp in range(K + 1)])
    else:
        table = np.asarray(block_table, np.int64).reshape(K + 1, K + 1)
    cp, cm = site_counts(pos, spin, alive, L)
    p, s = pos[live], spin[live]
    movers = p[(s > 0) & (p < L - 1)]
    out = dict(n=len(p), sum_sigma=sum(map(int, s)), sum_pos=sum(map(int, p)), n_wall=int(np.count_nonzero(p >= x_wall)),
               max_pos=int(p.max()) if len(p) else -1, n_range=int(np.count_nonzero((p >= lo) & (p <= hi))),
               attempts=len(movers), blocked=sum(int(table[cp[x + 1], cm[x + 1]]) for x in movers), sum_d=0, sum_d2=0, n_d=0)
    if ref_pos is not None:
        both = live & _live(ref_alive)
        d = [int(a) - int(b) for a, b in zip(pos[both], np.asarray(ref_pos, np.int64)[both])]
        out.update(sum_d=sum(d), sum_d2=sum(x * x for x in d), n_d=len(d))
    return out


def bin_sums(pos, spin, alive, L, nbins):
    """(plus, minus) live particles per bin of ceil(L / nbins) consecutive sites; bins that hold no site are 0."""
    width = -(-L // nbins)
    cp, cm = site_counts(pos, spin, alive, L)
    plus, minus = np.zeros(nbins, np.int64), np.zeros(nbins, np.int64)
    for b in range(nbins):
        plus[b], minus[b] = cp[b * width:(b + 1) * width].sum(), cm[b * width:(b + 1) * width].sum()
    return plus, minus


def structure_sums(pos, alive, L, k_max, m_field=None):
    """(n, sum over sites of count^2, fsum(m), fsum(m * m), F) with F[k] = (sum cos, -sum sin) of 2 pi ((k pos) mod L) / L over
    the live particles, k = 0 .. k_max - 1: the reduction mod L in Python integers, trigonometry and sums in np.longdouble.
    m * m is the binary64 product, as the kernel forms it; the two sums over m are correctly rounded (math.fsum)."""
    pos = np.asarray(pos, np.int64)[_live(alive)]
    count = np.bincount(pos, minlength=L)
    sites = [int(x) for x in np.flatnonzero(count)]
    weight = count[sites].astype(np.longdouble)
    F = np.zeros((k_max, 2), np.longdouble)
    for k in range(k_max):
        angle = _TWO_PI * np.array([(k * x) % L for x in sites], np.longdouble) / np.longdouble(L)
        F[k, 0], F[k, 1] = np.sum(weight * np.cos(angle)), -np.sum(weight * np.sin(angle))
    m = np.zeros(L) if m_field is None else np.asarray(m_field, np.float64)
    return len(pos), sum(int(c) * int(c) for c in count[sites]), math.fsum(m), math.fsum(m * m), F
