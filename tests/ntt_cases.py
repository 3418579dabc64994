"""Cases for the oracle parity of the exact convolution at every transform size and edge (csrc/ntt_conv.hpp, ntt_setup in
csrc/aps_hip.hip).  tests/test_ntt_cases_cpu.py checks the list itself on the CPU (a census: which transform every case runs),
tests/test_gpu_convolution_sizes.py runs it on the device.  A helper module, not a test.

Which kernels a handle launches is decided by log2_m (the smallest m with 2^m >= L + 2 reach), the field's width (one prime for
the 32-bit field, two for binary64) and APS_NTT_FUSED: ntt_strided<AXIS, INV, A, NP> is a separate compilation for every radix
A = a2 = m - 14 of the i2 sweeps, m = 14 has no i2 sweep at all, ntt_mid shifts by the run-time a2.  The one-block cases of the
rest of the suite run m = 15, 17, 18 and 21 only.  THE LIST IS PART OF THIS FILE'S BEHAVIOUR: every one-block size 14 .. 21 (32-bit)
and 15 .. 21 (binary64), each from 15 on fused and with APS_NTT_FUSED=0, between walls and on a torus, plus the edges
    fit         L + 2 reach = 2^m exactly (the circular convolution has not one spare word), and one site more (plans m + 1),
    ring        an even ring with a ring-wide table (2 reach = L: the tap at distance L / 2 counts once) beside an odd one,
    edge        the largest reach ntt_setup admits between walls for its L, and the next one up, which must keep the sweep,
    two ensembles of the binary64 field (grid z = prime * E + ensemble), with anchors, binding and exits.
Another size, sigma or particle number is another set of checks and is reviewed as such; the census fails when a change of the
table builder or of the plan rule moves a case to another transform.

tools/dev/fuzz_convolution.py is the development-time companion: it draws random lattices with L from 9000 .. 40000 (m <= 17)
and compares convolution and sweep on whatever device is at hand.  It finds what nobody thought of at small sizes; it is not
part of the suite and reaches none of m = 18 .. 21.  This list is the deterministic part: every compilation, every run.

A case is a plain dictionary:
    tag, L, K, sigma, periodic, fp32 (field width), betas (one per ensemble), N (particles per ensemble), blocks (steps per call:
    (1, 2, 37) covers single steps and graph replay; m >= 19 keeps (1, 2)), fused (the APS_NTT_FUSED values to run), log2_m (the
    transform it is meant to hit; None: ntt_setup must refuse it), extra (further LatticeGasParams keywords), seed, dt.
Particles sit on site 0, on site L - 1, in clusters within the reach of both walls (torus: across the seam) and in the interior.

Reference.  The trajectory comes from oracle.sync_oracle.SyncOracle (N x taps per step).  Its field_sites() over ALL sites costs
L x taps (58 s at L = 300 000 with a reach of 105 000), so {W, S, occupancy} on all sites come from `scatter_field`: for every
particle the table is added at its site +- reach on the extended lattice [-reach, L + reach), then the margins are folded back --
between walls onto the mirror sites (-1 - y and 2 L - 1 - y), on a torus modulo L, where an even ring with a ring-wide table drops
the -L / 2 tap.  Every weight sits on the grid 2^-q and the sums stay far below 2^53 grid units, so the binary64 sums are exact
whatever their order.  The CPU test pins it to field_sites() on all sites of small lattices and to the window stencil of
tests/test_gpu_parity.py on one large case.  `reference(case)` is computed once per case and shared by its fused and unfused runs;
nobody writes into it.

CPU seconds of reference(case) -- the oracle's trajectory plus a scatter after set_state and after every block --, measured on one
core where the list was written (tests/test_ntt_cases_cpu.py prints them):
    walls m14, m15 exact fit, m16 one past the fit    0.6 each         torus m16                        0.9
    walls m17 edge reach and its neighbour            1.5 each         ring-wide tori, m17 and m18      0.2 each
    walls m19   4.7      walls m20   4.1      walls m21   4.7          two ensembles, m15               0.7
about 35 s for the whole list, both field widths.
"""
import functools

import numpy as np

from oracle.gillespie_numpy import LatticeGasParams
from oracle import sync_oracle as so

SMALL_BLOCKS = (1, 2, 37)                 # single steps and graph replay
LARGE_BLOCKS = (1, 2)                     # m >= 19: the oracle costs N x taps per step
BOTH = ("1", "0")
# tile terms of the walls rule  2 reach + frame + own + 4 < L  (frame = 64 RS <= 512 sites, own <= 64 RS - 4): a bound for every geometry
TILE_TERMS_MAX = 512 + 508
# ... and the ones ts_choose_geometry takes at L = 40000 with one ensemble (614 workgroups wanted, 667 tiles of 60 sites are closest):
# the edge cases are cut to them; the device test reads them back from tiles_info()
EDGE_FRAME, EDGE_OWN = 64, 60
NTT_P0, NTT_P1 = 2013265921, 1811939329
ANCHORS = dict(anchor_positions=[0.3, 0.7], anchor_radius=0.02, k_on=2.0, k_off=1.0, k_exit=0.8)


def _case(tag, L, K, sigma, periodic, fp32, log2_m, N, blocks=SMALL_BLOCKS, fused=BOTH, betas=(1.1,), extra=None, seed=7, dt=0.05):
    return dict(tag=tag + ("_i32" if fp32 else "_f64"), L=L, K=K, sigma=sigma, periodic=periodic, fp32=fp32, log2_m=log2_m, N=N, blocks=blocks,
                fused=fused, betas=tuple(betas), extra=dict(extra or {}), seed=seed, dt=dt)


def _both_widths(tag, L, K, sigma, periodic, log2_m, N, **kw):
    return [_case(tag, L, K, sigma, periodic, True, log2_m, N, **kw), _case(tag, L, K, sigma, periodic, False, log2_m, N, **kw)]


@functools.lru_cache(maxsize=None)
def all_cases():
    c = []
    # m = 14: two sweeps, no i2 sweep (a2 = 0) -- one block, so the first sweep clears the coefficients (32-bit field only)
    c += [_case("walls_m14_two_sweeps", 12000, 2, 0.04, False, True, 14, 2500, fused=("1",))]
    # m = 15: the signal fills the transform exactly (28248 + 2 * 2260 = 2^15); one site more plans m = 16
    c += _both_widths("walls_m15_exact_fit", 28248, 2, 0.02, False, 15, 2500)
    c += _both_widths("walls_m16_one_past_fit", 28249, 2, 0.02, False, 16, 2500)
    c += [_case("torus_m16", 50000, 2, 0.03, True, True, 16, 2500, fused=("1",), seed=17),
          _case("torus_m16", 50000, 2, 0.015, True, False, 16, 2500, fused=("0",), seed=17)]
    # m = 17: the largest reach the walls rule admits at L = 40000 (2 * 19935 + 64 + 60 + 4 = 39998 < L) ...
    c += _both_widths("walls_m17_edge_reach", 40000, 2, 0.124593, False, 17, 900)
    # ... and one site of reach more: not eligible, the sweep runs and must match all the same
    c += [_case("walls_edge_reach_plus_one_sweeps", 40000, 2, 0.124599, False, True, None, 900, fused=("1",))]
    # m = 17 on an even ring with a ring-wide table: 2 reach = L = 65536 fills 2^17 exactly, the half-ring tap counts once
    c += _both_widths("torus_m17_even_ring_wide", 65536, 2, 0.3, True, 17, 600, seed=17)
    # m = 18: the odd ring beside it (every distance up to (L - 1) / 2; 65537 + 65536 is one word past 2^17)
    c += _both_widths("torus_m18_odd_ring_wide", 65537, 2, 0.3, True, 18, 600, seed=17)
    # m = 19 .. 21 between walls
    c += _both_widths("walls_m19", 300000, 1, 0.07, False, 19, 3000, blocks=LARGE_BLOCKS)
    c += _both_widths("walls_m20", 600000, 2, 0.05, False, 20, 2000, blocks=LARGE_BLOCKS)
    c += _both_widths("walls_m21", 1300000, 2, 0.05, False, 21, 1000, blocks=LARGE_BLOCKS)
    # two ensembles of the binary64 field: grid z = prime * E + ensemble; anchors, binding, exits
    c += [_case("walls_m15_two_ensembles", 20000, 2, 0.02, False, False, 15, 3000, betas=(0.4, 2.2), extra=ANCHORS, seed=12, dt=0.04)]
    return tuple(c)


def by_tag(tag):
    (case,) = [c for c in all_cases() if c["tag"] == tag]
    return case


def runs():
    """(case, APS_NTT_FUSED value) for every handle the device test creates."""
    return [(c, f) for c in all_cases() for f in c["fused"]]


def params(case, beta=None):
    base = dict(xlim=1.0, rate_diffusion=3.0, rate_active=4.0, beta=case["betas"][0] if beta is None else beta, scale_rates=False)
    base.update(case["extra"])
    return LatticeGasParams.from_kwargs(L=case["L"], local_kernel_sigma=case["sigma"], periodic=case["periodic"], site_capacity=case["K"], **base)


_TABLES = {}


def table(case):
    """(weight table, q) the oracle builds for the case's field width; read-only."""
    key = (case["L"], case["K"], case["sigma"], case["periodic"], case["fp32"])
    if key not in _TABLES:
        tab, q = so.build_table(params(case).sigma_grid, case["L"], case["K"], bool(case["periodic"]), 29 if case["fp32"] else 51)
        tab.setflags(write=False)
        _TABLES[key] = (tab, q)
    return _TABLES[key]


def reach(case):
    return len(table(case)[0]) - 1


def primes(case):
    return 1 if case["fp32"] else 2


def eligible(case, frame_sites=None, owned_sites=None):
    """ntt_setup's rules for a single handle, restated: (taken, reason).  Between walls the tile terms are a bound for every
    geometry unless the caller knows them (tiles_info() of a handle, or EDGE_FRAME / EDGE_OWN for the edge cases)."""
    L, Rt, K = case["L"], reach(case), case["K"]
    tab, q = table(case)
    if case["periodic"]:
        if not 2 * Rt <= L:
            return False, "torus: table beyond half the ring"
    else:
        tiles = TILE_TERMS_MAX if frame_sites is None else frame_sites + owned_sites
        if not 2 * Rt + tiles + 4 < L:
            return False, "walls: 2 reach + frame + own + 4 >= L"
    if 4 * Rt > (1 << 21) or L + 2 * Rt > (1 << 21):
        return False, "more than one block"
    wsum = float(np.sum(np.ldexp(tab, q)) * 2.0 - np.ldexp(tab[0], q))           # grid units: integers, exact
    modulus = float(NTT_P0) if case["fp32"] else float(NTT_P0) * float(NTT_P1)
    if not 2.0 * K * wsum < 0.5 * modulus:
        return False, "exactness: 2 K sum w 2^q reaches half the modulus"
    return True, "taken"


def expected_launches(log2_m, fused):
    """m = 14 has two strided sweeps and the contiguous one; from 15 on ntt_mid makes three, APS_NTT_FUSED=0 keeps five."""
    return 3 if log2_m == 14 or fused == "1" else 5


def search_exact_fit(m, fp32, sigma=0.02, K=2):
    """The lattice between walls whose L + 2 reach(L) is 2^m exactly (the reach depends on L); None: there is none."""
    probe = dict(K=K, sigma=sigma, periodic=False, fp32=fp32, extra={}, betas=(1.1,))
    for L in range(int((1 << m) / (1.0 + 8.0 * sigma)) - 64, int((1 << m) / (1.0 + 8.0 * sigma)) + 64):
        if L + 2 * reach(dict(probe, L=L)) == (1 << m):
            return L
    return None


def initial_state(case, ensemble=0):
    """Site 0, site L - 1, a cluster inside the reach of either wall (torus: the two together straddle the seam), one in the
    interior, a thin background; at most K per site, N particles, shuffled."""
    L, K, N, Rt = case["L"], case["K"], case["N"], reach(case)
    rng = np.random.default_rng(1000 * case["seed"] + ensemble)
    near = max(8, min(Rt // 2, 400))                              # well inside the reach of the wall
    n_cl = N // 5
    parts = [np.array([0, L - 1]), rng.integers(0, near, n_cl), rng.integers(L - near, L, n_cl), rng.integers(L // 3, L // 3 + 2 * near, n_cl)]
    u, cnt = np.unique(np.concatenate(parts), return_counts=True)
    keep = np.repeat(u, np.minimum(cnt, K))
    slots = np.repeat(np.arange(L), K - np.bincount(keep, minlength=L))
    fill = rng.choice(slots, size=N - len(keep), replace=False)
    pos = rng.permutation(np.concatenate([keep, fill])).astype(np.int32)
    spin = rng.choice(np.array([1, -1], np.int8), size=N)
    return pos, spin


def scatter_field(tab, pos, spin, alive, L, periodic):
    """{W, S, occupancy} on all sites by adding the table around every live particle: N x taps additions, exact in binary64."""
    tab = np.asarray(tab, dtype=np.float64)
    Rt = len(tab) - 1
    live = np.asarray(alive).astype(bool)
    pos, spin = np.asarray(pos, dtype=np.int64)[live], np.asarray(spin, dtype=np.float64)[live]
    wsym = np.concatenate([tab[::-1], tab[1:]])                   # taps -Rt .. +Rt
    if periodic and 2 * Rt == L:
        wsym[0] = 0.0                                             # even ring, ring-wide table: the half-ring tap counts once (+L / 2 is kept)
    occ = np.bincount(pos, minlength=L)
    sites = np.flatnonzero(occ)                                   # every occupied site once, with its deposits c_W and c_S
    c_w = occ[sites].astype(np.float64)
    c_s = np.bincount(pos, weights=spin, minlength=L)[sites]
    ext = np.zeros((2, L + 2 * Rt))                               # extended lattice: index = site + Rt
    for x, a, b in zip(sites, c_w, c_s):
        ext[0, x:x + 2 * Rt + 1] += a * wsym
        if b:
            ext[1, x:x + 2 * Rt + 1] += b * wsym
    out = ext[:, Rt:Rt + L].copy()
    if Rt:
        left, right = ext[:, :Rt], ext[:, Rt + L:]                # sites -Rt .. -1 and L .. L + Rt - 1
        if periodic:
            assert 2 * Rt <= L
            out[:, L - Rt:] += left                               # site y - L is site y
            out[:, :Rt] += right
        else:
            assert Rt <= L
            out[:, :Rt] += left[:, ::-1]                          # site -1 - y mirrors y
            out[:, L - Rt:] += right[:, ::-1]                     # site 2 L - 1 - y mirrors y
    return out[0], out[1], occ.astype(np.int32)


def snapshot(orc, tab, field=True):
    snap = dict(pos=orc.pos.copy(), spin=orc.spin.copy(), bound=orc.bound.copy(), alive=orc.alive.copy(), exits=np.array(orc.exits(), copy=True))
    if field:
        snap["W"], snap["S"], snap["occ"] = scatter_field(tab, orc.pos, orc.spin, orc.alive, orc.par.L, bool(orc.par.periodic))
    for v in snap.values():
        v.setflags(write=False)
    return snap


_REFERENCE = {}


def reference(case):
    """dict(table, q, start, ens): per ensemble the initial state and the oracle's snapshots after set_state and after every block
    of steps, each with {W, S, occupancy} on all sites by scatter_field.  Computed once per case; read-only."""
    if case["tag"] not in _REFERENCE:
        tab, q = table(case)
        ens = []
        for e, beta in enumerate(case["betas"]):
            orc = so.SyncOracle(params(case, beta), dt=case["dt"], seed=case["seed"], ensemble=e, **(dict(sum_bits=29) if case["fp32"] else {}))
            assert orc.q == q and np.array_equal(orc.table, tab)
            pos, spin = initial_state(case, e)
            orc.set_state(pos, spin)
            snaps = [snapshot(orc, tab)]
            for n in case["blocks"]:
                orc.run(n)
                snaps.append(snapshot(orc, tab))
            ens.append(dict(pos=pos, spin=spin, snaps=snaps))
        _REFERENCE[case["tag"]] = dict(table=tab, q=q, ens=ens)
    return _REFERENCE[case["tag"]]

