"""Cases for the parity of the fixed-dt stepper at EVERY frame size of its kernels (tests/test_sync_cases_cpu.py checks the table
itself on the CPU, tests/test_gpu_sync_frames.py runs it through every device path).  A helper module, not a test.

The step kernels are templates over the frame height RS (a frame is 64 RS sites, a tile owns 64 RS - 4 of them): tile_step,
tile_loop with four and with eight waves, field_update.  The library's geometry picks RS = 1 for every small lattice, so a case
here is a SHAPE RULE, not a lattice: `instance(case, rs)` gives the lattice, the particle number and the start state of the case
at frame height rs, sized from own(rs) so that the same tile structure (three tiles between walls with a ragged last one, one
tile, two tiles on a ring, ...) is met at every RS; the GPU test forces that frame (APS_TS_R, APS_FU_R).

Classes: {walls, torus} x {k1, kn (K in 2, 3, 5)} x {f64, i32 (the 32-bit field: fp32=True on the handle, sum_bits=29 on the
oracle)}.  Every class holds three seeded random draws (`draws()`; rates, beta, the four switches, anchors, dead and bound
particles from the start: the distributions of _random_case in tests/test_gpu_parity.py) and a share of the named edges
(`edges()`).  THE TABLE IS PART OF THIS FILE'S BEHAVIOUR: another seed, range or order is another set of checks.

Redraws.  A draw has to meet the conditions of tests/test_sync_cases_cpu.py at all eight RS (it moves, proposes hops both ways
and flips, has refused hops, binds / unbinds / records exits where its model says it can, carries accepted hops across a tile
boundary both ways, deposits within reach of each wall).  The distributions hold many sets that cannot (no diffusion, dt = 0.002
with slow rates, k_exit > 0 without `immobilize`: only a held particle leaves; K = 1 with k_on > 0: an anchor binds into free
capacity NEXT to the particle itself, so nothing ever binds with one cell per site).  Such a draw is drawn again from the same
distributions with the next attempt number; ATTEMPT below records the attempt every draw ended on (`python tests/sync_cases.py
--search`, run from the repository's root with the root on PYTHONPATH, is the loop that found them).  The first attempt that
passes is seldom one with anchors -- four of the 24 draws have them, one has all three anchor rates positive -- so the draws are
NOT what covers binding, unbinding and exits: the named edges anchors_exits_* (K > 1, every class), k1_bound_unbind_* (K = 1,
every class) and k1_exits_* are, and tests/test_sync_cases_cpu.py asserts that coverage class by class.

`oracle_run(tag, rs, ensemble=0)` steps SyncOracle through CALLS once per (case, rs) and keeps, after every call, the state, the
field on all sites with its sums and the per-particle sums (a `Snapshot` quacks like the oracle for check_lattice), the exit rows
at the end, and counts of what happened (proposals by kind, refused hops, boundary crossings, deposits per tile).  Cached and
shared: nobody writes into it."""
import functools
import sys
import time
import zlib

import numpy as np

from oracle import sync_oracle as so
from test_gpu_parity import params, random_state

RS_ALL = (1, 2, 3, 4, 5, 6, 7, 8)
CALLS = (7, 4, 1, 33, 2, 50, 3)                      # odd and even calls, calls too short for the loop, observations in between
WINDOW_CALLS = (1, 2, 3)
BCS, KCS, FIELDS = ("walls", "torus"), ("k1", "kn"), ("f64", "i32")
CLASSES = tuple((b, k, f) for b in BCS for k in KCS for f in FIELDS)
DRAWS_PER_CLASS = 3
DRAW_SEED = 20261020
EV_LEFT, EV_RIGHT, EV_FWD, EV_BIND, EV_UNBIND, EV_EXIT, EV_FLIP = 1, 2, 3, 4, 5, 6, 7
ORACLE_SECONDS = [0.0]                               # time spent inside oracle_run (the GPU test reports it)


# ----------------------------------------------------------------------------- geometry (restated from ts_choose_geometry)
def own(rs):
    """Sites a tile owns at frame height rs when the frame is forced: the frame's 64 rs sites less two halo sites a side."""
    return 64 * rs - 4


def tile_sites(L, rs):
    """own(rs), one less per turn while the last tile would hold one or two sites (the resident loop wants three: its
    neighbour's halo must lie inside it) -- never below half a frame, and only where there is more than one tile."""
    o = own(rs)
    while o > 32 * rs and L > o and L % o in (1, 2):
        o -= 1
    return o


def n_tiles(L, rs):
    o = tile_sites(L, rs)
    return (L + o - 1) // o


# ----------------------------------------------------------------------------- the cases
def _case(tag, bc, K, field, *, L, sigma, frac=0.5, n=None, dt=0.04, spins="random", dead=False, bound="none", table=False,
          beta2=None, **kw):
    """L = (a, b): a own(rs) + b sites.  n: a particle number ("full": L K) instead of frac L K.  bound: "none", "random" (any
    particle, 40 %) or "anchors" (every minus particle that starts on an anchor site)."""
    assert bc in BCS and field in FIELDS and K >= 1
    return dict(tag=tag, cls=(bc, "k1" if K == 1 else "kn", field), K=int(K), L=tuple(L), sigma=float(sigma), frac=float(frac), n=n,
                dt=float(dt), spins=spins, dead=bool(dead), bound=bound, table=bool(table), beta2=beta2, kw=dict(kw))


ATTEMPT = {}                 # (class, j) -> attempt number a draw ended on; filled from _ATTEMPT_TEXT below
_ATTEMPT_TEXT = """
walls/k1/f64 0 0
walls/k1/f64 1 9
walls/k1/f64 2 0
walls/k1/i32 0 9
walls/k1/i32 1 0
walls/k1/i32 2 6
walls/kn/f64 0 2
walls/kn/f64 1 1
walls/kn/f64 2 2
walls/kn/i32 0 5
walls/kn/i32 1 0
walls/kn/i32 2 6
torus/k1/f64 0 3
torus/k1/f64 1 12
torus/k1/f64 2 6
torus/k1/i32 0 0
torus/k1/i32 1 8
torus/k1/i32 2 1
torus/kn/f64 0 1
torus/kn/f64 1 0
torus/kn/f64 2 4
torus/kn/i32 0 4
torus/kn/i32 1 1
torus/kn/i32 2 0
"""


def _draw(cls, j, attempt):
    """The distributions of _random_case (tests/test_gpu_parity.py); the lattice comes from the shape rule L = 3 own + 5 and the
    width of the table by turns: j = 0 a reach below one tile at RS 8, j = 1 above two tiles (a ring's table ends at half the
    ring, so that draw lives on a ring of 6 own + 5 sites: three tiles of reach), j = 2 either."""
    bc, kc, field = cls
    rng = np.random.default_rng([DRAW_SEED, CLASSES.index(cls), j, attempt])
    K = 1 if kc == "k1" else (2, 3, 5)[j]
    sigma = float(rng.choice(((0.004, 0.02, 0.06), (0.2, 0.4), (0.004, 0.02, 0.11, 0.4))[j]))
    kw = dict(rate_diffusion=float(rng.choice([0.0, 0.05, 1.5, 9.0])), rate_active=float(rng.choice([0.0, 0.7, 6.0])),
              beta=float(rng.choice([0.0, 0.4, 1.7, 4.0])), minus_anchor=bool(rng.integers(2)),
              immobilize_when_anchored=bool(rng.integers(2)), suppress_flip_when_bound=bool(rng.integers(2)),
              crowding_suppresses_rates=bool(rng.integers(2)))
    if rng.integers(2):
        kw.update(anchor_positions=[float(x) for x in rng.random(int(rng.integers(1, 4)))], anchor_radius=float(rng.choice([0.0, 0.02, 0.2])),
                  k_on=float(rng.choice([0.0, 0.5, 4.0])), k_off=float(rng.choice([0.0, 0.3, 2.0])),
                  k_exit=float(rng.choice([0.0, 0.4, 3.0])))
    else:
        kw.update(k_on=0.0, k_off=0.0, k_exit=0.0)
    frac = float(rng.random() * rng.choice([0.2, 0.6, 1.0]))
    dt = float(rng.choice([0.002, 0.03, 0.2]))
    return _case(f"draw_{bc}_{kc}_{field}_{j}", bc, K, field, L=(6, 5) if bc == "torus" and j == 1 else (3, 5), sigma=sigma, frac=frac, dt=dt,
                 dead=j % 3 == 0,
                 bound="random" if j % 2 == 0 else "none", beta2=float(rng.choice([0.4, 1.7, 4.0])), **kw)


def can_bind(case):
    kw = case["kw"]
    return bool(kw.get("anchor_positions")) and kw.get("k_on", 0.0) > 0.0 and case["K"] > 1


def can_exit(case):
    """Only a held particle leaves: immobilize, spin -1, bound, on an anchor site (channels(), oracle/sync_oracle.c)."""
    kw = case["kw"]
    return (bool(kw.get("anchor_positions")) and kw.get("k_exit", 0.0) > 0.0 and kw.get("immobilize_when_anchored", True)
            and (case["bound"] != "none" or can_bind(case)))


def _plausible(case):
    """What can be told from a draw's parameters alone: the rest of the conditions is the CPU test's."""
    kw = case["kw"]
    if kw["rate_diffusion"] <= 0.0:
        return False                                         # no hop to the left, none refused
    if kw.get("anchor_positions"):
        if kw["k_on"] > 0.0 and kw["k_off"] > 0.0 and not can_bind(case):
            return False                                     # positive rates that bind nobody (K = 1)
        if kw["k_exit"] > 0.0 and not can_exit(case):
            return False                                     # a positive exit rate nobody can take
    return True


@functools.lru_cache(maxsize=None)
def draws():
    out = []
    for cls in CLASSES:
        for j in range(DRAWS_PER_CLASS):
            out.append(_draw(cls, j, ATTEMPT.get((cls, j), 0)))
    return tuple(out)


ANCHORS = dict(anchor_positions=[0.3, 0.7], anchor_radius=0.08, k_on=3.0, k_off=1.0)


@functools.lru_cache(maxsize=None)
def edges():
    """Named edges.  Each names its boundary condition and K itself; the two fields take turns (both where the edge is about
    the field's range or the capacity of the deposit lists)."""
    c = []
    # one tile: no neighbour at all between walls, the tile is its own neighbour on both sides on a ring
    c.append(_case("single_tile_walls", "walls", 2, "f64", L=(1, -7), sigma=0.1))
    c.append(_case("single_tile_torus", "torus", 1, "i32", L=(1, -7), sigma=0.1))
    # a last tile of exactly three sites, the least the loop takes (one or two make the geometry shrink its tiles)
    c.append(_case("last_tile_of_three_walls", "walls", 1, "i32", L=(1, 3), sigma=0.05))
    c.append(_case("last_tile_of_three_torus", "torus", 3, "i32", L=(1, 3), sigma=0.05))
    # two tiles on a ring: the left and the right neighbour are the same tile
    c.append(_case("two_tiles_torus_k1", "torus", 1, "f64", L=(2, 0), sigma=0.03))
    c.append(_case("two_tiles_torus_k2", "torus", 2, "i32", L=(2, 0), sigma=0.03))
    # a box comparable to the reach: every deposit has wall images in reach (the instance that carries the image list)
    c.append(_case("image_list_k1", "walls", 1, "f64", L=(3, 5), sigma=0.3, frac=0.6))
    c.append(_case("image_list_k3", "walls", 3, "i32", L=(3, 5), sigma=0.3, frac=0.6))
    # a table that spans the ring (reach L / 2): even L (the tap at L / 2 counts once) and odd L
    c.append(_case("ring_wide_even_k1", "torus", 1, "f64", L=(3, 6), sigma=0.4))
    c.append(_case("ring_wide_even_k2", "torus", 2, "i32", L=(3, 6), sigma=0.4))
    c.append(_case("ring_wide_odd_k1", "torus", 1, "i32", L=(3, 5), sigma=0.4))
    c.append(_case("ring_wide_odd_k2", "torus", 2, "f64", L=(3, 5), sigma=0.4))
    # a full lattice: every hop is refused, only flips happen
    c.append(_case("full_walls_k1", "walls", 1, "i32", L=(3, 5), sigma=0.02, n="full"))
    c.append(_case("full_torus_k3", "torus", 3, "f64", L=(3, 5), sigma=0.02, n="full"))
    # all spins +1 on a full lattice: |S| = W at its maximum, the top of the 32-bit grid
    c.append(_case("all_plus_full_walls_k2", "walls", 2, "i32", L=(3, 5), sigma=0.11, n="full", spins="plus"))
    c.append(_case("all_plus_full_torus_k3", "torus", 3, "i32", L=(3, 6), sigma=0.11, n="full", spins="plus"))
    c.append(_case("all_plus_full_torus_k1", "torus", 1, "f64", L=(3, 5), sigma=0.4, n="full", spins="plus"))
    c.append(_case("one_particle_walls", "walls", 2, "f64", L=(3, 5), sigma=0.02, n=1, rate_diffusion=6.0, dt=0.2))
    c.append(_case("one_particle_torus", "torus", 1, "i32", L=(3, 5), sigma=0.02, n=1, rate_diffusion=6.0, dt=0.2))
    # dense and diffusive: deposits in reach of a tile pass 128 per wave segment at RS >= 5 (frac 0.95 refuses most hops: the pooled
    # 1040 are left to half_full_k5_* below)
    c.append(_case("dense_k3_walls", "walls", 3, "f64", L=(3, 5), sigma=0.05, frac=0.95, rate_diffusion=6.0, dt=0.2))
    c.append(_case("dense_k3_torus", "torus", 3, "i32", L=(3, 5), sigma=0.05, frac=0.95, rate_diffusion=6.0, dt=0.2))
    c.append(_case("dense_k5_walls", "walls", 5, "i32", L=(3, 5), sigma=0.05, frac=0.95, rate_diffusion=6.0, dt=0.2))
    c.append(_case("dense_k5_torus", "torus", 5, "f64", L=(3, 5), sigma=0.05, frac=0.95, rate_diffusion=6.0, dt=0.2))
    c.append(_case("global_field_walls", "walls", 1, "f64", L=(3, 5), sigma=0.0, beta=1.6))
    c.append(_case("global_field_torus", "torus", 2, "f64", L=(3, 5), sigma=0.0, beta=1.6))
    c.append(_case("flip_table_walls", "walls", 1, "f64", L=(3, 5), sigma=0.02, table=True))
    c.append(_case("flip_table_torus", "torus", 2, "i32", L=(3, 5), sigma=0.02, table=True))
    # one cell per site, particles bound from the start that leave: the resident loop carries no exit code for K = 1 and must refuse
    c.append(_case("k1_exits_immobilize_walls", "walls", 1, "f64", L=(3, 5), sigma=0.02, bound="anchors", k_exit=1.5, **ANCHORS))
    c.append(_case("k1_exits_immobilize_torus", "torus", 1, "i32", L=(3, 5), sigma=0.02, bound="anchors", k_exit=1.5, **ANCHORS))
    # K > 1 with anchors, every anchor rate positive and `immobilize` on: particles bind, unbind and LEAVE -- the exit code of
    # tile_step and of the four-wave loop (dead marks and the exit log written from inside the loop) in both fields
    for bc, K, field in (("walls", 2, "f64"), ("walls", 3, "i32"), ("torus", 3, "f64"), ("torus", 2, "i32")):
        c.append(_case(f"anchors_exits_{bc}_k{K}", bc, K, field, L=(3, 5), sigma=0.02, k_exit=1.5, **ANCHORS))
    # one cell per site with particles bound from the start that unbind and never leave: anchors through the loops of K = 1
    # (eight waves included)
    for bc in BCS:
        for field in FIELDS:
            c.append(_case(f"k1_bound_unbind_{bc}_{field}", bc, 1, field, L=(3, 5), sigma=0.02, bound="random", k_exit=0.0, **ANCHORS))
    # half full and diffusive with five cells per site: most hops are granted, and a wide table puts them all in reach of a tile --
    # more than the pooled 1040 deposits of one class at the larger frames
    c.append(_case("half_full_k5_walls", "walls", 5, "i32", L=(3, 5), sigma=0.2, frac=0.5, rate_diffusion=6.0, dt=0.2))
    c.append(_case("half_full_k5_torus", "torus", 5, "f64", L=(3, 5), sigma=0.2, frac=0.5, rate_diffusion=6.0, dt=0.2))
    return tuple(c)


def all_cases():
    return draws() + edges()


def by_tag(tag):
    return next(c for c in all_cases() + site_range_cases() + window_cases() if c["tag"] == tag)


def is_draw(case):
    return case["tag"].startswith("draw_")


def tanh_table(n=16):
    """[2][n + 1]: a caller's flip rate 1 - 0.8 sigma tanh(2 m) tabulated at m = -1 + 2 i / n (aps_set_flip_table's layout)."""
    m = -1.0 + 2.0 * np.arange(n + 1) / n
    return np.ascontiguousarray(np.stack([1.0 - 0.8 * np.tanh(2.0 * m), 1.0 + 0.8 * np.tanh(2.0 * m)]))


# ----------------------------------------------------------------------------- site ranges and windowed tables
@functools.lru_cache(maxsize=None)
def site_range_cases():
    """K = 2 with exits on 4 * 3 * reach tiles and a ragged last one of seven sites (a Gaussian of 8 sites: its table ends within
    one tile at every RS, so reach = 1 between walls; across the seam of a ring the last tile is shorter than the table and a
    frame's reach takes in two tiles), the same lattice for two and for three ranks; 3 x 20 steps."""
    out = []
    for bc in BCS:
        out.append(_case(f"site_ranges_{bc}", bc, 2, "f64", L=(12 if bc == "walls" else 24, 7), sigma=-8.0, frac=0.45, rate_diffusion=3.0,
                         anchor_positions=[0.25, 0.5, 0.75], anchor_radius=0.02, k_on=2.0, k_off=1.0, k_exit=0.7))
    return tuple(out)


SITE_RANGE_RS = (2, 5, 8)
SITE_RANGE_CALLS = (20, 20, 20)


@functools.lru_cache(maxsize=None)
def window_cases():
    """Tables beyond LDS (tile_step<BC, false, ...>): the smallest such table between walls -- binary64: L = 60 000, sigma = 0.1,
    24 001 taps of 8 bytes; 32-bit field: L = 120 000, 48 001 taps of 4 bytes, q = 12 -- and on a ring whose table spans it
    (L / 2 + 1 entries; gathers from global memory, no windows).  One lattice for every RS: the oracle runs once per case."""
    out = []
    for bc in BCS:
        for K in (1, 3):
            for field in FIELDS:
                L = 60000 if field == "f64" else 120000
                sigma = 0.1 if (bc == "walls" or field == "f64") else 0.16       # (the coarse grid of the 32-bit field cuts a Gaussian short)
                c = _case(f"window_{bc}_k{K}_{field}", bc, K, field, L=(0, L), sigma=sigma, n=3000, dt=0.05)
                out.append(c)
    return tuple(out)


# ----------------------------------------------------------------------------- a case at one frame height
def lattice_sites(case, rs):
    a, b = case["L"]
    return a * own(rs) + b


@functools.lru_cache(maxsize=None)
def _instance(tag, rs, ensemble):
    case = by_tag(tag)
    L, K = lattice_sites(case, rs), case["K"]
    sigma = case["sigma"] if case["sigma"] >= 0 else -case["sigma"] / L          # negative: a width in sites
    kw = dict(case["kw"])
    if ensemble:
        kw["beta"] = case["beta2"]
    par = params(L=L, K=K, sigma=sigma, periodic=case["cls"][0] == "torus", **kw)
    N = L * K if case["n"] == "full" else (case["n"] if case["n"] is not None else max(1, int(case["frac"] * L * K)))
    key = zlib.crc32(tag.encode())
    rng = np.random.default_rng([key, rs, ensemble])
    pos, spin = random_state(rng, L, N, K)
    if case["spins"] == "plus":
        spin = np.ones(N, np.int8)
    alive = (rng.random(N) > 0.15).astype(np.uint8) if case["dead"] else np.ones(N, np.uint8)
    if case["bound"] == "random":
        bound = (rng.random(N) > 0.6).astype(np.uint8)
    elif case["bound"] == "anchors":
        bound = ((par.is_anchor_site[pos] != 0) & (spin < 0)).astype(np.uint8)
    else:
        bound = np.zeros(N, np.uint8)
    seed = int(key) * 1000003 + 17 * rs + 1
    for a in (pos, spin, bound, alive):
        a.setflags(write=False)
    return dict(case=case, rs=rs, L=L, K=K, N=N, par=par, pos=pos, spin=spin, bound=bound, alive=alive, dt=case["dt"], seed=seed,
                ensemble=ensemble, fp32=case["cls"][2] == "i32", flip_table=tanh_table() if case["table"] else None,
                periodic=case["cls"][0] == "torus")


def instance(case, rs, ensemble=0):
    return _instance(case["tag"], rs, ensemble)


def make_oracle(inst, flip_table="own"):
    orc = so.SyncOracle(inst["par"], dt=inst["dt"], seed=inst["seed"], ensemble=inst["ensemble"],
                        flip_table=inst["flip_table"] if flip_table == "own" else flip_table, **(dict(sum_bits=29) if inst["fp32"] else {}))
    orc.set_state(inst["pos"], inst["spin"], bound=inst["bound"], alive=inst["alive"])
    return orc


class Snapshot:
    """The oracle after a call, frozen: what check_lattice (tests/test_gpu_parity.py) and the state comparisons read."""

    def __init__(self, orc):
        self.par = orc.par
        self.pos, self.spin, self.bound, self.alive = orc.pos.copy(), orc.spin.copy(), orc.bound.copy(), orc.alive.copy()
        self._field = orc.field_sites()
        self.last_site_sums = orc.last_site_sums
        self._pairs = orc.pair_sums()
        self.step_index = orc.step_index
        for a in (self.pos, self.spin, self.bound, self.alive) + tuple(self._field) + tuple(self.last_site_sums) + tuple(self._pairs):
            a.setflags(write=False)

    def field_sites(self):
        return self._field

    def pair_sums(self):
        return self._pairs


def _tally(st, inst, o, reach, before, detail, after):
    """What one step did, from its proposal and acceptance bytes."""
    pos0, spin0, bound0, alive0 = before
    prop, acc = detail["prop"], detail["accepted"] != 0
    L = inst["L"]
    st["proposed"] += np.bincount(prop, minlength=8)[:8]
    hop = (prop == EV_LEFT) | (prop == EV_RIGHT) | (prop == EV_FWD)
    st["refused"] += int((hop & ~acc & (alive0 != 0)).sum())
    for code, key in ((EV_BIND, "bound"), (EV_UNBIND, "unbound"), (EV_EXIT, "left_system"), (EV_FLIP, "flipped")):
        st[key] += int(((prop == code) & acc).sum())
    ok = hop & acc
    old, new = pos0[ok].astype(np.int64), after[ok].astype(np.int64)
    cross = old // o != new // o
    to_left = prop[ok] == EV_LEFT
    st["cross_left"] += int((cross & to_left).sum())
    st["cross_right"] += int((cross & ~to_left).sum())
    # deposits: a hop takes a particle off one site and puts it on another (class P: plus particles, M: minus), a flip and an
    # exit deposit on the particle's site
    site = np.concatenate([old, new, pos0[acc & ((prop == EV_FLIP) | (prop == EV_EXIT))].astype(np.int64)])
    if site.size:
        st["near_left_wall"] += int((site <= reach).sum())
        st["near_right_wall"] += int((site >= L - 1 - reach).sum())
    # what a tile's deposit lists of one class hold in a step: the deposits within the table's reach of the sites it owns
    for sign in (1, -1):
        m = spin0[ok] == sign
        s2 = np.concatenate([old[m], new[m]])
        for lo in range(0, L if s2.size else 0, o):
            n_own = min(L, lo + o) - lo
            if inst["periodic"]:
                near = (((s2 - lo) % L) < n_own + reach) | (((lo - s2) % L) <= reach)
            else:
                near = (s2 >= lo - reach) & (s2 < lo + n_own + reach)
            st["max_class_deposits"] = max(st["max_class_deposits"], int(near.sum()))


@functools.lru_cache(maxsize=None)
def _oracle_run(tag, rs, ensemble, flip_table):
    t0 = time.perf_counter()
    inst = _instance(tag, rs, ensemble)
    case = inst["case"]
    calls = WINDOW_CALLS if tag.startswith("window_") else SITE_RANGE_CALLS if tag.startswith("site_ranges_") else CALLS
    orc = make_oracle(inst, "own" if flip_table else None)
    o, reach = tile_sites(inst["L"], rs), max(len(orc.table) - 1, 0) if inst["par"].sigma_kernel > 0 else inst["L"]
    st = dict(proposed=np.zeros(8, np.int64), refused=0, bound=0, unbound=0, left_system=0, flipped=0, cross_left=0, cross_right=0,
              near_left_wall=0, near_right_wall=0, max_class_deposits=0)
    snaps = []
    light = tag.startswith("window_")                        # (long lattices: no per-step tally)
    for n in calls:
        for _ in range(n):
            if light:
                orc.step()
                continue
            before = (orc.pos.copy(), orc.spin.copy(), orc.bound.copy(), orc.alive.copy())
            d = orc.step(want_detail=True)
            _tally(st, inst, o, reach, before, d, orc.pos)
        snaps.append(Snapshot(orc))
    moved = int((orc.pos != inst["pos"]).sum())
    out = dict(inst=inst, calls=calls, snaps=tuple(snaps), exits=orc.exits(), stats=st, moved=moved, table=orc.table, q=orc.q,
               tile_sites=o, n_tiles=n_tiles(inst["L"], rs), seconds=time.perf_counter() - t0)
    ORACLE_SECONDS[0] += out["seconds"]
    return out


def oracle_run(case, rs, ensemble=0, flip_table=True):
    """The oracle's trajectory of `case` at frame height rs (flip_table=False: the same run without the case's flip table)."""
    return _oracle_run(case["tag"], rs, ensemble, bool(flip_table))


# ----------------------------------------------------------------------------- which path admits which (case, rs)
def loop4_verdict(case, rs):
    """(eligible, reason the library gives when it is not), written out from loop_prepare and tl_kernel_f (csrc/aps_hip.hip), in
    the order loop_prepare asks: global field; one cell per site with particles that can leave; no kernel for the frame
    (binary64 frames of 8 rows, and of 7 rows with K > 1, would not fit 256 VGPRs and are not built)."""
    kw = case["kw"]
    if case["sigma"] == 0.0:
        return False, "global mean field"
    if case["K"] == 1 and kw.get("immobilize_when_anchored", True) and kw.get("k_exit", 0.0) > 0.0:
        return False, "particles can leave the system"
    if case["cls"][2] == "f64" and (rs == 8 or (rs == 7 and case["K"] > 1)):
        return False, "no kernel for this frame"
    return True, ""


def loop8_admits(case, rs):
    """Eight waves per tile: binary64, one cell per site, frames of 5 to 8 rows -- and a case the loop takes at all."""
    kw = case["kw"]
    return (case["cls"][1] == "k1" and case["cls"][2] == "f64" and rs >= 5 and case["sigma"] != 0.0
            and not (kw.get("immobilize_when_anchored", True) and kw.get("k_exit", 0.0) > 0.0))


def lattice_admits(case, rs):
    return case["cls"][2] == "f64" and rs >= 2


def ensemble_cases():
    """One walls and one torus draw per K class (the fields by turns) run as ensemble 1 of two."""
    want = [("walls", "k1", "f64"), ("torus", "k1", "i32"), ("walls", "kn", "i32"), ("torus", "kn", "f64")]
    return tuple(next(c for c in draws() if c["cls"] == cls and c["tag"].endswith("_1")) for cls in want)


def _search(max_attempts=60, only=()):
    """Finds ATTEMPT: for every draw (or those named as class:j in `only`) the first attempt that is plausible and meets the CPU
    test's conditions at every RS."""
    import test_sync_cases_cpu as T
    for cls in CLASSES:
        for j in range(DRAWS_PER_CLASS):
            if only and f"{'/'.join(cls)}:{j}" not in only:
                continue
            for attempt in range(max_attempts):
                case = _draw(cls, j, attempt)
                if not _plausible(case):
                    continue
                ATTEMPT[(cls, j)] = attempt
                draws.cache_clear()
                _instance.cache_clear()
                _oracle_run.cache_clear()
                try:
                    for rs in (8, 1, 2, 3, 4, 5, 6, 7):
                        T.check_draw(case, rs)
                except AssertionError as e:
                    print("   ", cls, j, attempt, "fails:", str(e)[:100], flush=True)
                    continue
                print(f"{'/'.join(cls)} {j} {attempt}", flush=True)
                break
            else:
                raise SystemExit(f"no attempt found for {cls} {j}")


for _line in _ATTEMPT_TEXT.split("\n"):
    if _line.strip():
        _c, _j, _a = _line.split()
        ATTEMPT[(tuple(_c.split("/")), int(_j))] = int(_a)

if __name__ == "__main__" and "--search" in sys.argv:
    import sync_cases                                        # (the module the CPU test imports, not __main__)
    sync_cases._search(only=tuple(a for a in sys.argv[1:] if ":" in a))
