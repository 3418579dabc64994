"""Parameter sets for the same-uniforms parity of the exact event loop (tests/test_exact_loop_cases_cpu.py checks the list itself
on the CPU, tests/test_gpu_exact_loop_random.py runs it through every entry point of the loop).  A helper module, not a test.

`hand_cases()` names the edges the ten hand-written sets of tests/test_gpu_gillespie.py leave out: rings of two sites, full
lattices, one particle, interaction ranges beyond the box, a caller's flip table (also at m = +1 and m = -1 exactly), runs that
empty, zero rates, K = 5 with crowding, and particle numbers on both sides of the slot-count boundaries of batch_shape (a lane
owns ceil(n_cap / 64) slots up to 1024 particles, ceil(n_cap / 256) above).  `random_cases()` draws 32 more from a fixed seed;
THE LIST IS PART OF THIS FILE'S BEHAVIOUR: another seed, range or order is another set of checks and is reviewed as such.

A case is a plain dictionary: the oracle's constructor keywords under "kw", the particle number, how the initial state is drawn
("spins", "bound"), the flip table ("table": (shape, flip_n) or None), the number of events to aim at ("events") or "T", and
"useed", which picks the table of uniforms.  `prepared(case)` adds what follows from it (oracle, state, T, observation times,
uniforms, flip table); `oracle_run(case)` is the trajectory of the CPU restatement of the reference under those uniforms, with
the margins of its draws.  Both are computed once per case and shared; nobody writes into them.

Margins.  The GPU's rates differ from the oracle's by up to 1e-10 relative (tests/test_gpu_gillespie.py), so the two sides can
only be held to the same trajectory when no draw lands that close to the threshold it is compared with.  MarginRng records,
per kind of comparison, the smallest distance over the run:
    particle  u1 against the normalised cumulative rates (the comparison of choice(p=...)),
    channel   v = u2 * rates[i] against the five channel edges, relative to rates[i],
    side      u3 against a / (a + b) where a hop picks its direction,
    time      an event's time against the observation times and T, relative to T (decides which state an observation records).
The CPU test asserts every one of them >= MARGIN_FLOOR = 1e-8 for every case; a case that fails it gets another "useed" here.

Flip tables are smooth (FLIP_SHAPES): the interpolation of a table across a jump has slope 1 / cell, which turns a 1e-10
difference in m into a rate difference no margin covers; the threshold callable of fixture G9 stays with its statistical test.
"""
import functools
import zlib

import numpy as np

from oracle.gillespie_numpy import GillespieOracle
from test_gpu_gillespie import TableRng

N_ROWS = 2048               # rows of a case's table of uniforms: no case is meant to fire more than about 1500 events
N_OBS = 12
MARGIN_FLOOR = 1e-8
RANDOM_SEED = 20261019
FLAGS = ("minus_anchor", "immobilize_when_anchored", "suppress_flip_when_bound", "crowding_suppresses_rates")

# name -> (flip_rate_fn(sigma, m), max |d2 f / dm2| on [-1, 1]); 4 / (3 sqrt 3) = max |2 tanh sech^2|
FLIP_SHAPES = {
    "tanh": (lambda s, m: 1.0 - 0.8 * np.asarray(s, float) * np.tanh(1.3 * np.asarray(m, float)), 0.8 * 1.3 ** 2 * 4.0 / (3.0 * np.sqrt(3.0))),
    "quad": (lambda s, m: np.where(np.asarray(s) > 0, 0.6 + 0.4 * np.asarray(m, float) ** 2, 0.5 + 0.3 * (np.asarray(m, float) + 0.2) ** 2), 0.8),
}


def flip_table(shape, n):
    """[2][n + 1]: the rows of spin +1 and -1 at m = -1 + 2 i / n (aps_set_flip_table's layout)."""
    m = -1.0 + 2.0 * np.arange(n + 1) / n
    fn = FLIP_SHAPES[shape][0]
    return np.stack([fn(np.ones(n + 1), m), fn(-np.ones(n + 1), m)])


def table_callable(tab):
    """flip_rate_fn(sigma, m) reading `tab` with the arithmetic of channels() (csrc/aps_common.hpp), operation for operation; the
    library is built with -ffp-contract=off, so given the same m the bits are the device's."""
    tab = np.ascontiguousarray(tab, dtype=np.float64)
    n = tab.shape[1] - 1

    def fn(sigma, m):
        u = (np.asarray(m, dtype=np.float64) + 1.0) * (0.5 * float(n))
        i = np.clip(u.astype(np.int64), 0, n - 1)
        f = u - i.astype(np.float64)
        row = np.where(np.asarray(sigma) > 0, 0, 1)
        a, b = tab[row, i], tab[row, i + 1]
        return a + f * (b - a)
    return fn


class MarginRng(TableRng):
    """TableRng that also records how far every draw was from the thresholds it was compared with; `orc.last_rt` is the rate
    table of the event being fired (SpyOracle keeps it)."""

    def __init__(self, table, orc):
        super().__init__(table)
        self.margin = dict(particle=np.inf, channel=np.inf, side=np.inf, time=np.inf)
        self.orc, self.i = orc, -1

    def _note(self, key, d):
        self.margin[key] = min(self.margin[key], float(d))

    def choice(self, n, p=None):
        cdf = np.cumsum(p)
        cdf /= cdf[-1]
        self._note("particle", np.min(np.abs(cdf - self.table[self.row, 1])))
        self.i = super().choice(n, p=p)
        return self.i

    def random(self):
        col, u = self.col, super().random()
        rt, i = self.orc.last_rt, self.i
        if col == 2:                                           # fire_event's edges, same association
            rate = rt["total"][i]
            e = rt["diff"][i]
            edges = [e]
            for key in ("act", "attach", "detach", "leave"):
                e = e + rt[key][i]
                edges.append(e)
            self._note("channel", np.min(np.abs(u * rate - np.array(edges))) / rate)
        else:
            a, b = rt["hop_l"][i], rt["hop_r"][i]
            self._note("side", abs(u - a / (a + b)))
        return u


class SpyOracle(GillespieOracle):
    def rate_table(self, *args):
        rt = super().rate_table(*args)
        self.last_rt = rt                                      # MarginRng reads the thresholds of the event being fired from it
        return rt


def margin_event_loop(orc, pos0, sigma0, bound0, table, T, times):
    """tests/test_gpu_gillespie.py's oracle_event_loop with a start state that may hold bound particles, the live-particle
    and event counts of every observation, and the margins of MarginRng.  A run whose total rate fell to zero (nobody left,
    or nothing can happen) ends as the device ends it (tests/test_gpu_edge_cases.py): the time is +inf and the event that
    could not fire is not counted."""
    rng = orc.rng = MarginRng(table, orc)
    L = orc.par.L
    pos, sigma, bound = pos0.copy(), sigma0.copy(), bound0.copy()
    cp, cm = np.bincount(pos[sigma == 1], minlength=L), np.bincount(pos[sigma == -1], minlength=L)
    snaps, live, events, exits = [(pos.copy(), sigma.copy(), bound.copy())], [pos.size], [0], ([], [])
    marks = np.append(times, T)
    k, t, ev, frozen = 1, 0.0, 0, False
    while t < T and k < len(times) and ev < len(table):
        tau = np.inf
        if pos.size:
            field = orc.mean_field(cp, cm)
            pos, sigma, bound, tau = orc.fire_event(pos, sigma, bound, field, cp, cm, t, exits)
        if np.isinf(tau):
            t, frozen = np.inf, True
            break
        ev += 1
        t += tau
        rng._note("time", np.min(np.abs(marks - t)) / T)
        if t > T:
            break
        while k < len(times) and times[k] <= t:
            snaps.append((pos.copy(), sigma.copy(), bound.copy()))
            live.append(pos.size)
            events.append(ev)
            k += 1
    return dict(snaps=snaps, live=live, events=events, exits=exits, t=t, ev=ev, frozen=frozen, margin=dict(rng.margin),
                n_left=int(pos.size))


# ----------------------------------------------------------------------------- the cases
def _case(tag, *, L, K, N, sigma=0.0, periodic=False, rd=0.5, ra=4.0, beta=1.0, anchors=None, radius=0.0, k_on=0.0, k_off=0.0,
          k_exit=0.0, minus_anchor=True, immobilize=True, suppress_flip=True, crowding=False, spins="random", bound="none",
          table=None, events=800, T=None, useed=0, low_activity=False):
    kw = dict(L=int(L), xlim=1.0, scale_rates=False, site_capacity=int(K), local_kernel_sigma=float(sigma), periodic=bool(periodic),
              rate_diffusion=float(rd), rate_active=float(ra), beta=float(beta), anchor_positions=anchors, anchor_radius=float(radius),
              k_on=float(k_on), k_off=float(k_off), k_exit=float(k_exit), minus_anchor=bool(minus_anchor),
              immobilize_when_anchored=bool(immobilize), suppress_flip_when_bound=bool(suppress_flip),
              crowding_suppresses_rates=bool(crowding))
    return dict(tag=tag, kw=kw, N=int(N), spins=spins, bound=bound, table=table, events=int(events), T=T, useed=int(useed),
                low_activity=bool(low_activity))


@functools.lru_cache(maxsize=None)
def hand_cases():
    c = [
        _case("ring_of_two_k3", L=2, K=3, N=4, periodic=True, sigma=0.3, beta=0.8),
        _case("walls_of_three_full", L=3, K=2, N=6, sigma=0.2, beta=1.2),
        _case("full_ring", L=40, K=2, N=80, periodic=True, sigma=0.05, beta=0.7),
        _case("full_ring_table", L=30, K=3, N=90, periodic=True, sigma=0.0, beta=0.7, table=("quad", 8)),
        _case("one_particle", L=50, K=1, N=1, sigma=0.04, beta=1.0, events=400),
        _case("one_particle_ring_table", L=7, K=2, N=1, periodic=True, sigma=0.0, beta=1.0, table=("tanh", 64), events=400),
        _case("ring_sigma_2p5_boxes", L=90, K=2, N=70, periodic=True, sigma=2.5, beta=1.5),
        _case("walls_reach_beyond_box", L=24, K=3, N=30, sigma=0.4, beta=1.5, events=500),
        _case("global_field_table", L=80, K=2, N=70, sigma=0.0, beta=1.0, table=("tanh", 8)),
        _case("all_plus_table_local", L=60, K=2, N=50, sigma=0.05, beta=1.0, spins="plus", table=("tanh", 8)),
        _case("all_plus_table_global", L=60, K=1, N=40, sigma=0.0, periodic=True, beta=1.0, spins="plus", table=("quad", 1)),
        _case("all_minus_table_global", L=60, K=2, N=40, sigma=0.0, beta=1.0, spins="minus", table=("tanh", 65536), events=350),
        _case("all_leave", L=60, K=2, N=40, sigma=0.03, beta=0.5, anchors=[0.0, 0.5, 0.99], radius=0.2, k_on=5.0, k_off=0.0, k_exit=8.0,
              T=9.0),
        _case("no_diffusion", L=120, K=2, N=100, sigma=0.02, rd=0.0, beta=1.0),
        _case("no_active_rate", L=120, K=2, N=100, sigma=0.02, periodic=True, ra=0.0, beta=1.0),
        _case("beta_zero", L=100, K=1, N=60, sigma=0.03, beta=0.0),
        _case("k5_crowding", L=70, K=5, N=240, sigma=0.03, periodic=True, beta=0.9, crowding=True),
        _case("k5_crowding_table_anchors", L=64, K=5, N=200, sigma=0.02, beta=0.9, crowding=True, table=("quad", 65536),
              anchors=[0.0, 1.0], radius=0.05, k_on=2.0, k_off=1.0, k_exit=0.5, immobilize=False, suppress_flip=False, bound="random"),
    ]
    # a particle binds only where its own site has room left (occ < K counts the particle itself), hence K = 2 in "all_leave"
    # both sides of the slot-count boundaries of batch_shape: L K just above n0, a short run
    for n0, K, per, tab in ((64, 1, False, None), (65, 2, True, ("tanh", 8)), (1024, 3, False, ("quad", 1)), (1025, 2, True, None)):
        L = n0 // K + 3
        c.append(_case(f"slots_{n0}", L=L, K=K, N=n0, periodic=per, sigma=1.5 / L, beta=1.0, table=tab, events=600,
                       anchors=[0.4], radius=2.0 / L, k_on=2.0, k_off=1.0, k_exit=0.3))
    return tuple(c)


USEED = {}                  # random case -> another table of uniforms, where the first one put a draw within MARGIN_FLOOR of a threshold


@functools.lru_cache(maxsize=None)
def random_cases(n=32, seed=RANDOM_SEED):
    rng = np.random.default_rng(seed)
    out = []
    for j in range(n):
        L = int(round(2.0 * 200.0 ** rng.random()))
        K = int(rng.integers(1, 6))
        periodic = bool(rng.random() < 0.5)
        mode = ("global", "narrow", "half", "over")[int(rng.integers(4))]
        if mode in ("half", "over") and not periodic:
            L = min(L, 48)                                     # the oracle's reflecting filter costs its radius per event
        reach = dict(narrow=rng.uniform(1.2, 12.0), half=rng.uniform(0.5, 1.0) * L, over=rng.uniform(1.05, 2.5) * L)
        sigma = 0.0 if mode == "global" else reach[mode] / 4.0 / L          # reach = 4 sigma_grid = 4 sigma L sites
        pick = rng.random()
        N = 1 if pick < 0.1 else (L * K if pick < 0.2 else int(rng.integers(1, L * K + 1)))
        beta = 0.0 if rng.random() < 0.1 else float(np.round(rng.uniform(0.0, 3.0), 3))
        rates = [0.0 if rng.random() < 1.0 / 6.0 else float(np.round(rng.uniform(lo, hi), 3))
                 for lo, hi in ((0.2, 1.5), (1.0, 6.0), (0.5, 4.0), (0.5, 4.0), (0.2, 2.0))]
        anchors = None
        if rng.random() < 0.65:
            anchors = [float(np.round(x, 3)) for x in rng.random(int(rng.integers(1, 4)))]
            if rng.random() < 0.4:
                anchors.append(0.0)                            # site 0
            if rng.random() < 0.4:
                anchors.append(1.0)                            # site L - 1
        radius = float(np.round(rng.uniform(0.0, 0.06), 4))
        flags = [bool(rng.random() < 0.5) for _ in range(4)]
        bound = "random" if rng.random() < 1.0 / 3.0 else "none"
        table = (("tanh", "quad")[int(rng.integers(2))], int(rng.choice([1, 8, 64, 65536]))) if rng.random() < 1.0 / 3.0 else None
        spins = "plus" if rng.random() < 0.1 else "random"
        events = int(rng.integers(400, 1200))
        out.append(_case(f"random_{j:02d}_{mode}", L=L, K=K, N=N, sigma=sigma, periodic=periodic, rd=rates[0], ra=rates[1], beta=beta,
                         anchors=anchors, radius=radius, k_on=rates[2], k_off=rates[3], k_exit=rates[4], minus_anchor=flags[0],
                         immobilize=flags[1], suppress_flip=flags[2], crowding=flags[3], spins=spins, bound=bound, table=table,
                         events=events, useed=USEED.get(j, 0)))
    return tuple(out)


def all_cases():
    return hand_cases() + random_cases()


def by_tag(tag):
    return next(c for c in all_cases() if c["tag"] == tag)


@functools.lru_cache(maxsize=None)
def _prepared(tag):
    case = by_tag(tag)
    kw, N = case["kw"], case["N"]
    L, K = kw["L"], kw["site_capacity"]
    key = zlib.crc32(tag.encode())
    rng = np.random.default_rng(key)
    pos0 = rng.choice(np.repeat(np.arange(L), K), size=N, replace=False).astype(np.int64)
    sigma0 = rng.choice(np.array([1, -1], np.int8), size=N)
    if case["spins"] != "random":
        sigma0 = np.full(N, 1 if case["spins"] == "plus" else -1, np.int8)
    bound0 = rng.random(N) < 0.3 if case["bound"] == "random" else np.zeros(N, bool)     # any spin, on and off the anchor sites
    tab = None if case["table"] is None else flip_table(*case["table"])
    orc = SpyOracle(init="fixed", N=N, rng=None, flip_rate_fn=None if tab is None else table_callable(tab), **kw)
    T = case["T"]
    if T is None:                                              # the events aimed at over the total rate of the start state
        cp, cm = np.bincount(pos0[sigma0 == 1], minlength=L), np.bincount(pos0[sigma0 == -1], minlength=L)
        R0 = float(orc.rate_table(pos0, sigma0, bound0, orc.mean_field(cp, cm), cp, cm)["total"].sum())
        T = float(f"{case['events'] / R0:.3g}") if R0 > 0 else 1.0
    times = (T / N_OBS) * np.arange(N_OBS)
    uniforms = np.random.default_rng([key, case["useed"]]).random((N_ROWS, 4))
    for a in (pos0, sigma0, bound0, times, uniforms):
        a.setflags(write=False)
    return dict(case=case, orc=orc, pos0=pos0, sigma0=sigma0, bound0=bound0, T=T, times=times, uniforms=uniforms, flip_table=tab)


def prepared(case):
    return _prepared(case["tag"])


@functools.lru_cache(maxsize=None)
def _oracle_run(tag):
    p = _prepared(tag)
    return margin_event_loop(p["orc"], p["pos0"], p["sigma0"], p["bound0"], p["uniforms"], p["T"], p["times"])


def oracle_run(case):
    return _oracle_run(case["tag"])


def features(case):
    """The names of what a case exercises (the census of tests/test_exact_loop_cases_cpu.py counts them)."""
    kw, p = case["kw"], prepared(case)
    L, K, N = kw["L"], kw["site_capacity"], case["N"]
    reach = 4.0 * kw["local_kernel_sigma"] * L
    mask = p["orc"].par.is_anchor_site
    f = {"ring" if kw["periodic"] else "walls", f"K={K}"}
    f.add("field_global" if reach == 0 else "field_narrow" if reach < L / 2 else "field_half" if reach <= L else "field_over")
    for name, on in (("K>3", K > 3), ("L<=3", L <= 3), ("one_particle", N == 1), ("full", N == L * K), ("beta=0", kw["beta"] == 0.0),
                     ("rate_diffusion=0", kw["rate_diffusion"] == 0.0), ("rate_active=0", kw["rate_active"] == 0.0),
                     ("anchors", bool(mask.any())), ("anchor_at_0", bool(mask[0])), ("anchor_at_L-1", bool(mask[-1])),
                     ("bound0", bool(p["bound0"].any())), ("bound0_plus", bool((p["bound0"] & (p["sigma0"] == 1)).any())),
                     ("bound0_off_anchor", bool((p["bound0"] & ~mask[p["pos0"]]).any())),
                     ("table", case["table"] is not None), ("polarised", N > 0 and abs(int(p["sigma0"].sum())) == N and N > 1),
                     ("four_wavefronts", N > 1024)):
        if on:
            f.add(name)
    if mask.any():
        for k in ("k_on", "k_off", "k_exit"):
            if kw[k] == 0.0:
                f.add(k + "=0")
    if case["table"] is not None:
        f.add(f"flip_n={case['table'][1]}")
    return f


def raw_keywords(case, sigma=True):
    """The keywords the raw entry points of gillespie.py share, for `case` (without states, betas, times and uniforms)."""
    P = prepared(case)["orc"].par
    kw = dict(L=P.L, K=P.K, periodic=P.periodic, rate_diffusion=P.rate_diffusion, rate_active=P.rate_active,
              minus_anchor=P.minus_anchor, immobilize=P.immobilize_when_anchored, suppress_flip=P.suppress_flip_when_bound,
              crowding=P.crowding_suppresses_rates, k_on=P.k_on, k_off=P.k_off, k_exit=P.k_exit, anchor_mask=P.is_anchor_site,
              flip_table=prepared(case)["flip_table"])
    if sigma:
        kw["sigma_grid"] = P.sigma_grid if P.sigma_kernel > 0 else 0.0
    return kw
