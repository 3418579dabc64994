"""ORACLE (test infrastructure): the random streams of the device's exact event loop and of the PDE tracers, on the CPU.

Plain NumPy, written from the Random123 definition of Philox4x32-10 (Salmon et al., SC'11) and from the layouts that
include/gillespie.h, include/gillespie_many.h, include/gillespie_mixed.h and include/pde.h promise -- not from the kernels.
A table built here and handed to an entry point as `uniforms` (or `rand_u` / `rand_n`) must reproduce the seeded run of
that entry point; tests/test_gpu_exact_loop_streams.py and tests/test_gpu_pde_streams.py hold the kernels to that.

Only tests/ may import this module."""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57                # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85                # Weyl increments of the key (golden ratio, sqrt(3) - 1)
MASK32, MASK64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF

EXACT_LOOP_DOMAIN_A = 0x47494C31               # counter word 3 of an event's first block: waiting time, particle
EXACT_LOOP_DOMAIN_B = 0x47494C32               # ... of its second block: channel, left / right
PDE_TRACER_DOMAIN = 0x7AC3                     # counter word 3 of the PDE tracer noise


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32 with ten rounds, vectorised: the six arguments broadcast against each other, each taken mod 2^32.
    Returns uint32 [..., 4]."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & np.uint64(MASK32) for v in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    m32, sh = np.uint64(MASK32), np.uint64(32)
    for r in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2            # 32 x 32 -> 64 bit products: no overflow in uint64
        ka, kb = (k0 + np.uint64(r * W0)) & m32, (k1 + np.uint64(r * W1)) & m32
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ ka, p1 & m32, (p0 >> sh) ^ c3 ^ kb, p0 & m32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def uniform53(a, b):
    """Two 32-bit words -> a binary64 in [0, 1) on the grid 2^-53: the top 27 bits of a above the top 26 bits of b."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return ((a >> np.uint64(5)) * np.uint64(1 << 26) + (b >> np.uint64(6))).astype(np.float64) * 2.0 ** -53


def split_key(key):
    """A 64-bit key -> its (low, high) 32-bit words."""
    key = int(key) & MASK64
    return key & MASK32, key >> 32


def exact_loop_words(key, stream, n_events, first_event=0):
    """The eight Philox words of events first_event .. first_event + n_events - 1: uint32 [n_events, 8] = x0..x3 of the
    counter (e & 0xFFFFFFFF, e >> 32, stream, 0x47494C31), then y0..y3 of (..., 0x47494C32), under the key (key & 0xFFFFFFFF, key >> 32)."""
    e = np.arange(int(first_event), int(first_event) + int(n_events), dtype=np.uint64)
    lo, hi = e & np.uint64(MASK32), e >> np.uint64(32)
    k0, k1 = split_key(key)
    st = int(stream) & MASK32
    x = philox4x32_10(lo, hi, st, EXACT_LOOP_DOMAIN_A, k0, k1)
    y = philox4x32_10(lo, hi, st, EXACT_LOOP_DOMAIN_B, k0, k1)
    return np.concatenate([x, y], axis=-1)


def uniforms_from_words(w):
    """uint32 [..., 8] -> float64 [..., 4]: (waiting time u0, particle u1, channel u2, left / right u3)."""
    w = np.asarray(w)
    return np.stack([uniform53(w[..., 0], w[..., 1]), uniform53(w[..., 2], w[..., 3]),
                     uniform53(w[..., 4], w[..., 5]), uniform53(w[..., 6], w[..., 7])], axis=-1)


def exact_loop_uniforms(key, stream, n_events, first_event=0):
    """The table a seeded exact-loop system draws: float64 [n_events, 4], row e = the four numbers of event e.  Column 0 is the
    uniform u0 itself; the kernel forms the waiting time -log1p(-u0) / R from it."""
    return uniforms_from_words(exact_loop_words(key, stream, n_events, first_event))


def pde_tracer_noise(key, system, nsteps, n_tracers):
    """(rand_u, rand_n), each float64 [nsteps + 1, n_tracers]: tracer i of system `system` at step n draws from the counter
    (n, i, system, 0x7AC3); u = uniform53(x0, x1), g = the cosine branch of Box-Muller on ((x2 + 1/2) 2^-32, (x3 + 1/2) 2^-32)."""
    n = np.arange(int(nsteps) + 1, dtype=np.uint64)[:, None]
    i = np.arange(int(n_tracers), dtype=np.uint64)[None, :]
    k0, k1 = split_key(key)
    x = philox4x32_10(n, i, int(system) & MASK32, PDE_TRACER_DOMAIN, k0, k1)
    u = uniform53(x[..., 0], x[..., 1])
    r1 = (x[..., 2].astype(np.float64) + 0.5) * 2.0 ** -32
    r2 = (x[..., 3].astype(np.float64) + 0.5) * 2.0 ** -32
    return u, np.sqrt(-2.0 * np.log(r1)) * np.cos(2.0 * np.pi * r2)


# ---- which key and stream a system of each entry point draws with (the table of the headers)

def batch_stream(seed, s):
    """gil_run_batch and its structure / capture / profile forms: key = seed, stream = s."""
    return int(seed) & MASK64, int(s)


def large_stream(seed):
    """gil_run_large: key = seed, stream = 0."""
    return int(seed) & MASK64, 0


def many_large_stream(seed, s):
    """gilm_run: key = (seed + s) mod 2^64, stream = 0."""
    return (int(seed) + int(s)) & MASK64, 0


def mixed_stream(seeds, streams, s):
    """gilx_run, gilxs_run: key = seed[s], stream = stream[s]."""
    return int(seeds[s]) & MASK64, int(streams[s])
