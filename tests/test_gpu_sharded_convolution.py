"""GPU suite: site-sharded tiles handles that update the field by the exact convolution (csrc/ntt_conv.hpp on a window per
rank, overlap-save).  A rank transforms [own_lo - Rt - 2, own_hi + Rt + 2): its own deposits plus the coefficient slices its
neighbours send with the halo (ADDED on arrival), and keeps {W, S} of [own_lo - 2, own_hi + 2).  Ranks are emulated with one
handle each on one device (aps_propose -> aps_halo_copy -> aps_commit) or run as real processes (aps_step, peer stores); the
merged result must equal a single handle, and where the size allows the oracle, bit for bit."""
import importlib
import os
import sys

import numpy as np
import pytest

from oracle.gillespie_numpy import LatticeGasParams
from oracle import sync_oracle as so

pytestmark = pytest.mark.gpu
PKG = "hydrodynamic-limits-of-active-particle-systems-with-mean-field-interactions_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 2                                                           # halo sites whose {W, S} a rank keeps either side


@pytest.fixture(scope="module")
def capi():
    mod = importlib.import_module(PKG + ".capi")
    assert mod.device_count() >= 1, "no GPU visible"
    return mod


def _params(L, K=1, sigma=0.002, periodic=False, **kw):
    base = dict(xlim=1.0, rate_diffusion=3.0, rate_active=4.0, beta=1.1, scale_rates=False)
    base.update(kw)
    return LatticeGasParams.from_kwargs(L=L, local_kernel_sigma=sigma, periodic=periodic, site_capacity=K, **base)


def _handle(capi, par, n, rank=0, world=1, ntt=None, **kw):
    if ntt is not None:
        os.environ["APS_NTT"] = ntt
    try:
        return capi.Handle(L=par.L, K=par.K, periodic=par.periodic, sigma_grid=par.sigma_grid, rate_diffusion=par.rate_diffusion,
                           rate_active=par.rate_active, beta=[par.beta], dt=0.04, seed=31, n_particles=n, minus_anchor=par.minus_anchor,
                           immobilize=par.immobilize_when_anchored, suppress_flip=par.suppress_flip_when_bound, k_on=par.k_on,
                           k_off=par.k_off, k_exit=par.k_exit, anchor_mask=par.is_anchor_site, rank=rank, world=world, method="tiles", **kw)
    finally:
        if ntt is not None:
            del os.environ["APS_NTT"]


def _random_state(rng, L, N, K):
    pos = rng.permutation(rng.choice(np.repeat(np.arange(L), K), size=N, replace=False)).astype(np.int32)
    return pos, rng.choice(np.array([1, -1], np.int8), size=N)


def _neighbours(r, world, periodic):
    return sorted({(r - 1) % world, (r + 1) % world} if periodic else {q for q in (r - 1, r + 1) if 0 <= q < world})


def _emulated_step(ranks, periodic):
    world = len(ranks)
    for h in ranks:
        h.propose()
    for r, h in enumerate(ranks):
        for q in _neighbours(r, world, periodic):
            h.halo_from(ranks[q])
    for h in ranks:
        h.commit()


def _merged_state(ranks, n):
    pos, spin, bound, alive = np.zeros(n, np.int32), np.zeros(n, np.int8), np.zeros(n, np.uint8), np.full(n, 255, np.uint8)
    seen = np.zeros(n, int)
    for h in ranks:
        p, s, b, a = h.get_state()
        mine = a != 2
        pos[mine], spin[mine], bound[mine], alive[mine] = p[mine], s[mine], b[mine], a[mine]
        seen += mine
    return pos, spin, bound, alive, seen


def _check_own_sites(ranks, single):
    Ws, Ss, occs = single.get_lattice()
    for h in ranks:
        lo, hi = h.owned_sites()
        W, S, occ = h.get_lattice()
        assert np.array_equal(W[lo:hi], Ws[lo:hi]) and np.array_equal(S[lo:hi], Ss[lo:hi]) and np.array_equal(occ[lo:hi], occs[lo:hi]), (lo, hi)


def _assert_convolution_ranks(ranks, par):
    Rt = len(ranks[0].table()[0]) - 1
    for h in ranks:
        info = h.ntt_info()
        lo, hi = h.owned_sites()
        assert info["on"] and h.halo_info()[0] == 1, info
        assert 14 <= info["log2_m"] <= 21 and (1 << info["log2_m"]) >= (hi - lo) + 2 * (Rt + G), info
    return Rt


EMULATED = [
    dict(world=2, periodic=False, fp32=True, L=8000, K=2, extras=True),
    dict(world=3, periodic=True, fp32=True, L=12000, K=1, extras=False),
    dict(world=4, periodic=False, fp32=False, L=16000, K=2, extras=False),
    dict(world=3, periodic=True, fp32=False, L=15000, K=2, extras=True),
]


@pytest.mark.parametrize("case", EMULATED, ids=["walls_i32_w2_anchors_exits", "torus_i32_w3", "walls_f64_w4", "torus_f64_w3_anchors_exits"])
def test_emulated_ranks_convolution_equal_single_handle_and_oracle(capi, case):
    """APS_NTT=1: every rank of a site-sharded handle takes the convolution with one exchange per step.  After every block of
    steps the merged state equals the single handle and the oracle; {W, S, occupancy} on the own sites equal the single handle's;
    the exit logs add up.  The first commit is tried before the halo arrived: it is refused, and the retry gives the same bits."""
    world, periodic, fp32, L, K = case["world"], case["periodic"], case["fp32"], case["L"], case["K"]
    extra = dict(anchor_positions=[0.1, 0.45, 0.8], anchor_radius=0.02, k_on=2.0, k_off=1.0, k_exit=0.6) if case["extras"] else {}
    par = _params(L, K=K, periodic=periodic, **extra)
    rng = np.random.default_rng(5 + world)
    N = int(0.4 * L * K)
    pos, spin = _random_state(rng, L, N, K)
    orc = so.SyncOracle(par, dt=0.04, seed=31, **(dict(sum_bits=29) if fp32 else {}))
    orc.set_state(pos, spin)
    ranks = [_handle(capi, par, N, rank=r, world=world, ntt="1", fp32=fp32) for r in range(world)]
    single = _handle(capi, par, N, ntt="1", fp32=fp32)
    try:
        _assert_convolution_ranks(ranks, par)
        for h in ranks + [single]:
            h.set_state(pos, spin)
        for block, n in enumerate((1, 9, 20, 20)):
            for i in range(n):
                if block == 0:                                     # a commit before the halo: refused, nothing launched
                    for h in ranks:
                        h.propose()
                    with pytest.raises(capi.ApsError):
                        ranks[0].commit()
                    for r, h in enumerate(ranks):
                        for q in _neighbours(r, world, periodic):
                            h.halo_from(ranks[q])
                    for h in ranks:
                        h.commit()
                else:
                    _emulated_step(ranks, periodic)
            single.step(n)
            orc.run(n)
            p, s, b, a, seen = _merged_state(ranks, N)
            assert np.array_equal(seen, np.ones(N, int)), block
            for x, y in zip((p, s, b, a), single.get_state()):
                assert np.array_equal(x, y), block
            assert np.array_equal(p, orc.pos) and np.array_equal(s, orc.spin) and np.array_equal(b, orc.bound) and np.array_equal(a, orc.alive), block
            _check_own_sites(ranks, single)
        assert (p != pos).mean() > 0.3
        ex = np.concatenate([h.exits() for h in ranks])
        ex = ex[np.lexsort((ex[:, 2], ex[:, 0]))]
        assert np.array_equal(ex, single.exits()) and np.array_equal(ex, orc.exits())
        if case["extras"]:
            assert len(ex) > 0 and b.any()
    finally:
        for h in ranks + [single]:
            h.close()


def test_table_beyond_lds_takes_the_convolution_by_default(capi):
    """A table beyond LDS (about 42 000 taps) at moderate L, 32-bit field, three ranks between walls, no APS_NTT: the library
    picks the convolution on every rank (and on the single handle), the results are bit-equal to the single handle."""
    L, N, world, nsteps = 300000, 90000, 3, 24
    par = _params(L, K=1, sigma=0.035, rate_diffusion=0.5, rate_active=5.0)
    rng = np.random.default_rng(41)
    pos = rng.choice(L, size=N, replace=False).astype(np.int32)
    spin = rng.choice(np.array([1, -1], np.int8), size=N)
    ranks = [_handle(capi, par, N, rank=r, world=world, fp32=True) for r in range(world)]
    single = _handle(capi, par, N, fp32=True)
    try:
        assert not ranks[0].tiles_info()["table_in_lds"] and single.ntt_info()["on"]
        Rt = _assert_convolution_ranks(ranks, par)
        assert Rt > 30000
        for h in ranks + [single]:
            h.set_state(pos, spin)
        for n in (5, nsteps - 5):
            for _ in range(n):
                _emulated_step(ranks, False)
            single.step(n)
            p, s, b, a, seen = _merged_state(ranks, N)
            assert np.array_equal(seen, np.ones(N, int))
            for x, y in zip((p, s, b, a), single.get_state()):
                assert np.array_equal(x, y)
            _check_own_sites(ranks, single)
    finally:
        for h in ranks + [single]:
            h.close()


def test_config5_as_eight_site_ranges(capi):
    """BASELINE config 5 (N = 1e6, L = 2e6, 32-bit field, 40 001-tap table) as eight site ranges on one device, every rank by the
    convolution on its own window: merged state and {W, S, occupancy} on the own sites equal the single handle after 20 steps
    (the single handle takes the convolution too and is pinned to the oracle by test_fp32_config5_scale_against_oracle_windows)."""
    L, N, world, nsteps = 2_000_000, 1_000_000, 8, 20
    par = LatticeGasParams.from_kwargs(L=L, xlim=1.0, rate_diffusion=0.02, rate_active=5.0, beta=0.7,
                                       scale_rates=False, local_kernel_sigma=0.005, site_capacity=1)
    rng = np.random.default_rng(12)
    pos = rng.choice(L, size=N, replace=False).astype(np.int32)
    spin = rng.choice(np.array([1, -1], np.int8), size=N)
    ranks = [_handle(capi, par, N, rank=r, world=world, fp32=True) for r in range(world)]
    single = _handle(capi, par, N, fp32=True)
    try:
        assert single.ntt_info()["on"]
        _assert_convolution_ranks(ranks, par)
        assert all(h.ntt_info()["log2_m"] == 19 for h in ranks)
        for h in ranks + [single]:
            h.set_state(pos, spin)
        for _ in range(nsteps):
            _emulated_step(ranks, False)
        single.step(nsteps)
        p, s, b, a, seen = _merged_state(ranks, N)
        assert np.array_equal(seen, np.ones(N, int))
        for x, y in zip((p, s, b, a), single.get_state()):
            assert np.array_equal(x, y)
        assert (p != pos).mean() > 0.05
        _check_own_sites(ranks, single)
    finally:
        for h in ranks + [single]:
            h.close()


def test_halo_rules_of_convolution_ranks(capi):
    """An explicit halo interval k > 1 keeps the sweep; the library's choice (0) and k = 1 take the convolution with one exchange
    per step; the blocks a rank sends are the sizes its neighbours expect (3 sites of cells + Rt + 3 coefficients of c_W and c_S)."""
    L, K, world = 9000, 2, 3
    par = _params(L, K=K)
    N = 6000
    for k, on in ((3, False), (1, True), (0, True)):
        ranks = [_handle(capi, par, N, rank=r, world=world, ntt="1", fp32=True, halo_interval=k) for r in range(world)]
        try:
            assert all(h.ntt_info()["on"] == on for h in ranks), k
            assert all(h.halo_info()[0] == (k if k else 1) for h in ranks) if on else all(h.halo_info()[0] == 3 for h in ranks)
            sizes = [h.halo_sizes() for h in ranks]
            for r in range(world - 1):                           # rank r's last block -> r + 1, rank r + 1's first block -> r
                assert sizes[r][0][1] == sizes[r + 1][1][1] > 0 and sizes[r + 1][0][0] == sizes[r][1][0] > 0
            assert sizes[0][0][0] == sizes[0][1][1] == 0 and sizes[-1][0][1] == sizes[-1][1][0] == 0
            if on:
                Rt = len(ranks[0].table()[0]) - 1
                cells, coef = -(-3 * K * 4 // 16) * 16, -(-(Rt + G + 1) * 4 // 16) * 16
                assert sizes[1][0][0] == sizes[1][0][1] == cells + 2 * coef
        finally:
            for h in ranks:
                h.close()


def test_a_block_is_added_once_per_step(capi):
    """Received coefficients are ADDED, so a second delivery of the same block in one step is refused (aps_halo_copy and
    aps_halo_unpack) instead of counting them twice; after the refusals the step commits and stays bit-equal to the single handle."""
    L, K, world = 9000, 2, 2
    par = _params(L, K=K, periodic=True)
    rng = np.random.default_rng(3)
    N = 6000
    pos, spin = _random_state(rng, L, N, K)
    ranks = [_handle(capi, par, N, rank=r, world=world, ntt="1", fp32=True) for r in range(world)]
    single = _handle(capi, par, N, ntt="1", fp32=True)
    try:
        assert all(h.ntt_info()["on"] for h in ranks)
        for h in ranks + [single]:
            h.set_state(pos, spin)
        for step in range(6):
            for h in ranks:
                h.propose()
            if step % 2 == 0:                                    # both blocks of the torus neighbour by device copy
                ranks[0].halo_from(ranks[1])
                with pytest.raises(capi.ApsError):
                    ranks[0].halo_from(ranks[1])
                ranks[1].halo_from(ranks[0])
            else:                                                # the same blocks as host bytes
                for dst, src in ((ranks[0], ranks[1]), (ranks[1], ranks[0])):
                    blocks = [src.halo_pack(0), src.halo_pack(1)]
                    dst.halo_unpack(1, blocks[1])                # the left neighbour's last block
                    with pytest.raises(capi.ApsError):
                        dst.halo_unpack(1, blocks[1])
                    dst.halo_unpack(0, blocks[0])                # the right neighbour's first block
            for h in ranks:
                h.commit()
        single.step(6)
        p, s, b, a, seen = _merged_state(ranks, N)
        assert np.array_equal(seen, np.ones(N, int))
        for x, y in zip((p, s, b, a), single.get_state()):
            assert np.array_equal(x, y)
        _check_own_sites(ranks, single)
    finally:
        for h in ranks + [single]:
            h.close()


def _sharded_conv_worker(rank, world, periodic, port, out_dir):
    """One process per rank on device 0, APS_NTT=1, stepping through aps_step with the halo moved by peer stores."""
    sys.path.insert(0, ROOT)
    os.environ["APS_NTT"] = "1"
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        capi = importlib.import_module(PKG + ".capi")
        par, pos, spin = _process_case(periodic)
        h = _handle(capi, par, len(pos), rank=rank, world=world, fp32=True)
        assert h.ntt_info()["on"] and h.halo_info()[0] == 1
        h.set_state(pos, spin)
        blobs = [None] * world
        dist.all_gather_object(blobs, h.ipc_export())
        left, right = (rank - 1) % world, (rank + 1) % world
        if not periodic:
            left, right = (left if rank > 0 else None), (right if rank < world - 1 else None)
        h.ipc_connect(None if left is None else blobs[left], None if right is None else blobs[right])
        assert h.exchange_kind() == "ipc-peer"
        for n in (1, 6, 2, 21):
            h.step(n)
        p, s, b, a = h.get_state()
        lo, hi = h.owned_sites()
        W, S, occ = h.get_lattice()
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), pos=p, spin=s, bound=b, alive=a, exits=h.exits(), lo=lo, hi=hi, W=W, S=S, occ=occ)
        dist.barrier()                                         # nobody frees a landing buffer a neighbour may still be writing to
        h.close()
    finally:
        dist.destroy_process_group()


def _process_case(periodic):
    par = _params(9000, K=2, periodic=periodic, anchor_positions=[0.3, 0.6], anchor_radius=0.02, k_on=2.0, k_off=1.0, k_exit=0.5)
    rng = np.random.default_rng(29)
    pos, spin = _random_state(rng, 9000, 7000, 2)
    return par, pos, spin


@pytest.mark.parametrize("world,periodic", [(2, True), (3, False)], ids=["torus_w2", "walls_w3"])
def test_convolution_ranks_across_processes_by_peer_stores(tmp_path, capi, world, periodic):
    """Real processes on one GPU, each a site range taking the convolution, stepped by aps_step calls of various lengths with the
    production transport (peer stores into the neighbour process's landing buffer, coefficients added on arrival): the merged
    state, the exit log and {W, S, occupancy} on the own sites equal a single handle's after 30 steps."""
    pytest.importorskip("torch")
    import torch.multiprocessing as mp
    port = 35300 + (os.getpid() % 1500) + 17 * world
    mp.spawn(_sharded_conv_worker, args=(world, periodic, port, str(tmp_path)), nprocs=world, join=True)
    par, pos, spin = _process_case(periodic)
    single = _handle(capi, par, len(pos), fp32=True)
    try:
        single.set_state(pos, spin)
        single.step(30)
        want, want_exits = single.get_state(), single.exits()
        Ws, Ss, occs = single.get_lattice()
    finally:
        single.close()
    n = len(pos)
    seen, exits = np.zeros(n, int), []
    merged = [np.zeros(n, np.int32), np.zeros(n, np.int8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)]
    for r in range(world):
        got = np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))
        mine = got["alive"] != 2
        seen += mine
        for m, key in zip(merged, ("pos", "spin", "bound", "alive")):
            m[mine] = got[key][mine]
        lo, hi = int(got["lo"]), int(got["hi"])
        assert np.array_equal(got["W"][lo:hi], Ws[lo:hi]) and np.array_equal(got["S"][lo:hi], Ss[lo:hi]) and np.array_equal(got["occ"][lo:hi], occs[lo:hi])
        exits.append(got["exits"])
    assert np.array_equal(seen, np.ones(n, int))
    for m, w in zip(merged, want):
        assert np.array_equal(m, w)
    ex = np.concatenate(exits)
    assert np.array_equal(ex[np.lexsort((ex[:, 2], ex[:, 0]))], want_exits)
