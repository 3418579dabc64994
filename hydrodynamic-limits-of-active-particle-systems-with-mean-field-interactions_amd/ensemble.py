"""Batched beta sweeps: the reference's `sweep_beta_ensemble` / `sweep_over_betas` loops
(PARTICLE_solver_BIOLOGY_EXCLUSION_sweep_beta.py:56-117, :828-1028) with every (beta, run) pair stepped
together as independent ensembles of one GPU handle, and the per-run observables of observables.py.
The two outer sweeps of the other drivers are here too: `sweep_over_sigmas` (interaction range,
..._sweep_beta_2.py:1030-1075) and `sweep_over_densities` (particle number x beta, ..._double_sweep.py:851-861) --
one batched handle per sigma / per particle number (the weight table and the state capacity differ), all (beta, run)
pairs inside it; under the exact dynamics `one_launch=True` puts the whole sweep into ONE mixed launch of the event loop
(include/gillespie_mixed.h: a weight table and a blocking table per system; with `allow_large=True` also at L > 4096 or
N > 2048, include/gillespie_mixed_many.h).  `sweep_betas_for_structures` / `sweep_beta_structure_ensemble` are the pattern study's drivers
(PARTICLE_solver_BIOLOGY_local_structure.py:105-193), all (beta, run) pairs in one launch, the per-run observables from sums
taken on the GPU; `sweep_sigmas_for_structures` is that study over the interaction range, all (sigma, beta, run) systems in one mixed
launch with the window reduction on the device (include/gillespie_mixed_structure.h).  `capture_study` is the anchor-capture study (PARTICLE_solver_CLASS.py:766-976) as an ensemble in one launch.
`profile_sweep` gives the ensemble density and field profiles per beta (the means over runs of rho_plus_list, rho_minus_list,
m_local_list, PARTICLE_solver_CLASS.py:205-213), all (beta, run) pairs in one launch and summed over the runs on the GPU;
`profile_sweep_over_sigmas` and `profile_sweep_over_densities` are that study over the interaction range and over the particle
number, all systems in ONE mixed launch of either shape (include/gillespie_mixed_profile.h)."""
from __future__ import annotations

import warnings

import numpy as np

from . import observables
from .particle_system import ParticleSystem, run_batched, run_batched_statistics


def sweep_over_betas(beta_values, n_runs_per_beta=10, ps_kwargs=None, init_kwargs=None, run_kwargs=None,
                     rng_seeds=None, keep_outputs=False, on_device=False, dynamics=None, obs_per_launch=None):
    """Returns a dict with the keys the reference saves (`beta_values, means, stds, ses, D_means, D_ses, m_means,
    m_stds, m_ses, rho_means, rho_ses, block_means, block_ses`, ..._sweep_beta.py:952-968) plus `raw_by_beta`.
    `rng_seeds[b][r]` seeds the initial condition of run r at beta b (None: unseeded, like the reference).
    `on_device=True` evaluates the observables from integer sums taken on the GPU at each observation time
    (run_batched_statistics; needs k_exit = 0) instead of from the M x L arrays of `run()`; `run_kwargs` may then
    only hold T and obs_dt.  `dynamics="exact"` runs the reference's event-by-event dynamics resident on the GPU
    (gillespie.run_batched_exact / run_batched_exact_statistics), `"sync"` the fixed-dt scheme; the default follows
    ParticleSystem's: exact unless `ps_kwargs` asks for the stepper (`dt` or `mode="sync"`).  `obs_per_launch=n` (exact
    dynamics only): the runs as a chain of launches of at most n observations each instead of one persistent launch
    (gillespie.run_batched_exact: the same numbers, bit for bit)."""
    ps_kwargs, init_kwargs, run_kwargs = dict(ps_kwargs or {}), dict(init_kwargs or {}), dict(run_kwargs or {})
    if dynamics is None:
        dynamics = "sync" if (ps_kwargs.get("dt") is not None or ps_kwargs.get("mode") == "sync") else "exact"
    if obs_per_launch is not None and dynamics != "exact":
        raise ValueError("obs_per_launch needs the exact dynamics; the fixed-dt stepper has no checkpointed launch")
    chain = {} if obs_per_launch is None else {"obs_per_launch": obs_per_launch}
    systems, owner = [], []
    for bi, beta in enumerate(beta_values):
        for r in range(n_runs_per_beta):
            rng = None if rng_seeds is None else np.random.default_rng(int(rng_seeds[bi][r]))
            systems.append(ParticleSystem(beta=beta, rng=rng, **ps_kwargs, **init_kwargs))
            owner.append(bi)
    if dynamics not in ("sync", "exact"):
        raise ValueError("dynamics must be 'sync' or 'exact'")
    if on_device:
        if keep_outputs:
            raise ValueError("on_device=True keeps no per-run outputs")
        outs = None
        slim = {k: v for k, v in run_kwargs.items() if k in ("T", "obs_dt")}
        if dynamics == "exact":
            from .gillespie import run_batched_exact_statistics
            rows = run_batched_exact_statistics(systems, **slim, **chain)
        else:
            rows = run_batched_statistics(systems, **slim)
    elif dynamics == "exact":
        from .gillespie import run_batched_exact
        outs = run_batched_exact(systems, want_m_local=False, **run_kwargs, **chain)
        rows = [observables.run_observables(out, ps.L, ps.dx) for ps, out in zip(systems, outs)]
    else:
        outs = run_batched(systems, **run_kwargs)
        rows = [observables.run_observables(out, ps.L, ps.dx) for ps, out in zip(systems, outs)]
    out = _beta_statistics(rows, owner, beta_values)
    if keep_outputs:
        out["outs"] = outs
    return out


def _beta_statistics(rows, owner, beta_values):
    """The per-beta reduction of sweep_over_betas over the per-run rows; owner[i] is the beta index of rows[i]."""
    res = {k: [] for k in ("means", "stds", "ses", "D_means", "D_ses", "m_means", "m_stds", "m_ses", "rho_means", "rho_ses",
                           "block_means", "block_ses", "raw_by_beta")}
    for bi in range(len(beta_values)):
        st = observables.ensemble_statistics([row for row, o in zip(rows, owner) if o == bi])
        for src, dst in (("mean", "means"), ("std", "stds"), ("se", "ses"), ("D_mean", "D_means"), ("D_se", "D_ses"),
                         ("m_mean", "m_means"), ("m_std", "m_stds"), ("m_se", "m_ses"), ("rho_mean", "rho_means"),
                         ("rho_se", "rho_ses"), ("block_mean", "block_means"), ("block_se", "block_ses"), ("v_array", "raw_by_beta")):
            res[dst].append(st[src])
    out = {k: (np.array(v) if k != "raw_by_beta" else v) for k, v in res.items()}
    out["beta_values"] = np.asarray(beta_values, dtype=float)
    return out


def _chain_keywords(who, one_launch, stepper, obs_per_launch, resume, return_checkpoint):
    """The keywords a sweep passes on to its mixed launch for a run in segments (gillespie.MixedCheckpoint), or ValueError where
    there is no such launch: `stepper` (the fixed-dt dynamics), or a sweep that is not one launch."""
    given = [k for k, v in (("obs_per_launch", obs_per_launch), ("resume", resume), ("return_checkpoint", return_checkpoint or None)) if v is not None]
    if not given:
        return {}
    if stepper:
        raise ValueError(f"{given[0]} needs the exact dynamics; the fixed-dt stepper has no checkpointed launch")
    if not one_launch:
        raise ValueError(f"{who}: {given[0]} needs one_launch=True; the loop of one launch per case has no common checkpoint")
    return dict(obs_per_launch=obs_per_launch, resume=resume, return_checkpoint=bool(return_checkpoint))


def _is_stepper(ps_kwargs, dynamics):
    ps_kwargs = ps_kwargs or {}
    return dynamics == "sync" or (dynamics is None and (ps_kwargs.get("dt") is not None or ps_kwargs.get("mode") == "sync"))


def _sweeps_in_one_launch(who, cases, beta_values, n_runs_per_beta, run_kwargs, rng_seeds, on_device, dynamics, allow_large=False, chain=None):
    """One sweep_over_betas per case = (ps_kwargs, init_kwargs), all cases in ONE mixed launch of the exact event loop
    (gillespie.run_batched_exact_statistics_mixed / run_batched_exact_mixed).  The systems are built in the order of the host
    loop, and every case is a group of the launch: its systems draw what the case's own launch draws.  Returns the list of the
    per-case sweep dictionaries.  ValueError where no mixed launch exists: the fixed-dt stepper, a large shape (L > 4096 or
    N > 2048) without `allow_large`, a launch over the 160 KB of LDS.  `chain` (_chain_keywords): the launch in segments; with
    its return_checkpoint the result is (the list, the MixedCheckpoint)."""
    from . import gillespie
    run_kwargs, chain = dict(run_kwargs or {}), dict(chain or {})
    for ps_kwargs, _ in cases:
        d = dynamics
        if d is None:
            d = "sync" if (ps_kwargs.get("dt") is not None or ps_kwargs.get("mode") == "sync") else "exact"
        if d not in ("sync", "exact"):
            raise ValueError("dynamics must be 'sync' or 'exact'")
        if d != "exact":
            raise ValueError(f"{who}: one_launch=True needs the exact dynamics; the fixed-dt stepper has no mixed launch")
    systems, group, owner = [], [], []
    for ci, (ps_kwargs, init_kwargs) in enumerate(cases):
        for bi, beta in enumerate(beta_values):
            for r in range(n_runs_per_beta):
                rng = None if rng_seeds is None else np.random.default_rng(int(rng_seeds[bi][r]))
                systems.append(ParticleSystem(beta=beta, rng=rng, **ps_kwargs, **init_kwargs))
                group.append(ci)
                owner.append(bi)
    if on_device:
        slim = {k: v for k, v in run_kwargs.items() if k in ("T", "obs_dt")}
        rows = gillespie.run_batched_exact_statistics_mixed(systems, groups=group, allow_large=allow_large, **slim, **chain)
    else:
        rows = gillespie.run_batched_exact_mixed(systems, want_m_local=False, groups=group, allow_large=allow_large, **run_kwargs, **chain)
    ck = None
    if chain.get("return_checkpoint"):
        rows, ck = rows
    if not on_device:
        rows = [observables.run_observables(out, ps.L, ps.dx) for ps, out in zip(systems, rows)]
    per = len(beta_values) * n_runs_per_beta
    sweeps = [_beta_statistics(rows[ci * per:(ci + 1) * per], owner[ci * per:(ci + 1) * per], beta_values) for ci in range(len(cases))]
    return (sweeps, ck) if chain.get("return_checkpoint") else sweeps


def sweep_beta_ensemble(beta, n_runs=10, ps_kwargs=None, init_kwargs=None, run_kwargs=None, rng_seeds=None):
    """One beta, n_runs batched runs; same return tuple as the reference function (:117)."""
    r = sweep_over_betas([beta], n_runs, ps_kwargs, init_kwargs, run_kwargs,
                         None if rng_seeds is None else [rng_seeds], keep_outputs=True)
    return (float(r["means"][0]), float(r["stds"][0]), float(r["ses"][0]), r["raw_by_beta"][0], r["outs"],
            float(r["m_means"][0]), float(r["m_stds"][0]), float(r["m_ses"][0]), float(r["rho_means"][0]),
            float(r["rho_ses"][0]), float(r["block_means"][0]), float(r["block_ses"][0]), float(r["D_means"][0]),
            float(r["D_ses"][0]))


def sweep_over_sigmas(sigma_values, beta_values, n_runs_per_beta=5, ps_kwargs=None, init_kwargs=None, run_kwargs=None,
                      rng_seeds=None, on_device=False, dynamics=None, one_launch=False, allow_large=False, obs_per_launch=None,
                      resume=None, return_checkpoint=False):
    """The sigma sweep of PARTICLE_solver_BIOLOGY_EXCLUSION_sweep_beta_2.py:1030-1075: for every interaction range
    `local_kernel_sigma` a whole beta sweep (one GPU handle per sigma: the weight table changes; sigma = 0 selects the global
    mean field, sigma wider than the box the folded table).  Returns {sigma: {"beta", "v_mean", "v_se", "D_mean", "D_se",
    "ps_kwargs"}} like the reference (which also writes one .npz per sigma; saving is left to the caller).
    `one_launch=True` (exact dynamics only): all (sigma, beta, run) systems in one mixed launch, with the draws and hence the
    numbers of the loop over sigma; ValueError for the fixed-dt stepper, a large shape or a launch over the LDS limit.
    `allow_large=True` (with one_launch): a large shape (L > 4096 or N > 2048) is one mixed launch of the large-system kernel
    (include/gillespie_mixed_many.h) instead of a ValueError.  Its numbers equal the host loop's where every case of the sweep is
    itself a large shape, which is always so when L > 4096; cases below the limit in a sweep that straddles it run on the large
    kernel with its keys and equal gillespie.run_many_large_raw for them, not the batch kernel.
    `obs_per_launch=n`, `resume=MixedCheckpoint`, `return_checkpoint=True` (with one_launch, exact dynamics): the one launch as a
    chain of launches of at most n observations, started from a checkpoint of the same sweep, and returning (results, checkpoint)
    (gillespie.run_batched_exact_mixed); the numbers are the one launch's, bit for bit.  ValueError without one_launch or under
    the fixed-dt stepper."""
    results = {}
    kws = [dict(ps_kwargs or {}, local_kernel_sigma=float(sigma)) for sigma in sigma_values]
    chain = _chain_keywords("sweep_over_sigmas", one_launch, _is_stepper(ps_kwargs, dynamics), obs_per_launch, resume, return_checkpoint)
    if one_launch:
        sweeps = _sweeps_in_one_launch("sweep_over_sigmas", [(kw, dict(init_kwargs or {})) for kw in kws], beta_values, n_runs_per_beta,
                                       run_kwargs, rng_seeds, on_device, dynamics, allow_large, chain)
        if return_checkpoint:
            sweeps, ck = sweeps
    for si, (sigma, kw) in enumerate(zip(sigma_values, kws)):
        r = sweeps[si] if one_launch else sweep_over_betas(beta_values, n_runs_per_beta, kw, init_kwargs, run_kwargs, rng_seeds,
                                                           on_device=on_device, dynamics=dynamics)
        results[sigma] = {"beta": np.asarray(beta_values, dtype=float), "v_mean": r["means"], "v_se": r["ses"], "D_mean": r["D_means"],
                          "D_se": r["D_ses"], "m_mean": r["m_means"], "block_mean": r["block_means"], "ps_kwargs": kw}
    return (results, ck) if return_checkpoint else results


def sweep_over_densities(n_part_values, beta_values, n_runs_per_beta=4, ps_kwargs=None, init_kwargs=None, run_kwargs=None,
                         rng_seeds=None, on_device=False, dynamics=None, one_launch=False, allow_large=False, obs_per_launch=None,
                         resume=None, return_checkpoint=False):
    """The density x beta double sweep of PARTICLE_solver_BIOLOGY_EXCLUSION_double_sweep.py:851-861
    (`list_N_part = np.linspace(50, 950, 19)`: N arrives as a float there and is used as an integer): one batched beta sweep
    per particle number.  Returns a list of the per-N sweep dictionaries (keys of `sweep_over_betas`) with "N_part" added;
    the reference's fit of the blocking coefficients f, g to them (`rho_model`, :290-317) is closed-form SciPy on these
    numbers and stays with the caller.
    `one_launch=True` (exact dynamics only): all (N, beta, run) systems in one mixed launch, each counted with the blocking
    table of its own particle number, with the draws and hence the numbers of the loop over N; ValueError for the fixed-dt
    stepper, a large shape or a launch over the LDS limit.
    `allow_large=True` (with one_launch): as in sweep_over_sigmas.  Here a sweep straddles the limit when L <= 4096 and only some
    particle numbers exceed 2048: the launch is then the large kernel's for all of them, and the particle numbers below the limit
    equal gillespie.run_many_large_raw, not the host loop's batch kernel.
    `obs_per_launch`, `resume`, `return_checkpoint`: as in sweep_over_sigmas."""
    out = []
    for n_part in n_part_values:
        if float(n_part) != int(n_part):
            raise ValueError("particle numbers must be integral")
    iks = [dict(init_kwargs or {}, N=int(n_part)) for n_part in n_part_values]
    chain = _chain_keywords("sweep_over_densities", one_launch, _is_stepper(ps_kwargs, dynamics), obs_per_launch, resume, return_checkpoint)
    if one_launch:
        sweeps = _sweeps_in_one_launch("sweep_over_densities", [(dict(ps_kwargs or {}), ik) for ik in iks], beta_values, n_runs_per_beta,
                                       run_kwargs, rng_seeds, on_device, dynamics, allow_large, chain)
        if return_checkpoint:
            sweeps, ck = sweeps
    for ni, (n_part, ik) in enumerate(zip(n_part_values, iks)):
        r = sweeps[ni] if one_launch else sweep_over_betas(beta_values, n_runs_per_beta, ps_kwargs, ik, run_kwargs, rng_seeds,
                                                           on_device=on_device, dynamics=dynamics)
        r["N_part"] = int(n_part)
        out.append(r)
    return (out, ck) if return_checkpoint else out


def structure_ensemble_statistics(rows):
    """The reduction at the end of the reference's sweep_beta_structure_ensemble (PARTICLE_solver_BIOLOGY_local_structure.py
    :137-165) over the per-run dicts of structure observables; `raw` is the list itself."""
    n = len(rows)
    col = {k: np.array([r[k] for r in rows]) for k in ("var_mean", "low_k_power", "dominant_k", "m_local_var", "lowk_variance")}
    stack = np.stack([r["fft_mean"] for r in rows], axis=0)
    root = np.sqrt(n)
    return {"var_mean": col["var_mean"].mean(), "var_se": col["var_mean"].std(ddof=1) / root,
            "low_k_power_mean": col["low_k_power"].mean(), "low_k_power_se": col["low_k_power"].std(ddof=1) / root,
            "dominant_k_mode": int(np.round(col["dominant_k"].mean())),
            "m_local_var_mean": col["m_local_var"].mean(), "m_local_var_se": col["m_local_var"].std(ddof=1) / root,
            "fft_mean_mean": stack.mean(axis=0), "fft_mean_se": stack.std(axis=0, ddof=1) / root,
            "lowk_var_mean": col["lowk_variance"].mean(), "lowk_var_se": col["lowk_variance"].std(ddof=1) / root,
            "raw": rows}


def sweep_betas_for_structures(beta_values, n_runs_per_beta, ps_kwargs, init_kwargs, run_kwargs, start_fraction=0.5, k_max=None,
                               rng_seeds=None, dynamics=None):
    """The reference's structure sweep (PARTICLE_solver_BIOLOGY_local_structure.py:167-193, driver :671-753): {beta: result of
    sweep_beta_structure_ensemble}.  All (beta, run) pairs run in ONE launch; the per-run structure observables come from sums
    taken on the GPU at the observations of the window, so nothing of size M x L or M x n_cap exists and `raw` holds the per-run
    dicts without the reference's 'out'.  `rng_seeds[b][r]` seeds the initial condition of run r at beta b.  `run_kwargs` may
    hold T, obs_dt and the reference's record_fft / record_var (accepted and ignored: the sums are always taken).
    `dynamics` as in sweep_over_betas: "exact" (gillespie.run_batched_exact_structure) unless `ps_kwargs` asks for the stepper
    (`dt` or `mode="sync"`), then "sync" (particle_system.run_batched_structure)."""
    ps_kwargs, init_kwargs, run_kwargs = dict(ps_kwargs or {}), dict(init_kwargs or {}), dict(run_kwargs or {})
    if dynamics is None:
        dynamics = "sync" if (ps_kwargs.get("dt") is not None or ps_kwargs.get("mode") == "sync") else "exact"
    if dynamics not in ("sync", "exact"):
        raise ValueError("dynamics must be 'sync' or 'exact'")
    unknown = set(run_kwargs) - {"T", "obs_dt", "record_fft", "record_var"}
    if unknown:
        raise ValueError(f"run_kwargs may hold T, obs_dt, record_fft, record_var; got {sorted(unknown)}")
    slim = {k: v for k, v in run_kwargs.items() if k in ("T", "obs_dt")}
    systems, owner = [], []
    for bi, beta in enumerate(beta_values):
        for r in range(n_runs_per_beta):
            rng = None if rng_seeds is None else np.random.default_rng(int(rng_seeds[bi][r]))
            systems.append(ParticleSystem(beta=beta, rng=rng, **ps_kwargs, **init_kwargs))
            owner.append(bi)
    if dynamics == "exact":
        from .gillespie import run_batched_exact_structure
        rows = run_batched_exact_structure(systems, start_fraction=start_fraction, k_max=k_max, **slim)
    else:
        from .particle_system import run_batched_structure
        rows = run_batched_structure(systems, start_fraction=start_fraction, k_max=k_max, **slim)
    return {beta: structure_ensemble_statistics([row for row, o in zip(rows, owner) if o == bi]) for bi, beta in enumerate(beta_values)}


def sweep_sigmas_for_structures(sigma_values, beta_values, n_runs_per_beta, ps_kwargs, init_kwargs, run_kwargs, start_fraction=0.5,
                                k_max=None, rng_seeds=None, one_launch=True, return_series=False, obs_per_launch=None, resume=None,
                                return_checkpoint=False):
    """The pattern study over the interaction range: for every `local_kernel_sigma` of `sigma_values` the structure sweep of
    sweep_betas_for_structures -- the particle counterpart of pde.sweep_over_kernel_sigmas and of the reference's
    IMEX_PDE_solver_run_sweep_magn*.py.  Returns {sigma: {beta: structure_ensemble_statistics(...)}}.
    `one_launch=True`: all (sigma, beta, run) systems in ONE mixed launch of the exact event loop that takes the structure sums
    and reduces them over the window on the device (gillespie.run_batched_exact_structure_mixed): nothing of size observations x
    modes leaves the GPU.  The systems are built in the order of the host loop over sigma and every sigma is a group of the
    launch, so each sigma draws what its own launch draws.  `one_launch=False` is that host loop, one launch per sigma
    (gillespie.run_batched_exact_structure).
    `return_series=True`: returns (results, series) with series[sigma][beta] = {"times_obs", "m_abs_series", "var_series"}, the
    means over the runs of |m|(t) and var(total)(t): the arrays the PDE width sweep records per width.
    Exact dynamics only: ValueError for the fixed-dt stepper (`dt` or `mode="sync"` in ps_kwargs) and, with one_launch, for a
    large shape (L > 4096 or N > 2048), neither of which has a mixed launch -- raised here before any system is built where the
    numbers are known (L, and N of init="fixed"), and by the launch's own check once a Poisson initial state is drawn; `run_kwargs` may hold T, obs_dt, record_fft, record_var.
    `obs_per_launch`, `resume`, `return_checkpoint` (with one_launch): as in sweep_over_sigmas; the window sums travel in the
    MixedCheckpoint (gillespie.run_batched_exact_structure_mixed), and (results[, series], checkpoint) is returned."""
    from . import gillespie
    who = "sweep_sigmas_for_structures"
    ps_kwargs, init_kwargs, run_kwargs = dict(ps_kwargs or {}), dict(init_kwargs or {}), dict(run_kwargs or {})
    chain = _chain_keywords(who, one_launch, _is_stepper(ps_kwargs, None), obs_per_launch, resume, return_checkpoint)
    if ps_kwargs.get("dt") is not None or ps_kwargs.get("mode") == "sync":
        raise ValueError(f"{who} needs the exact dynamics; the fixed-dt stepper has no mixed launch")
    unknown = set(run_kwargs) - {"T", "obs_dt", "record_fft", "record_var"}
    if unknown:
        raise ValueError(f"run_kwargs may hold T, obs_dt, record_fft, record_var; got {sorted(unknown)}")
    slim = {k: v for k, v in run_kwargs.items() if k in ("T", "obs_dt")}
    L = int(ps_kwargs["L"])
    n_fixed = int(init_kwargs.get("N", 1000)) if init_kwargs.get("init", "fixed") == "fixed" else 0   # poisson: _mixed_launch raises the same ValueError once the states are drawn
    if one_launch and (L > gillespie.GIL_MAX_L or n_fixed > gillespie.GIL_MAX_N):
        raise ValueError(f"{who}: L = {L}, N = {n_fixed} is a large shape (beyond L = {gillespie.GIL_MAX_L}, "
                         f"N = {gillespie.GIL_MAX_N}); the large-system kernel takes no mixed batches")
    systems, group, owner = [], [], []
    for si, sigma in enumerate(sigma_values):
        for bi, beta in enumerate(beta_values):
            for r in range(n_runs_per_beta):
                rng = None if rng_seeds is None else np.random.default_rng(int(rng_seeds[bi][r]))
                systems.append(ParticleSystem(beta=beta, rng=rng, **dict(ps_kwargs, local_kernel_sigma=float(sigma)), **init_kwargs))
                group.append(si)
                owner.append(bi)
    per = len(beta_values) * n_runs_per_beta
    if one_launch:
        rows = gillespie.run_batched_exact_structure_mixed(systems, start_fraction=start_fraction, k_max=k_max, groups=group,
                                                           reduce="device", return_series=return_series, **slim, **chain)
        if return_checkpoint:
            rows, ck = rows
    else:
        rows = []
        for si in range(len(sigma_values)):
            mine = systems[si * per:(si + 1) * per]
            if return_series:                  # the series need the head rows: the mixed entry point, one sigma per launch
                rows += gillespie.run_batched_exact_structure_mixed(mine, start_fraction=start_fraction, k_max=k_max, reduce="rows",
                                                                    return_series=True, **slim)
            else:
                rows += gillespie.run_batched_exact_structure(mine, start_fraction=start_fraction, k_max=k_max, **slim)
    results, series = {}, {}
    for si, sigma in enumerate(sigma_values):
        mine, own = rows[si * per:(si + 1) * per], owner[si * per:(si + 1) * per]
        by_beta = [[row for row, o in zip(mine, own) if o == bi] for bi in range(len(beta_values))]
        if return_series:
            series[sigma] = {beta: {"times_obs": sel[0]["times_obs"].copy(),
                                    "m_abs_series": np.mean([np.abs(row["m_series"]) for row in sel], axis=0),
                                    "var_series": np.mean([row["var_series"] for row in sel], axis=0)}
                             for beta, sel in zip(beta_values, by_beta)}
            by_beta = [[{k: v for k, v in row.items() if k not in ("times_obs", "m_series", "var_series", "fft_amp_series")} for row in sel]
                       for sel in by_beta]
        results[sigma] = {beta: structure_ensemble_statistics(sel) for beta, sel in zip(beta_values, by_beta)}
    out = (results, series) if return_series else (results,)
    if return_checkpoint:
        out += (ck,)
    return out if len(out) > 1 else out[0]


def sweep_beta_structure_ensemble(beta, n_runs, ps_kwargs, init_kwargs, run_kwargs, start_fraction=0.5, k_max=None, rng_seeds=None,
                                  dynamics=None):
    """One beta, n_runs runs in one launch; the reference's result keys (:146-165).  `rng_seeds[r]` seeds run r."""
    return sweep_betas_for_structures([beta], n_runs, ps_kwargs, init_kwargs, run_kwargs, start_fraction, k_max,
                                      None if rng_seeds is None else [rng_seeds], dynamics)[beta]


def capture_study(ps_kwargs, init_kwargs, n_runs, run_kwargs, rng_seeds=None, on_device=True, c_bins=16, h_bins=40, h_dt=None,
                  start_fraction=0.0):
    """The anchor-capture study (PARTICLE_solver_BIOLOGY_EXCLUSION.py with its anchors switched on, analysed by
    PARTICLE_solver_CLASS.py:766-976) as an ensemble: `n_runs` runs of one parameter set in ONE launch of the exact event loop.
    Returns `<key>_mean`, `<key>_std` (ddof=1) and `<key>_se` across runs for `survival` [M], `cumulative_exits` [M][G],
    `cumulative_exits_total` [M], `exit_position_hist` [50] and `cluster_hist` [c_bins] (each run's cluster-size counts
    averaged over its observations from int(start_fraction * M) on), plus `times_obs`, `n_runs` and `raw` (the per-run dicts).
    `run_kwargs` holds T and obs_dt; `rng_seeds[r]` seeds the initial condition of run r.

    on_device=True (gillespie.run_batched_exact_capture): the counts come from the event loop itself, and the result also has
    `life_mean_*` [2] (mean bound lifetime per way of ending: unbinding, exit; runs where nothing ended that way are left out
    of the statistics), `life_hist_sum` [2][h_bins] (the runs' lifetime histograms added) and `life_edges`.
    on_device=False (gillespie.run_batched_exact + observables.capture_observables): the same keys from full outputs, WITHOUT
    the lifetime keys -- snapshots show only whether a particle slot is bound at the observation times, so a lifetime could be
    had to obs_dt at best and binds and unbinds between two observations would be missed; the event times exist on the
    device only."""
    from . import gillespie
    ps_kwargs, init_kwargs, run_kwargs = dict(ps_kwargs or {}), dict(init_kwargs or {}), dict(run_kwargs or {})
    unknown = set(run_kwargs) - {"T", "obs_dt"}
    if unknown:
        raise ValueError(f"run_kwargs may hold T and obs_dt; got {sorted(unknown)}")
    systems = [ParticleSystem(rng=None if rng_seeds is None else np.random.default_rng(int(rng_seeds[r])), **ps_kwargs, **init_kwargs)
               for r in range(n_runs)]
    if on_device:
        rows = gillespie.run_batched_exact_capture(systems, c_bins=c_bins, h_bins=h_bins, h_dt=h_dt, start_fraction=0.0, **run_kwargs)
    else:
        groups = observables.anchor_groups(systems[0]) if len(systems[0].anchor_idxs) else None
        outs = gillespie.run_batched_exact(systems, want_m_local=False, **run_kwargs)
        rows = [observables.capture_observables(out, groups, c_bins) for out in outs]
    M = len(rows[0]["survival"])
    start = int(start_fraction * M)
    per_run = {key: np.stack([np.asarray(r[key], dtype=float) for r in rows])
               for key in ("survival", "cumulative_exits", "cumulative_exits_total", "exit_position_hist")}
    per_run["cluster_hist"] = np.stack([np.asarray(r["cluster_hist"][start:], dtype=float).mean(axis=0) for r in rows])
    if on_device:
        per_run["life_mean"] = np.stack([r["life_mean"] for r in rows])
    res = {"times_obs": np.arange(0.0, run_kwargs.get("T", 10.0), run_kwargs.get("obs_dt", 0.01)), "n_runs": n_runs, "raw": rows}
    with np.errstate(invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)            # a way of ending that no run saw: nan, quietly
        for key, v in per_run.items():
            n = np.sum(~np.isnan(v), axis=0)
            res[key + "_mean"] = np.nanmean(v, axis=0)
            res[key + "_std"] = np.nanstd(v, axis=0, ddof=1)
            res[key + "_se"] = res[key + "_std"] / np.sqrt(np.maximum(n, 1))
    if on_device:
        res["life_hist_sum"] = np.sum([r["life_hist"] for r in rows], axis=0)
        res["life_edges"] = rows[0]["life_edges"]
    return res


def profile_sweep(beta_values, n_runs_per_beta, ps_kwargs, init_kwargs, run_kwargs, n_bins, rng_seeds=None, want_field=False,
                  on_device=True, obs_per_launch=None, resume=None, return_checkpoint=False):
    """Space-time profiles per beta under the exact dynamics: {beta: observables.DeviceProfiles.result()} -- per observation and
    bin the mean and standard error over the runs of the plus, minus, total and signed counts, the reference's densities
    `rho_plus`, `rho_minus`, `rho_total` (count / (N bin_sites dx)) and, with `want_field`, the mean field `field_mean`.  All
    (beta, run) pairs run in ONE launch, group = beta index.  `run_kwargs` holds T and obs_dt; `rng_seeds[b][r]` seeds the
    initial condition of run r at beta b.  Needs k_exit = 0 and the same N for the runs of a beta.

    on_device=True (gillespie.run_batched_exact_profiles): the event loop adds every run's bin counts to its beta's sums, and
    [betas][observations][7][n_bins] integers leave the GPU.  on_device=False (gillespie.run_batched_exact +
    observables.profile_observables): the same keys from the full state outputs, a bincount per run and observation on the host.
    `obs_per_launch=n`, `resume=ProfileCheckpoint`, `return_checkpoint=True` (on_device only): the one launch as a chain of launches
    of at most n observations, started from a checkpoint of the same sweep, and returning (results, checkpoint)
    (gillespie.run_batched_exact_profiles, include/gillespie_profile_resume.h); the numbers are the one launch's, bit for bit."""
    from . import gillespie
    ps_kwargs, init_kwargs, run_kwargs = dict(ps_kwargs or {}), dict(init_kwargs or {}), dict(run_kwargs or {})
    chain = _chain_keywords("profile_sweep", True, _is_stepper(ps_kwargs, None), obs_per_launch, resume, return_checkpoint)
    if chain and not on_device:
        raise ValueError("profile_sweep: the chain keywords need on_device=True; the host route has no checkpointed profile launch")
    unknown = set(run_kwargs) - {"T", "obs_dt"}
    if unknown:
        raise ValueError(f"run_kwargs may hold T and obs_dt; got {sorted(unknown)}")
    systems, owner = [], []
    for bi, beta in enumerate(beta_values):
        for r in range(n_runs_per_beta):
            rng = None if rng_seeds is None else np.random.default_rng(int(rng_seeds[bi][r]))
            systems.append(ParticleSystem(beta=beta, rng=rng, **ps_kwargs, **init_kwargs))
            owner.append(bi)
    if on_device:
        rows = gillespie.run_batched_exact_profiles(systems, n_bins=n_bins, groups=owner, want_field=want_field, **run_kwargs, **chain)
        if return_checkpoint:
            rows, ck = rows
    else:
        outs = gillespie.run_batched_exact(systems, want_m_local=want_field, **run_kwargs)
        rows = [observables.profile_observables([o for o, g in zip(outs, owner) if g == bi], n_bins, want_field, dx=systems[0].dx)
                for bi in range(len(beta_values))]
    res = {beta: rows[bi] for bi, beta in enumerate(beta_values)}
    return (res, ck) if return_checkpoint else res


def _profile_sweeps_in_one_launch(who, cases, beta_values, n_runs_per_beta, run_kwargs, n_bins, rng_seeds, want_field, allow_large, chain=None):
    """The profile sweeps of `cases` = [(ps_kwargs, init_kwargs)] as ONE mixed launch (gillespie.run_batched_exact_profiles_mixed):
    the systems are built in the order of the host loop over the cases, the ensemble group is (case, beta) and every case is a
    group of `mixed_keys`, so each case draws what its own `profile_sweep` launch draws.  Returns [case][beta index] results.
    `chain` (_chain_keywords): the launch in segments; with its return_checkpoint the result is (the list, the MixedProfileCheckpoint)."""
    from . import gillespie
    run_kwargs, chain = dict(run_kwargs or {}), dict(chain or {})
    unknown = set(run_kwargs) - {"T", "obs_dt"}
    if unknown:
        raise ValueError(f"run_kwargs may hold T and obs_dt; got {sorted(unknown)}")
    for ps_kwargs, _ in cases:
        if _is_stepper(ps_kwargs, None):
            raise ValueError(f"{who} needs the exact dynamics; the fixed-dt stepper has no mixed launch")
    systems, group, key_group, B = [], [], [], len(beta_values)
    for ci, (ps_kwargs, init_kwargs) in enumerate(cases):
        for bi, beta in enumerate(beta_values):
            for r in range(n_runs_per_beta):
                rng = None if rng_seeds is None else np.random.default_rng(int(rng_seeds[bi][r]))
                systems.append(ParticleSystem(beta=beta, rng=rng, **ps_kwargs, **init_kwargs))
                group.append(ci * B + bi)
                key_group.append(ci)
    rows = gillespie.run_batched_exact_profiles_mixed(systems, n_bins=n_bins, groups=group, key_groups=key_group, want_field=want_field,
                                                      allow_large=allow_large, **run_kwargs, **chain)
    ck = None
    if chain.get("return_checkpoint"):
        rows, ck = rows
    per_case = [rows[ci * B:(ci + 1) * B] for ci in range(len(cases))]
    return (per_case, ck) if chain.get("return_checkpoint") else per_case


def profile_sweep_over_sigmas(sigma_values, beta_values, n_runs_per_beta, ps_kwargs, init_kwargs, run_kwargs, n_bins, rng_seeds=None,
                              want_field=False, one_launch=True, allow_large=False, obs_per_launch=None, resume=None, return_checkpoint=False):
    """`profile_sweep` for every interaction range `local_kernel_sigma` of `sigma_values`: {sigma: {beta: profiles}}, the particle
    side of the comparison with pde.sweep_over_kernel_sigmas (the ensemble means of PARTICLE_solver_CLASS.py:205-213, :517-536
    per width).  `one_launch=True`: all (sigma, beta, run) systems in ONE mixed launch that adds every run's bin counts to the sums
    of its (sigma, beta) group (gillespie.run_batched_exact_profiles_mixed, include/gillespie_mixed_profile.h), with the draws and
    hence the numbers of the loop over sigma.  `one_launch=False` is that host loop, one `profile_sweep` launch per sigma.
    `allow_large=True` (with one_launch): a launch the library plans as a large shape (L > 4096, N > 2048, or profile slots that
    do not fit beside the loop) runs on the large-system kernel instead of a ValueError; its numbers equal the host loop's where
    every sigma's own launch is a large shape too, which is always so when L > 4096.  Exact dynamics only.
    `obs_per_launch=n`, `resume=MixedProfileCheckpoint`, `return_checkpoint=True` (with one_launch): the one launch as a chain of
    launches of at most n observations, started from a checkpoint of the same sweep, and returning (results, checkpoint)
    (gillespie.run_batched_exact_profiles_mixed); the numbers are the one launch's, bit for bit.  ValueError without one_launch."""
    kws = [dict(ps_kwargs or {}, local_kernel_sigma=float(sigma)) for sigma in sigma_values]
    chain = _chain_keywords("profile_sweep_over_sigmas", one_launch, _is_stepper(ps_kwargs, None), obs_per_launch, resume, return_checkpoint)
    if one_launch:
        rows = _profile_sweeps_in_one_launch("profile_sweep_over_sigmas", [(kw, dict(init_kwargs or {})) for kw in kws], beta_values,
                                             n_runs_per_beta, run_kwargs, n_bins, rng_seeds, want_field, allow_large, chain)
        if return_checkpoint:
            rows, ck = rows
        res = {sigma: dict(zip(beta_values, rows[si])) for si, sigma in enumerate(sigma_values)}
        return (res, ck) if return_checkpoint else res
    return {sigma: profile_sweep(beta_values, n_runs_per_beta, kw, init_kwargs, run_kwargs, n_bins, rng_seeds, want_field)
            for sigma, kw in zip(sigma_values, kws)}


def profile_sweep_over_densities(n_part_values, beta_values, n_runs_per_beta, ps_kwargs, init_kwargs, run_kwargs, n_bins, rng_seeds=None,
                                 want_field=False, one_launch=True, allow_large=False, obs_per_launch=None, resume=None,
                                 return_checkpoint=False):
    """`profile_sweep` for every particle number of `n_part_values` (the density N / L, the route to the hydrodynamic limit):
    {N: {beta: profiles}}.  `one_launch`, `allow_large`: as in profile_sweep_over_sigmas, the group being (N, beta) and every N a
    group of `mixed_keys`; here a sweep straddles the limit when L <= 4096 and only some particle numbers exceed 2048.
    `obs_per_launch`, `resume`, `return_checkpoint` (with one_launch): as in profile_sweep_over_sigmas."""
    for n_part in n_part_values:
        if float(n_part) != int(n_part):
            raise ValueError("particle numbers must be integral")
    iks = [dict(init_kwargs or {}, N=int(n_part)) for n_part in n_part_values]
    chain = _chain_keywords("profile_sweep_over_densities", one_launch, _is_stepper(ps_kwargs, None), obs_per_launch, resume, return_checkpoint)
    if one_launch:
        rows = _profile_sweeps_in_one_launch("profile_sweep_over_densities", [(dict(ps_kwargs or {}), ik) for ik in iks], beta_values,
                                             n_runs_per_beta, run_kwargs, n_bins, rng_seeds, want_field, allow_large, chain)
        if return_checkpoint:
            rows, ck = rows
        res = {int(n_part): dict(zip(beta_values, rows[ni])) for ni, n_part in enumerate(n_part_values)}
        return (res, ck) if return_checkpoint else res
    return {int(n_part): profile_sweep(beta_values, n_runs_per_beta, ps_kwargs, ik, run_kwargs, n_bins, rng_seeds, want_field)
            for n_part, ik in zip(n_part_values, iks)}
