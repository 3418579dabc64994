"""Ensemble observables of the reference's sweep drivers, restated (host side, NumPy).

These are the quantities the reference's statistics are judged on; they consume the `out`
dictionary of `ParticleSystem.run`.  Reference map (file = PARTICLE_solver_BIOLOGY_EXCLUSION_sweep_beta.py):
    velocity_and_window      <- compute_v_eff_and_window      :123-162
    front_density            <- compute_rho_eff               :165-194
    blocking_probability     <- compute_blocking_probability  :197-229   (vectorised; the reference loops in Python)
    mean_magnetisation       <- compute_mean_magnetizatoin    :316-319
    active_diffusivity       <- compute_D_eff_active          :500-525
    ensemble_statistics      <- the reduction at the end of sweep_beta_ensemble :97-117
    structure_observables    <- extract_structure_observables_from_out of PARTICLE_solver_BIOLOGY_local_structure.py:55-103
Pinned by fixtures tests/golden/g7_observables.npz and g10_structure.npz (generated from the reference's own functions).
"""
from __future__ import annotations

import numpy as np


def velocity_and_window(out, L, boundary_xmin=0.99, max_boundary_fraction=0.06, min_window_fraction=0.10):
    """Centre-of-mass velocity and the averaging window [start, end).

    The window logic reproduces the reference as written: frames with too much mass at the right wall are
    collected as INDICES, and the reference then bit-inverts a slice of that index array, which is non-zero
    for every element -- so if any flagged index sits at position >= start of that array the window closes at
    `start` and is re-opened to the minimum length; otherwise it runs to the end."""
    times = out["times_obs"]
    total = out["total_list"]
    M = total.shape[0]
    grid = np.linspace(0.0, 1.0, total.shape[1])
    dx = grid[1] - grid[0]
    at_wall = total[:, grid >= boundary_xmin].sum(axis=1) * dx
    mass = total.sum(axis=1) * dx
    frac_boundary = at_wall / (mass + 1e-12)
    flagged = np.flatnonzero(frac_boundary >= max_boundary_fraction)
    start = int(0.65 * M)
    if flagged.size == 0:
        end = M
    else:
        end = M if flagged[start:].size == 0 else start
        shortest = max(3, int(min_window_fraction * M))
        if end - start < shortest:
            end = min(M, start + shortest)
    grid = np.linspace(0.0, 1.0, L)
    com = (total * grid).sum(axis=1) / (total.sum(axis=1) + 1e-12)
    v_eff = np.gradient(com, times)
    return float(np.mean(v_eff[start:end])), v_eff, times, start, end, frac_boundary


def front_density(out, start, end, window_fraction=0.05):
    total = np.asarray(out["total_list"])
    grid = np.linspace(0.0, 1.0, total.shape[1])
    dx = grid[1] - grid[0]
    vals = []
    for t in range(start, end):
        occupied = np.flatnonzero(total[t] > 0)
        if occupied.size == 0:
            continue
        x_front = grid[occupied[-1]]
        window = (grid >= x_front - window_fraction) & (grid <= x_front)
        if window.any():
            vals.append(total[t][window].sum() * dx / window_fraction)
    return float(np.mean(vals))


def blocking_probability(out, start, end):
    """Share of the + density whose right neighbour site carries total density >= 1 (reference units)."""
    total = np.asarray(out["total_list"])[start:end]
    plus = np.asarray(out["rho_p_list"])[start:end]
    movers = np.where(plus[:, :-1] > 0, plus[:, :-1], 0.0)
    attempts = movers.sum()
    if attempts == 0:
        return 0.0
    return float((movers * (total[:, 1:] >= 1.0)).sum() / attempts)


def mean_magnetisation(out, start, end):
    return float(np.mean(np.asarray(out["m_global"], dtype=float)[start:end]))


def active_diffusivity(out, dx, start, end):
    times, frames = out["times_obs"], out["pos_list"]
    ref, t_ref = frames[start] * dx, times[start]
    spread, lag = [], []
    for k in range(start + 1, end):
        cur = frames[k] * dx
        n = min(len(ref), len(cur))
        if n < 2:
            continue
        disp = cur[:n] - ref[:n]
        spread.append(np.sum((disp - np.mean(disp)) ** 2) / (n - 1))
        lag.append(times[k] - t_ref)
    return np.polyfit(lag, spread, 1)[0]


def run_observables(out, L, dx):
    """All five per-run observables with the reference's default window parameters."""
    v, _, _, start, end, _ = velocity_and_window(out, L)
    return dict(v=v, D=active_diffusivity(out, dx, start, end), m=mean_magnetisation(out, start, end),
                rho=front_density(out, start, end), block=blocking_probability(out, start, end), window=(start, end))


def ensemble_statistics(rows):
    """Mean / sample standard deviation / standard error over runs, keyed like the reference's savez arrays
    (..._sweep_beta.py:952-968: means, stds, ses, D_means, D_ses, m_means, m_stds, m_ses, rho_means, rho_ses,
    block_means, block_ses)."""
    n = len(rows)
    col = {k: np.array([r[k] for r in rows], dtype=float) for k in ("v", "D", "m", "rho", "block")}
    sd = {k: (float(a.std(ddof=1)) if n > 1 else 0.0) for k, a in col.items()}
    root = np.sqrt(max(1, n))
    return dict(mean=float(col["v"].mean()), std=sd["v"], se=sd["v"] / root, v_array=col["v"],
                D_mean=float(col["D"].mean()), D_se=sd["D"] / root,
                m_mean=float(col["m"].mean()), m_std=sd["m"], m_se=sd["m"] / root,
                rho_mean=float(col["rho"].mean()), rho_se=sd["rho"] / root,
                block_mean=float(col["block"].mean()), block_se=sd["block"] / root)


# ---------------------------------------------------------------------------------------------------------------
# The same five observables from the device-side integer sums (aps_observe_scalars): no M x L arrays leave the GPU.
class DeviceObservables:
    """Per-run accumulator.  `plan(k)` tells the stepping loop what to ask the device for at observation k,
    `add(k, sums, front)` stores the answer, `result()` evaluates the reference's formulas
    (PARTICLE_solver_BIOLOGY_EXCLUSION_sweep_beta.py:123-229, :316-319, :500-525) on the stored sums.
    Exact for the integer parts; the float parts differ from the array formulas only by summation order."""

    def __init__(self, times, L, dx, K, boundary_xmin=0.99, max_boundary_fraction=0.06, min_window_fraction=0.10,
                 front_window_fraction=0.05):
        self.times, self.L, self.dx, self.K = np.asarray(times, dtype=float), int(L), float(dx), int(K)
        self.M = len(self.times)
        self.grid = np.linspace(0.0, 1.0, self.L)
        self.gdx = self.grid[1] - self.grid[0]
        self.x_wall = int(np.searchsorted(self.grid, boundary_xmin, side="left"))
        self.max_boundary_fraction, self.min_window_fraction = max_boundary_fraction, min_window_fraction
        self.wf = front_window_fraction
        self.start = int(0.65 * self.M)
        self.rows = [None] * self.M
        self.front = [None] * self.M

    def block_table(self, n_live):
        """Is a right neighbour with (plus, minus) particles 'blocking'?  total density >= 1 in the reference's units
        rho = count / (N_now * dx), evaluated with the reference's float operations."""
        denom = float(max(1, n_live)) * self.dx
        cp, cm = np.meshgrid(np.arange(self.K + 1), np.arange(self.K + 1), indexing="ij")
        return ((cp / denom).astype(float) + (cm / denom).astype(float) >= 1.0).astype(np.uint8)

    def front_range(self, max_pos):
        """Site range [lo, hi] of the reference's front window below the right-most occupied site."""
        x_front = self.grid[max_pos]
        lo = int(np.searchsorted(self.grid, x_front - self.wf, side="left"))
        return lo, int(max_pos)

    def add(self, k, sums, n_front=None):
        self.rows[k] = dict(sums)
        self.front[k] = n_front

    def result(self):
        M, dx, gdx = self.M, self.dx, self.gdx
        n = np.array([r["n"] for r in self.rows], dtype=float)
        dens = 1.0 / (np.maximum(n, 1.0) * dx)                     # one particle in the reference's density units
        mass = n * dens * gdx
        frac_boundary = np.array([r["n_wall"] for r in self.rows]) * dens * gdx / (mass + 1e-12)
        flagged = np.flatnonzero(frac_boundary >= self.max_boundary_fraction)
        start = self.start
        if flagged.size == 0:
            end = M
        else:
            end = M if flagged[start:].size == 0 else start
            shortest = max(3, int(self.min_window_fraction * M))
            if end - start < shortest:
                end = min(M, start + shortest)
        com = (np.array([r["sum_pos"] for r in self.rows]) / (self.L - 1.0)) * dens / (n * dens + 1e-12)
        v_ts = np.gradient(com, self.times)
        m_glob = np.array([r["sum_sigma"] / r["n"] if r["n"] else np.nan for r in self.rows])
        fronts = [self.front[k] * dens[k] * gdx / self.wf for k in range(start, end) if self.front[k] is not None]
        att = sum(self.rows[k]["attempts"] * dens[k] for k in range(start, end))
        blk = sum(self.rows[k]["blocked"] * dens[k] for k in range(start, end))
        spread, lag = [], []
        for k in range(start + 1, end):
            r = self.rows[k]
            nd = r["n_d"]
            if nd < 2:
                continue
            spread.append(dx * dx * (r["sum_d2"] - r["sum_d"] ** 2 / nd) / (nd - 1))
            lag.append(self.times[k] - self.times[start])
        D = np.polyfit(lag, spread, 1)[0] if len(lag) >= 2 else float("nan")
        return dict(v=float(np.mean(v_ts[start:end])), D=float(D), m=float(np.mean(m_glob[start:end])),
                    rho=float(np.mean(fronts)) if fronts else float("nan"), block=float(blk / att) if att else 0.0,
                    window=(start, end), v_ts=v_ts, frac_boundary=frac_boundary, m_global=m_glob)


# ------------------------------------------------------------------------------------------------ structure observables
def structure_observables(out, start_fraction=0.5, k_max=None):
    """Pattern / clustering observables of a run made with record_fft=True, record_var=True
    (PARTICLE_solver_BIOLOGY_local_structure.py:55-103): time mean and spread of var(total) and of the Fourier
    amplitudes |fft(total)| over the steady-state window [start_fraction * M, M), the dominant non-zero mode, the summed
    low-k amplitudes (k = 1..24), the variance of the local magnetisation over window x lattice and the mean low-k power."""
    M = len(out["times_obs"])
    start = int(start_fraction * M)
    var_ts = np.asarray(out["var_list"], dtype=float)[start:]
    amp = np.asarray(out["fft_amp_list"], dtype=float)
    if k_max is not None:
        amp = amp[:, :k_max]
    ss = amp[start:]
    fft_mean, fft_std = ss.mean(axis=0), ss.std(axis=0, ddof=1)
    cut = min(25, amp.shape[1])
    m_ss = np.asarray(out["m_local_list"], dtype=float)[start:]
    return {"var_mean": var_ts.mean(), "var_std": var_ts.std(ddof=1), "fft_mean": fft_mean, "fft_std": fft_std,
            "dominant_k": int(np.argmax(fft_mean[1:]) + 1), "low_k_power": float(np.sum(fft_mean[1:cut])),
            "m_local_var": float(np.var(m_ss)), "lowk_variance": float(np.mean(np.sum(ss[:, 1:cut] ** 2, axis=1)))}


extract_structure_observables_from_out = structure_observables      # the reference's name


class DeviceStructure:
    """The same eight observables accumulated from what the GPU returns per observation (aps_observe_structure): the live
    particle number n, sum over sites of count^2, sum and sum of squares of the local magnetisation over the L sites, and the
    first k_max Fourier sums of the site histogram.  Nothing of size M x L ever leaves the device.

    total = count / (n dx) (ref :205-213), so var(total) = (sum c^2 / L - (n / L)^2) / (n dx)^2 and
    |fft(total)|_k = |sum_x c_x exp(-2 pi i k x / L)| / (n dx)."""

    def __init__(self, n_obs, L, dx, start_fraction=0.5, k_max=None):
        self.M, self.L, self.dx = int(n_obs), int(L), float(dx)
        self.start = int(start_fraction * self.M)
        self.k_max = self.L if k_max is None else min(int(k_max), self.L)
        self.var, self.amp, self.m1, self.m2 = [], [], 0.0, 0.0
        self.nm = 0

    def add(self, k, n_live, sum_c2, sum_m, sum_m2, re_im):
        if k < self.start:
            return
        L, nd = self.L, float(n_live) * self.dx
        self.var.append((sum_c2 / L - (n_live / L) ** 2) / (nd * nd) if n_live else np.nan)
        z = np.asarray(re_im, dtype=float).reshape(-1, 2)
        self.amp.append(np.hypot(z[:, 0], z[:, 1]) / nd if n_live else np.full(len(z), np.nan))
        self.m1 += sum_m
        self.m2 += sum_m2
        self.nm += L

    def result(self):
        var, amp = np.array(self.var), np.array(self.amp)
        fft_mean, fft_std = amp.mean(axis=0), amp.std(axis=0, ddof=1)
        cut = min(25, amp.shape[1])
        mean_m = self.m1 / self.nm
        return {"var_mean": var.mean(), "var_std": var.std(ddof=1), "fft_mean": fft_mean, "fft_std": fft_std,
                "dominant_k": int(np.argmax(fft_mean[1:]) + 1), "low_k_power": float(np.sum(fft_mean[1:cut])),
                "m_local_var": float(self.m2 / self.nm - mean_m * mean_m),
                "lowk_variance": float(np.mean(np.sum(amp[:, 1:cut] ** 2, axis=1)))}


class DeviceStructureWindow:
    """The eight observables of DeviceStructure from what a mixed structure launch reduces on the device
    (include/gillespie_mixed_structure.h), without the rows: `head` [M][4] (n, sum c^2, sum m, sum m^2 of every observation),
    `window` [k_max][3] (per mode a0, sum d, sum d^2 over the window, d = a - a0, a = |sum_x c_x exp(-2 pi i k x / L)| / n),
    `n_window` observations accumulated and `n_empty` window observations without a live particle.

    |fft(total)|_k = a_k / dx, so fft_mean = (a0 + sum d / M_w) / dx and, shifted sums being free of cancellation,
    fft_std^2 = (sum d^2 - (sum d)^2 / M_w) / (M_w - 1) / dx^2; sum_t a^2 = sum d^2 + 2 a0 sum d + M_w a0^2 gives lowk_variance.
    var_* and m_local_var come from the head rows exactly as DeviceStructure takes them from the rows.  With an empty
    observation in the window DeviceStructure's amplitudes and var are NaN; so are they here."""

    def __init__(self, head, window, n_window, n_empty, L, dx, start_fraction=0.5):
        self.head, self.win = np.asarray(head, dtype=float), np.asarray(window, dtype=float)
        self.M, self.L, self.dx = len(self.head), int(L), float(dx)
        self.start = int(start_fraction * self.M)
        self.n_window, self.n_empty = int(n_window), int(n_empty)

    def var_series(self):
        """var(total) of every observation (NaN where no particle is alive)."""
        n, c2 = self.head[:, 0], self.head[:, 1]
        nd = n * self.dx
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(n > 0, (c2 / self.L - (n / self.L) ** 2) / (nd * nd), np.nan)

    def result(self):
        h = self.head[self.start:]
        var = self.var_series()[self.start:]
        Mw, dx = self.n_window, self.dx
        a0, s1, s2 = self.win[:, 0], self.win[:, 1], self.win[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            fft_mean = (a0 + s1 / Mw) / dx
            fft_std = np.sqrt(np.maximum(s2 - s1 * s1 / Mw, 0.0) / (Mw - 1)) / dx
            sum_a2 = (s2 + 2.0 * a0 * s1 + Mw * a0 * a0) / (dx * dx)
        cut = min(25, len(a0))
        lowk = float(np.sum(sum_a2[1:cut]) / Mw) if Mw else np.nan
        if self.n_empty or Mw != len(h):           # an empty observation: DeviceStructure's NaNs
            fft_mean, fft_std, lowk = np.full(len(a0), np.nan), np.full(len(a0), np.nan), np.nan
        nm = self.L * len(h)
        m1, m2 = sum(h[:, 2].tolist()), sum(h[:, 3].tolist())   # in observation order, as DeviceStructure.add
        mean_m = m1 / nm
        return {"var_mean": var.mean(), "var_std": var.std(ddof=1), "fft_mean": fft_mean, "fft_std": fft_std,
                "dominant_k": int(np.argmax(fft_mean[1:]) + 1), "low_k_power": float(np.sum(fft_mean[1:cut])),
                "m_local_var": float(m2 / nm - mean_m * mean_m), "lowk_variance": lowk}


# ------------------------------------------------------------------------------------------------ anchor-capture study
EXIT_POSITION_BINS = 50


def anchor_groups(ps):
    """Site -> anchor id (PARTICLE_solver_CLASS.py:923-928): for every site of `ps.anchor_idx_array` the nearest centre of
    `ps.anchor_idxs` (argmin: the first centre on ties), -1 elsewhere.  int32 [L], the `group_of_site` of gilc_run."""
    groups = np.full(int(ps.L), -1, np.int32)
    centres = np.asarray(ps.anchor_idxs, dtype=int)
    sites = np.asarray(ps.anchor_idx_array, dtype=int)
    if centres.size and sites.size:
        groups[sites] = np.argmin(np.abs(centres[None, :] - sites[:, None]), axis=1)
    return groups


def cluster_counts(occupied, c_bins):
    """Maximal runs of True in `occupied`, scanned from site 0 to L - 1 without joining across the seam
    (get_cluster_sizes, ref :769-781): (occupied sites, clusters, largest, sum of size^2, histogram over sizes
    1 .. c_bins - 1 and >= c_bins)."""
    o = np.concatenate([[0], np.asarray(occupied, dtype=np.int8), [0]])
    d = np.diff(o)
    sizes = np.flatnonzero(d == -1) - np.flatnonzero(d == 1)
    hist = np.bincount(np.minimum(sizes, c_bins) - 1, minlength=c_bins).astype(np.int64)
    return int(sizes.sum()), int(sizes.size), int(sizes.max()) if sizes.size else 0, int((sizes.astype(np.int64) ** 2).sum()), hist


def _survival_keys(times_obs, n_t):
    """ref :848-855"""
    n_t = np.asarray(n_t, dtype=float)
    n0 = n_t[0]
    flux = np.clip(-np.gradient(n_t, times_obs), 0, None) if len(n_t) > 1 else np.zeros_like(n_t)
    fpt_pdf = flux / n0
    total_exited = n0 - n_t[-1]
    return {"survival": n_t / n0, "fpt_pdf": fpt_pdf, "fpt_pdf_cond": flux / total_exited if total_exited > 0 else fpt_pdf * 0.0}


def capture_observables(out, group_of_site, c_bins=16):
    """The capture study's curves (PARTICLE_solver_CLASS.py:766-976) from the full outputs of one run (`ParticleSystem.run`,
    gillespie.run_batched_exact): `survival`, `fpt_pdf`, `fpt_pdf_cond` (ref :848-855); `cumulative_exits` [M][G] and
    `cumulative_exits_total` [M] (ref :934-954: exit times binned by the observation times, searchsorted side="right", then
    cumulated; G = largest group id + 1); `exit_position_hist`, 50 bins of exit position / L (ref :893; over [0, 1] here,
    so that runs can be added, where the reference lets the bins follow the data); and per observation the cluster
    quantities `occupied_sites`, `n_clusters`, `largest_cluster`, `sum_size2` [M] and `cluster_hist` [M][c_bins] (ref :769-783,
    which looks at the last observation only).  Clusters do not join across the seam of a ring, as in the reference."""
    times = np.asarray(out["times_obs"], dtype=float)
    M = len(times)
    total = np.asarray(out["total_list"])
    L = total.shape[1]
    groups = np.full(L, -1, int) if group_of_site is None else np.asarray(group_of_site, dtype=int)
    G = int(groups.max()) + 1 if groups.size else 0
    res = _survival_keys(times, out["particle_count_list"])
    exit_t, exit_x = np.asarray(out["exit_times"], dtype=float), np.asarray(out["exit_positions"], dtype=int)
    dt = times[1] - times[0] if M > 1 else 1.0
    edges = np.concatenate([times, [times[-1] + dt]])
    counts = np.zeros((M, max(G, 0)), np.int64)
    for t, x in zip(exit_t, exit_x):
        g = groups[x] if 0 <= x < L else -1
        b = int(np.searchsorted(edges, t, side="right")) - 1
        if g >= 0 and 0 <= b < M:
            counts[b, g] += 1
    res["cumulative_exits"] = np.cumsum(counts, axis=0)
    res["cumulative_exits_total"] = res["cumulative_exits"].sum(axis=1)
    res["exit_position_hist"] = np.histogram(exit_x / L, bins=EXIT_POSITION_BINS, range=(0.0, 1.0))[0].astype(np.int64)
    rows = [cluster_counts(total[k] > 1e-12, c_bins) for k in range(M)]
    for j, key in enumerate(("occupied_sites", "n_clusters", "largest_cluster", "sum_size2")):
        res[key] = np.array([r[j] for r in rows], np.int64)
    res["cluster_hist"] = np.stack([r[4] for r in rows])
    return res


class DeviceCapture:
    """The keys of `capture_observables` from what gilc_run returns for one system (include/gillespie_capture.h) -- the live
    counts of the scalar sums, the rows of capture counts, the exit log -- plus the lifetimes of bound states, which only the
    event loop resolves: `life_hist` [2][h_bins] (ended by unbinding, by exit), `life_edges`, `life_count`, `life_mean`,
    `life_var` [2] (nan where nothing ended that way) and `binds`, `unbinds`, `n_bound` [M].

    Row k counts the exits logged with a time < times_obs[k] (the event that crossed an observation was drawn before it), so
    the reference's bin b of the cumulative exits is row b + 1 and its last bin the last row, the run's total."""

    def __init__(self, times_obs, L, n_groups, c_bins, h_dt):
        self.times, self.L, self.G, self.c_bins, self.h_dt = np.asarray(times_obs, dtype=float), int(L), int(n_groups), int(c_bins), float(h_dt)

    def result(self, n_live, rows, exits, life_hist, life_sums):
        rows = np.asarray(rows, dtype=np.int64)
        G = self.G
        res = _survival_keys(self.times, n_live)
        shifted = np.concatenate([rows[1:], rows[-1:]], axis=0)
        res["cumulative_exits"] = shifted[:, 9:9 + G].copy()
        res["cumulative_exits_total"] = res["cumulative_exits"].sum(axis=1)
        exit_x = np.asarray(exits, dtype=float).reshape(-1, 3)[:, 1]
        res["exit_position_hist"] = np.histogram(exit_x / self.L, bins=EXIT_POSITION_BINS, range=(0.0, 1.0))[0].astype(np.int64)
        for j, key in enumerate(("occupied_sites", "n_clusters", "largest_cluster", "sum_size2")):
            res[key] = rows[:, 5 + j].copy()
        res["cluster_hist"] = rows[:, 9 + G:9 + G + self.c_bins].copy()
        res.update(n_bound=rows[:, 1].copy(), binds=rows[:, 2].copy(), unbinds=rows[:, 3].copy())
        hist, sums = np.asarray(life_hist, dtype=np.int64), np.asarray(life_sums, dtype=float)
        count = hist.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(count > 0, sums[:, 0] / count, np.nan)
            var = np.where(count > 0, sums[:, 1] / count - mean * mean, np.nan)
        res.update(life_hist=hist.copy(), life_edges=self.h_dt * np.arange(hist.shape[1] + 1), life_count=count, life_mean=mean, life_var=var)
        return res


# ------------------------------------------------------------------------------------------------ ensemble profiles
def profile_bins(L, n_bins):
    """The bin rule of gilp_run and aps_observe_bins: (width, bins that hold sites, sites per bin [n_bins])."""
    L, n_bins = int(L), int(n_bins)
    width = -(-L // n_bins)
    used = -(-L // width)
    sites = np.zeros(n_bins, np.int64)
    sites[:used] = width
    sites[used - 1] = L - (used - 1) * width
    return width, used, sites


class DeviceProfiles:
    """The ensemble profiles of one group from what gilp_run returns for it (include/gillespie_profile.h): `ensemble_sums`
    [M][7][n_bins] (sums over the members of n+, n-, n_bound, n+^2, n-^2, n+ n- per bin, and of the field in 2^-32 fixed point)
    and `members` [M].  `result()` gives, per observation and bin,
      `plus_mean`, `minus_mean`, `total_mean`, `signed_mean` (n+ - n-) and their `_se` (standard error over the members, ddof = 1;
          the variances of total and signed count take the cross column: var+ + var- +/- 2 cov), `bound_mean` (the device takes
          no second moment of the bound count, so it has no `_se`),
      `field_mean` with the field: the mean over members and over the bin's sites of m(x),
      `rho_plus`, `rho_minus`, `rho_total` and their `_se`: the densities in the reference's normalisation count / (N bin_sites
          dx) (PARTICLE_solver_CLASS.py:205-213), the ensemble means of rho_plus_list, rho_minus_list coarse-grained to the bins,
      `times_obs`, `members`, `bin_sites` [n_bins], `bin_width`, `n_bins_used`.
    Observations no member recorded (and those before `first_obs`) are nan; a standard error needs two members.

    The reference divides each run by its current particle number, which a sum over runs cannot reproduce: the densities need
    all members to start with the same N and k_exit = 0, anything else is a ValueError."""

    def __init__(self, times_obs, L, dx, n_bins, ensemble_sums, members, n_particles, k_exit=0.0, want_field=False, first_obs=0):
        self.times, self.L, self.dx, self.n_bins = np.asarray(times_obs, dtype=float), int(L), float(dx), int(n_bins)
        self.sums, self.members = np.asarray(ensemble_sums, dtype=np.int64), np.asarray(members, dtype=np.int64)
        if self.sums.shape != (len(self.times), 7, self.n_bins) or self.members.shape != (len(self.times),):
            raise ValueError("ensemble_sums must be [observations][7][n_bins] and members [observations]")
        ns = {int(n) for n in np.atleast_1d(n_particles)}
        if len(ns) != 1:
            raise ValueError(f"the members of a group must start with the same particle number, got {sorted(ns)}")
        if k_exit:
            raise ValueError("the profile densities need k_exit = 0: the reference divides every run by its current particle number")
        self.N, self.want_field, self.first_obs = ns.pop(), bool(want_field), int(first_obs)
        self.width, self.used, self.bin_sites = profile_bins(self.L, self.n_bins)

    @staticmethod
    def _moments(n, s1, s2):
        """mean and standard error (ddof = 1) from n, sum x, sum x^2; the variance's numerator in exact integers"""
        n = n[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(n > 0, s1 / np.maximum(n, 1), np.nan)
            var = np.where(n > 1, (n * s2 - s1 * s1) / np.maximum(n * (n - 1), 1).astype(float), np.nan)
            return mean, np.sqrt(var / np.maximum(n, 1))

    def result(self):
        n, s = self.members, self.sums
        p1, m1, b1, p2, m2, pm = (s[:, j, :] for j in range(6))
        res = {"times_obs": self.times.copy(), "members": n.copy(), "bin_sites": self.bin_sites.copy(), "bin_width": self.width,
               "n_bins_used": self.used}
        res["plus_mean"], res["plus_se"] = self._moments(n, p1, p2)
        res["minus_mean"], res["minus_se"] = self._moments(n, m1, m2)
        res["total_mean"], res["total_se"] = self._moments(n, p1 + m1, p2 + m2 + 2 * pm)
        res["signed_mean"], res["signed_se"] = self._moments(n, p1 - m1, p2 + m2 - 2 * pm)
        res["bound_mean"] = self._moments(n, b1, b1)[0]
        sites = np.where(self.bin_sites > 0, self.bin_sites, 1).astype(float)
        if self.want_field:
            with np.errstate(invalid="ignore", divide="ignore"):
                res["field_mean"] = np.where(n[:, None] > 0, s[:, 6, :] / 4294967296.0 / np.maximum(n, 1)[:, None] / sites, np.nan)
        norm = self.N * sites * self.dx
        for src, dst in (("plus", "rho_plus"), ("minus", "rho_minus"), ("total", "rho_total")):
            res[dst], res[dst + "_se"] = res[src + "_mean"] / norm, res[src + "_se"] / norm
        return res


def profile_sums(outs, n_bins, want_field=False, first_obs=0):
    """What gilp_run would return for ONE group made of the runs `outs` (full outputs of gillespie.run_batched_exact): the
    integer `ensemble_sums` [M][7][n_bins], `members` [M] and the per-run counts [runs][M][3][n_bins], by bincount on the host.
    The field column sums llrint(m_local_list * 2^32) over the bin's sites."""
    M, L = np.asarray(outs[0]["total_list"]).shape
    width, used, _ = profile_bins(L, n_bins)
    sums, members, rows = np.zeros((M, 7, n_bins), np.int64), np.zeros(M, np.int64), np.zeros((len(outs), M, 3, n_bins), np.int64)
    for r, out in enumerate(outs):
        for k in range(first_obs, M):
            if out["pos_list"][k] is None:
                continue                                           # the run ended before this observation
            pos = np.asarray(out["pos_list"][k], dtype=np.int64)
            # count / (N dx) per site, and sum(total) = 1 / dx: the counts come back as integers
            scale = pos.size / max(float(np.sum(out["total_list"][k])), 1e-300)
            cp = np.rint(np.asarray(out["rho_p_list"][k]) * scale).astype(np.int64)
            cm = np.rint(np.asarray(out["rho_m_list"][k]) * scale).astype(np.int64)
            cb = np.bincount(pos[np.asarray(out["bound_list"][k], dtype=bool)], minlength=L)
            b = np.arange(L) // width
            np_, nm, nd = (np.bincount(b, weights=c, minlength=n_bins).astype(np.int64) for c in (cp, cm, cb))
            rows[r, k] = np_, nm, nd
            sums[k, :6] += np.stack([np_, nm, nd, np_ * np_, nm * nm, np_ * nm])
            if want_field:
                q = np.rint(np.asarray(out["m_local_list"][k], dtype=float) * 4294967296.0).astype(np.int64)
                np.add.at(sums[k, 6], b, q)
            members[k] += 1
    return sums, members, rows


def profile_observables(outs, n_bins, want_field=False, first_obs=0, dx=None):
    """The keys of `DeviceProfiles.result` for one group from the full outputs of its runs (gillespie.run_batched_exact): a
    bincount per run and observation on the host.  `dx=None`: read off the outputs (the site densities of a run add up to 1 / dx)."""
    first = outs[0]
    M, L = np.asarray(first["total_list"]).shape
    if dx is None:
        dx = 1.0 / float(np.sum(first["total_list"][0]))
    sums, members, _ = profile_sums(outs, n_bins, want_field, first_obs)
    return DeviceProfiles(first["times_obs"], L, dx, n_bins, sums, members, [o["particle_count_list"][0] for o in outs],
                          0.0, want_field, first_obs).result()
