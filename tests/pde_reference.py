"""Extended-precision restatement of the hydrodynamic-limit scheme (the reference's IMEX_PDE_solver_class.py:64-233, :243-255),
fields and series only, for tests/pde_cases.py, tests/test_pde_cases_cpu.py and tests/test_gpu_pde_random.py.
A helper module, not a test: NumPy in `numpy.longdouble` (64-bit significand), no device code, no import of the package and
none of oracle/pde_numpy.py.  tests/test_pde_cases_cpu.py checks it against mpmath at 40 digits and against fixture G6.

What it is for: a yardstick better than the binary64 oracle.  The oracle multiplies rffts, whose round-off of about 1e-17 is
divided by den + 1e-12 on empty sites; here the Gaussian-kernel magnetisation is an untruncated direct circular sum, whose
errors are relative, and the diffusion solve multiplies by a dense inverse computed by Gauss-Jordan elimination in the same
arithmetic.  Parameters enter as the binary64 numbers every implementation is given (dx = xlim / L is formed in binary64, as
the reference and the device form it); all arithmetic after that is extended.

No tracers: their discrete decisions (the cell index of a tracer that starts exactly on a grid point, the flip comparison)
belong to the binary64 oracle.

`solve` takes a batch: rho_p0, rho_m0 [S, L] and betas [S] of one model, and returns arrays with a leading system axis."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "tests/pde_reference.py needs numpy.longdouble with at least a 64-bit significand"
_TWO_PI = LD(8) * np.arctan(LD(1))
KEYS = ("rho_p", "rho_m", "m_series", "var_series", "snapshots", "m_snapshots")


def inverse(a):
    """The inverse of a square longdouble matrix by Gauss-Jordan elimination with partial pivoting."""
    n = a.shape[0]
    w = np.concatenate([np.array(a, dtype=LD), np.eye(n, dtype=LD)], axis=1)
    for c in range(n):
        p = c + int(np.argmax(np.abs(w[c:, c])))
        if p != c:
            w[[c, p]] = w[[p, c]]
        w[c] = w[c] / w[c, c]
        f = w[:, c].copy()
        f[c] = 0
        w -= f[:, None] * w[c][None, :]
    return w[:, n:]


def diffusion_matrix(L, dx, dt, gamma, bc):
    """I - gamma dt Lap / dx^2 (ref :68-82)."""
    lap = np.zeros((L, L), dtype=LD)
    i = np.arange(L)
    lap[i, i] = -2
    lap[i[1:], i[:-1]] = 1
    lap[i[:-1], i[1:]] = 1
    if bc == "periodic":
        lap[0, L - 1] = lap[L - 1, 0] = 1
    elif bc == "neumann":
        lap[0, 1] = 2
        lap[L - 1, L - 2] = 2
    else:
        raise ValueError("bc must be 'periodic' or 'neumann'")
    return np.eye(L, dtype=LD) - LD(gamma) * LD(dt) * lap / LD(dx) ** 2


def kernel_matrix(L, dx, kernel_sigma):
    """K[j, i] = k((j - i) mod L), the Gaussian of the ring distance normalised over the ring (ref :84-93)."""
    i = np.arange(L)
    dist = np.minimum(i, L - i).astype(LD) * LD(dx)
    k = np.exp(-LD(0.5) * (dist / LD(kernel_sigma)) ** 2)
    k = k / k.sum()
    return k[(i[:, None] - i[None, :]) % L]


def _apply(A, x):
    """A applied to every row of x [S, L] (einsum: numpy's fastest longdouble product)."""
    return np.einsum("sl,jl->sj", x, A)


def magnetization(rho_p, rho_m, mode, K):
    """[S, L] (ref :154-166); mode 0: the local ratio, 1: K applied to numerator and denominator, 2: the global mean."""
    eps = LD(1e-12)
    if mode == 0:
        return (rho_p - rho_m) / (rho_p + rho_m + eps)
    if mode == 2:
        m = (rho_p - rho_m).sum(axis=1) / ((rho_p + rho_m).sum(axis=1) + eps)
        return np.repeat(m[:, None], rho_p.shape[1], axis=1)
    return _apply(K, rho_p - rho_m) / (_apply(K, rho_p + rho_m) + eps)


def cw_rate(beta, sigma, m):
    """ref :64-66; beta [S, 1]."""
    return np.clip(np.exp(-beta * sigma * m), LD(1e-8), LD(1e8))


def upwind(rho, direction, dx, bc):
    """ref :168-185 on [S, L]."""
    d = np.zeros_like(rho)
    if direction > 0:
        d[:, 1:] = (rho[:, 1:] - rho[:, :-1]) / dx
        if bc != "neumann":
            d[:, 0] = (rho[:, 0] - rho[:, -1]) / dx
    else:
        d[:, :-1] = (rho[:, 1:] - rho[:, :-1]) / dx
        if bc != "neumann":
            d[:, -1] = (rho[:, 0] - rho[:, -1]) / dx
    return d


def kernel_mode(gaussian_kernel, kernel_sigma):
    return 0 if not gaussian_kernel else 2 if kernel_sigma > 100000 else 1


def solve(*, L, xlim, dt, nsteps, gamma, lam, betas, bc, active_model, gaussian_kernel, kernel_sigma, snapshot_interval,
          rho_p0, rho_m0, n_fft_modes=0, keep_m=False):
    """The fields and series of ref :236-255 + :187-233 for every system of the batch, as longdouble arrays:
    rho_p, rho_m [S, L]; m_series, var_series [S, nsteps + 1]; snapshots, m_snapshots [S, n_snap, L]; fft [S, nsteps + 1,
    n_fft_modes] complex as (fft_re, fft_im); with keep_m the magnetisation field of every step, m_fields [S, nsteps + 1, L]."""
    dx = float(xlim) / L                                             # binary64, as everywhere else
    mode = kernel_mode(gaussian_kernel, kernel_sigma)
    Ainv = inverse(diffusion_matrix(L, dx, dt, gamma, bc))
    K = kernel_matrix(L, dx, kernel_sigma) if mode == 1 else None
    rho_p, rho_m = np.array(rho_p0, dtype=LD).reshape(-1, L), np.array(rho_m0, dtype=LD).reshape(-1, L)
    S = rho_p.shape[0]
    beta = np.asarray(betas, dtype=np.float64).astype(LD).reshape(S, 1)
    dxl, dtl, laml = LD(dx), LD(dt), LD(lam)
    jk = (np.arange(n_fft_modes)[:, None] * np.arange(L)[None, :]) % L
    ang = _TWO_PI * jk.astype(LD) / LD(L)
    cos_t, sin_t = np.cos(ang).T, np.sin(ang).T                      # [L, modes]
    m_series, var_series = np.zeros((S, nsteps + 1), LD), np.zeros((S, nsteps + 1), LD)
    fft_re, fft_im = np.zeros((S, nsteps + 1, n_fft_modes), LD), np.zeros((S, nsteps + 1, n_fft_modes), LD)
    snaps, m_snaps, m_fields = [], [], []
    for n in range(nsteps + 1):
        total = rho_p + rho_m
        m = magnetization(rho_p, rho_m, mode, K)
        m_series[:, n] = m.mean(axis=1)
        var_series[:, n] = ((total - total.mean(axis=1, keepdims=True)) ** 2).mean(axis=1)
        if n_fft_modes:
            fft_re[:, n] = (total @ cos_t) / LD(L)                  # rfft: sum x_j exp(-2 pi i j k / L)
            fft_im[:, n] = -(total @ sin_t) / LD(L)
        if n % snapshot_interval == 0:
            snaps.append(total.copy())
            m_snaps.append(rho_p - rho_m)
        if keep_m:
            m_fields.append(m)
        if n == nsteps:
            break
        dp, dm = _apply(Ainv, rho_p), _apply(Ainv, rho_m)                   # implicit diffusion, ref :189-190
        R_p = cw_rate(beta, -1, m) * dm - cw_rate(beta, +1, m) * dp
        if active_model == "bidirectional":                          # ref :192-204
            rho_p = np.clip(dp + dtl * (-laml * upwind(dp, +1, dxl, bc) + R_p), 0, None)
            rho_m = np.clip(dm + dtl * (+laml * upwind(dm, -1, dxl, bc) - R_p), 0, None)
        else:                                                        # ref :205-227
            star_p = np.clip(dp + dtl * R_p, 0, None)
            rho_m = np.clip(dm + dtl * (-R_p), 0, None)
            rho_p = np.clip(star_p + dtl * (-laml * upwind(star_p, +1, dxl, bc)), 0, None)
        M0 = (dp + dm).sum(axis=1, keepdims=True)                    # ref :229-233
        M1 = (rho_p + rho_m).sum(axis=1, keepdims=True)
        rho_p, rho_m = rho_p * (M0 / M1), rho_m * (M0 / M1)
    out = dict(rho_p=rho_p, rho_m=rho_m, m_series=m_series, var_series=var_series, snapshots=np.stack(snaps, axis=1),
               m_snapshots=np.stack(m_snaps, axis=1), fft_re=fft_re, fft_im=fft_im,
               times=np.arange(len(snaps)) * snapshot_interval * dt)
    if keep_m:
        out["m_fields"] = np.stack(m_fields, axis=1)
    return out


def scale(ref, key):
    """The scale a deviation from ref[key] is measured in: the largest magnitude, for m_series at least 1e-3 (m is a ratio in
    [-1, 1]: the floor makes a relative 1e-11 an absolute 1e-14)."""
    s = float(np.max(np.abs(ref)))
    return max(s, 1e-3) if key == "m_series" else max(s, 1e-300)


def deviation(got, ref, key):
    """max |got - ref| over the scale of ref, the difference taken in extended precision."""
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - ref))) / scale(ref, key)
