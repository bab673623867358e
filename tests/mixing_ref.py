"""The numerical spec of bnmf_mixing restated in numpy float64, operation for operation: vectorised over the elements,
explicit loops over the samples (inside canon64_colsum) and the lags, the canonical W = 64 order for every sum.  Only + - * / and sqrt,
which numpy rounds correctly as the device does, so the device must give these bits.  Beside it a second, independent implementation
(FFT autocovariances, np.mean / np.var) against which the restatement itself is checked.  Shared by tests/test_mixing_host.py and
tests/test_gpu_mixing.py.  Test infrastructure only."""
import math

import numpy as np

from waic_ref import canon64_colsum

ROWS = ("mean", "var", "ess", "mcse", "rhat", "pairs", "exit", "mean_a", "var_a", "mean_b", "var_b")
LOW_ESS, HIGH_RHAT = 100.0, 1.01


def renormalised_series(Pw, Ew):
    """Pw [S][K][N], Ew [S][N][G] (samples oldest first) -> the series of the elements, xP [S][K N], xE [S][N G], in the column-major
    element order of the C ABI: cs_s[n] = k_map_colsum (the canonical sum over k), x = P / cs, x = E * cs (k_map_stats)."""
    Pw, Ew = np.asarray(Pw, dtype=np.float64), np.asarray(Ew, dtype=np.float64)
    S = Pw.shape[0]
    cs = np.stack([canon64_colsum(Pw[s]) for s in range(S)])                     # [S][N]
    with np.errstate(divide="ignore", invalid="ignore"):
        xP, xE = Pw / cs[:, None, :], Ew * cs[:, :, None]
    return xP.transpose(0, 2, 1).reshape(S, -1), xE.transpose(0, 2, 1).reshape(S, -1)


def mixing_reference(x):
    """x [S][L]: L series of S samples.  Returns the 11 rows by name (each length L; pairs and exit as float64, as the device writes
    them), `rows` ([11][L]) and n_clamped: how many Gammas the monotone clamp changed."""
    x = np.asarray(x, dtype=np.float64)
    S, L = x.shape
    assert S >= 4
    dS, h = float(S), S // 2
    dh, dh1 = float(h), float(h - 1)
    tau_min = 1.0 / math.log10(S)
    nan = np.full(L, np.nan)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mu = canon64_colsum(x) / dS
        xa, xb = x[:h], x[S - h:]
        mean_a, mean_b = canon64_colsum(xa) / dh, canon64_colsum(xb) / dh
        da, db = xa - mean_a[None, :], xb - mean_b[None, :]
        var_a, var_b = canon64_colsum(da * da) / dh1, canon64_colsum(db * db) / dh1
        d = x - mu[None, :]
        q0 = canon64_colsum(d * d)
        var, gamma0 = q0 / float(S - 1), q0 / dS
        ok = (gamma0 > 0.0) & ~(x == x[0][None, :]).all(axis=0)        # a constant series is degenerate whatever rounding left in gamma0
        W = (var_a + var_b) * 0.5
        mb = (mean_a + mean_b) * 0.5
        Bn = (mean_a - mb) * (mean_a - mb) + (mean_b - mb) * (mean_b - mb)
        vp = W * (dh1 / dh) + Bn
        rhat = np.where(ok & (W > 0.0), np.sqrt(vp / W), nan)

        def rho(t, idx):
            dd = d[:, idx]
            return (canon64_colsum(dd[:S - t] * dd[t:]) / dS) / gamma0[idx]
        every = np.arange(L)
        Gp = rho(0, every) + rho(1, every)
        total = Gp.copy()
        pairs, ex = np.where(ok, 1.0, 0.0), np.where(ok, 1.0, 0.0)
        active = ok.copy()
        n_clamped, m = 0, 1
        while 2 * m + 1 <= S - 2 and active.any():
            idx = np.where(active)[0]
            Gm = rho(2 * m, idx) + rho(2 * m + 1, idx)
            pos = Gm > 0.0
            ex[idx[~pos]] = 0.0
            active[idx[~pos]] = False
            go, g = idx[pos], Gm[pos]
            gm = np.where(g < Gp[go], g, Gp[go])
            n_clamped += int((gm != g).sum())
            total[go] = total[go] + gm
            Gp[go] = gm
            pairs[go] = pairs[go] + 1.0
            m += 1
        tau = 2.0 * total - 1.0
        tau = np.where(tau < tau_min, tau_min, tau)
        ess = np.where(ok, dS / tau, nan)
        mcse = np.where(ok, np.sqrt(var / ess), nan)
    out = dict(mean=mu, var=var, ess=ess, mcse=mcse, rhat=rhat, pairs=pairs, exit=ex, mean_a=mean_a, var_a=var_a, mean_b=mean_b, var_b=var_b)
    out["rows"] = np.stack([out[k] for k in ROWS])
    out["tau"] = np.where(ok, tau, nan)
    out["n_clamped"] = n_clamped
    return out


def mixing_summary(rowsP, rowsE, K, N, S, keep=None):
    """bnmf_mixing_info from the per-element rows: the scan in element order, P then E, over the factors keep flags (None = all)."""
    keep = np.ones(N, dtype=bool) if keep is None else np.asarray(keep) != 0
    lenP, lenE = rowsP.shape[1], rowsE.shape[1]
    selP, selE = keep[np.arange(lenP) // K], keep[np.arange(lenE) % N]
    info = dict(n_used=S, n_half=S // 2, n_const=0, n_ran_out=0, n_low_ess=0, n_high_rhat=0)
    for side, rows, sel in (("P", rowsP, selP), ("E", rowsE, selE)):
        ess, rhat, pairs, ex = rows[2], rows[4], rows[5], rows[6]
        with np.errstate(invalid="ignore"):
            info["n_const"] += int((sel & (pairs == 0.0)).sum())
            info["n_ran_out"] += int((sel & (ex == 1.0)).sum())
            info["n_low_ess"] += int((sel & (ess < LOW_ESS)).sum())
            info["n_high_rhat"] += int((sel & (rhat > HIGH_RHAT)).sum())
        for name, v, pick in (("min_ess", ess, np.argmin), ("max_rhat", rhat, np.argmax)):
            at = np.where(sel & ~np.isnan(v))[0]
            if at.size:
                i = int(at[pick(v[at])])                                          # argmin / argmax return the first of equals
                info[f"{name}_{side}"], info[f"{name}_{side}_at"] = float(v[i]), i
            else:
                info[f"{name}_{side}"], info[f"{name}_{side}_at"] = float("nan"), -1
    return info


def mixing_independent(x, eps=1e-9):
    """The same quantities by other means: autocovariances by FFT, np.mean / np.var, a scalar loop over the Gammas of each series.
    Returns tau (floored), ess, pairs, exit, rhat and `fragile`: the series for which some Gamma the rule looks at lies within eps of
    zero or of its (clamped) predecessor, so that rounding may decide pairs / exit."""
    x = np.asarray(x, dtype=np.float64)
    S, L = x.shape
    d = x - x.mean(axis=0)
    nfft = 1 << int(math.ceil(math.log2(2 * S)))
    f = np.fft.rfft(d, n=nfft, axis=0)
    acov = np.fft.irfft(f * np.conj(f), n=nfft, axis=0)[:S] / S
    tau_min = 1.0 / math.log10(S)
    tau, pairs, ex, fragile = np.full(L, np.nan), np.zeros(L, dtype=int), np.zeros(L, dtype=int), np.zeros(L, dtype=bool)
    for j in range(L):
        if not acov[0, j] > 0:
            continue
        r = acov[:, j] / acov[0, j]
        prev = r[0] + r[1]
        tot, n, out = prev, 1, 1
        m = 1
        while 2 * m + 1 <= S - 2:
            g = r[2 * m] + r[2 * m + 1]
            if abs(g) < eps or abs(g - prev) < eps:
                fragile[j] = True
            if not g > 0:
                out = 0
                break
            prev = min(g, prev)
            tot += prev
            n += 1
            m += 1
        tau[j], pairs[j], ex[j] = max(2 * tot - 1, tau_min), n, out
    h = S // 2
    a, b = x[:h], x[S - h:]
    W = (a.var(axis=0, ddof=1) + b.var(axis=0, ddof=1)) / 2
    B_over_n = np.var(np.stack([a.mean(axis=0), b.mean(axis=0)]), axis=0, ddof=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rhat = np.sqrt(((h - 1) / h * W + B_over_n) / W)
    return dict(tau=tau, ess=S / tau, pairs=pairs, exit=ex, rhat=rhat, fragile=fragile, mean=x.mean(axis=0), var=x.var(axis=0, ddof=1))


def ar1(phi, S, L, seed):
    """L seeded stationary AR(1) series of S samples, unit innovation variance: [S][L]"""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((S, L))
    x = np.empty((S, L))
    x[0] = e[0] / math.sqrt(1.0 - phi * phi)
    for s in range(1, S):
        x[s] = phi * x[s - 1] + e[s]
    return x
