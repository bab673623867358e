"""The numerical spec of bnmf_waic restated in numpy: the same sample order and the same streaming formulas, in any
floating type (float64, longdouble).  Shared by tests/test_waic_host.py (checked against closed forms) and tests/test_gpu_waic.py
(the device against it).  Test infrastructure only."""
import math

import numpy as np

LN_SQRT_2PI = 0.91893853320467274178      # the double the device subtracts (dnorm_log_sd)


def lgfact_table(max_m, dtype):
    """lgamma(m + 1), m = 0..max_m: libm in float64, the running sum of log(i) in a wider type"""
    if np.dtype(dtype) == np.float64:
        return np.array([math.lgamma(m + 1.0) for m in range(max_m + 1)])
    return np.concatenate([[dtype(0)], np.cumsum(np.log(np.arange(1, max_m + 1).astype(dtype)))]).astype(dtype)


def waic_reference(P, E, A, sigmasq, M, likelihood, dtype=np.float64):
    """P [S][K][N], E [S][N][G], A [S][N], sigmasq [S][G] (normal; else None), M [K][G]; samples oldest first.
    Returns the per-cell values (lppd, p, mean, elpd: K x G), their column sums and totals, se_elpd, n_high_var, and `mag`
    (K x G): the sum over the samples of the magnitudes of the terms of l_s, the scale of the device's rounding error."""
    T = np.dtype(dtype).type
    P, E, A = (np.asarray(x, dtype=np.float64).astype(T) for x in (P, E, A))
    S, K, N = P.shape
    G = E.shape[2]
    normal = likelihood == "normal"
    Mt = np.asarray(M, dtype=np.float64).astype(T)
    if normal:
        sig = np.asarray(sigmasq, dtype=np.float64).astype(T)
    else:
        Mi = np.asarray(M).astype(np.int64)
        lgf = lgfact_table(int(Mi.max()), T)[Mi]
    a = np.full((K, G), -np.inf, dtype=T)
    r, mu, m2, mag = (np.zeros((K, G), dtype=T) for _ in range(4))
    tiny = T(1e-6)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(S):
            c = np.zeros((K, G), dtype=T)
            for n in range(N):                                   # n ascending from +0.0, (P * A) * E
                c = c + (P[s, :, n] * A[s, n])[:, None] * E[s, n, :][None, :]
            if normal:
                sd = np.sqrt(sig[s])[None, :]
                lsd = np.log(sd)
                z = (Mt - c) / sd
                l = (-T(LN_SQRT_2PI) - lsd) - T(0.5) * (z * z)
                mag = mag + (np.abs(lsd) + T(LN_SQRT_2PI) + T(0.5) * (z * z))
            else:
                mh = np.where(c < tiny, tiny, c)
                lmh = np.log(mh)
                l = (Mt * lmh - mh) - lgf
                mag = mag + (np.abs(Mt * lmh) + mh + lgf)
            up = l > a
            ex = np.exp(np.where(up, a - l, l - a))
            r = np.where(up, r * ex + T(1), r + ex)
            a = np.where(up, l, a)
            d = l - mu
            mu = mu + d * (T(1) / T(s + 1))
            m2 = m2 + d * (l - mu)
    lppd = a + np.log(r / T(S))
    p = m2 / T(S - 1)
    elpd = lppd - p
    n = T(K * G)
    var = ((elpd - elpd.sum() / n) ** 2).sum() / (n - T(1)) if K * G > 1 else T(0)
    return dict(lppd_cell=lppd, p_cell=p, mean_cell=mu, elpd_cell=elpd, mag=mag,
                lppd_col=lppd.sum(axis=0), p_col=p.sum(axis=0), mean_col=mu.sum(axis=0),
                lppd=lppd.sum(), p_waic=p.sum(), mean_loglik=mu.sum(), elpd_waic=elpd.sum(), waic=T(-2) * elpd.sum(),
                se_elpd=np.sqrt(n * var), n_high_var=int((p > T(0.4)).sum()), n_used=S)


def canon64_colsum(x):
    """Column sums of x (K x G, float64) in the canonical W = 64 order: accumulator l adds rows l, l + 64, ... from +0.0, then the
    halving tree acc[i] += acc[i + h], h = 32 .. 1 (wave_tree64)."""
    x = np.asarray(x, dtype=np.float64)
    K, G = x.shape
    acc = np.zeros((64, G))
    for k in range(K):
        acc[k % 64] = acc[k % 64] + x[k]
    h = 32
    while h >= 1:
        acc[:h] = acc[:h] + acc[h:2 * h]
        h //= 2
    return acc[0].copy()


def seq_sum(x):
    """sequential float64 sum from +0.0 in index order (the host's totals over g)"""
    t = 0.0
    for v in np.asarray(x, dtype=np.float64).ravel():
        t = t + float(v)
    return t
