"""DESIGN.md 20 restated in numpy float64, operation for operation: the regression of exposures on tumour covariates over a recorded
range (bnmf_regress).  Only + - * /, sqrt, comparisons and integer counts, every sum in the order the spec fixes, so the device is held
to this bit for bit.  Test infrastructure only."""
import math

import numpy as np

from contrast_ref import canon64, moments, per_tumour
from map_ref import interpolate, type7

STATS = ("load", "share", "sqrt_load")
BLOCK = 1024
MAX_Q = 16


class Refused(ValueError):
    """the restatement's refusals: .code is the ABI's (-1 BNMF_EINVAL, -2 BNMF_ESIZE)"""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def canonB(v):
    """step 3: the blocked canonical sum along axis 0: blocks of 1,024, each the canonical W = 64 sum, added in order from +0.0"""
    v = np.asarray(v, dtype=np.float64)
    tot = np.zeros(v.shape[1:])
    for i0 in range(0, v.shape[0], BLOCK):
        tot = tot + canon64(v[i0:i0 + BLOCK])
    return tot


def gram(D):
    """step 4.  D [m][Q] in member order"""
    Q = D.shape[1]
    Gm = np.zeros((Q, Q))
    for j in range(Q):
        for k in range(j + 1):
            Gm[j, k] = Gm[k, j] = float(canonB(D[:, j] * D[:, k]))
    return Gm


def cholesky(Gm):
    """step 5: L, min_pivot_ratio, min_pivot_at; a pivot that is not > 0 or not finite is refused"""
    Q = Gm.shape[0]
    L = np.zeros((Q, Q))
    ratio, at = 0.0, -1
    for j in range(Q):
        d = float(Gm[j, j])
        for t in range(j):
            d = d - float(L[j, t]) * float(L[j, t])
        if not d > 0.0 or math.isinf(d):
            raise Refused(-1, f"design is not of full column rank (column {j})")
        rj = d / float(Gm[j, j])
        if at < 0 or rj < ratio:
            ratio, at = rj, j
        L[j, j] = math.sqrt(d)
        for i in range(j + 1, Q):
            w = float(Gm[i, j])
            for t in range(j):
                w = w - float(L[i, t]) * float(L[j, t])
            L[i, j] = w / float(L[j, j])
    return L, ratio, at


def solve(L, w):
    """step 7.  w [Q][...] -> beta [Q][...]"""
    Q = L.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        z = [None] * Q
        for j in range(Q):
            v = w[j]
            for t in range(j):
                v = v - L[j, t] * z[t]
            z[j] = v / L[j, j]
        beta = [None] * Q
        for j in range(Q - 1, -1, -1):
            v = z[j]
            for t in range(j + 1, Q):
                v = v - L[t, j] * beta[t]
            beta[j] = v / L[j, j]
    return np.stack(beta)


def responses(P, E, A, members):
    """steps 1 - 2 -> Y [m][3][S][N] over the members"""
    x, r, _, t = per_tumour(P, E, A, 0.0)
    with np.errstate(invalid="ignore"):
        Y = np.stack([x, r, np.sqrt(x)])                                           # [3][S][N][G]
    return np.ascontiguousarray(np.moveaxis(Y[:, :, :, members], 3, 0)), t


def fit_samples(Y, D, L):
    """steps 6 - 8 for responses Y [m][...] -> beta [Q][...], r2, sigma2 [...]"""
    m, Q = D.shape
    ex = (slice(None),) + (None,) * (Y.ndim - 1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        w = np.stack([canonB(Y * D[:, j][ex]) for j in range(Q)])
        sy = canonB(Y)
        beta = solve(L, w)
        yh = np.zeros(Y.shape)
        for j in range(Q):
            yh = yh + D[:, j][ex] * beta[j][None]
        rss = canonB((Y - yh) * (Y - yh))
        ybar = sy / float(m)
        tss = canonB((Y - ybar[None]) * (Y - ybar[None]))
        r2 = np.where(tss > 0, 1.0 - rss / np.where(tss > 0, tss, 1.0), np.nan)
        sigma2 = rss / float(m - Q)
    return beta, r2, sigma2


def reduce(beta, r2, sigma2, ci):
    """steps 9 - 10.  beta [Q][3][S][N], r2 / sigma2 [3][S][N] -> coef [3][6][N][Q], fit [3][5][N], n_credible [3][Q]"""
    Q, _, S, N = beta.shape
    coef, fit = np.zeros((3, 6, N, Q)), np.zeros((3, 5, N))
    n_credible = np.zeros((3, Q), dtype=np.int64)
    for q in range(3):
        b = np.moveaxis(beta[:, q], 0, 2)                                           # [S][N][Q]
        mean, var, lo, hi = moments(b, ci)
        coef[q] = np.stack([mean, var, lo, hi, (b > 0).sum(axis=0) / float(S), (b < 0).sum(axis=0) / float(S)])
        n_credible[q] = ((lo > 0) | (hi < 0)).sum(axis=0)
        for n in range(N):
            v = r2[q, :, n]
            v = v[~np.isnan(v)]
            fit[q, :3, n] = np.nan
            if v.size:
                fit[q, 0, n] = float(canon64(v)) / float(v.size)
            if v.size and ci > 0:
                xs = np.sort(v)
                fit[q, 1, n] = interpolate(xs, *type7(v.size, (1.0 - ci) / 2.0))
                fit[q, 2, n] = interpolate(xs, *type7(v.size, (1.0 + ci) / 2.0))
            fit[q, 3, n] = float(v.size)
            fit[q, 4, n] = float(canon64(sigma2[q, :, n])) / float(S)
    return coef, fit, n_credible


def regress_reference(P, E, A, design, include=None, credible_interval=0.95):
    """P [S][K][N], E [S][N][G], A [S][N]: the USED samples, oldest first; design [G][Q]; include [G] of 0 / 1 or None.  Returns what
    Engine.regress returns with series=True and Y, L, Gm of the steps in between; refuses (Refused) what the call refuses after its
    arguments' shapes."""
    design = np.asarray(design, dtype=np.float64)
    G, Q = design.shape
    S = np.asarray(P).shape[0]
    inc = np.ones(G, dtype=np.int64) if include is None else np.asarray(include, dtype=np.int64)
    if ((inc != 0) & (inc != 1)).any():
        raise Refused(-1, "include is neither 0 nor 1")
    members = np.where(inc == 1)[0]
    m = members.size
    if Q < 1 or Q > MAX_Q:
        raise Refused(-1, f"Q = {Q}")
    D = np.ascontiguousarray(design[members])
    if not np.isfinite(D).all():
        i, j = np.argwhere(~np.isfinite(D))[0]
        raise Refused(-1, f"design[{members[i]}, {j}] is not finite")
    ci = float(credible_interval)
    if not ci < 1.0:
        raise Refused(-1, "credible_interval must be below 1")
    if S < 2:
        raise Refused(-2, f"{S} used samples")
    if m <= Q:
        raise Refused(-2, f"{m} included tumours for Q = {Q}")
    Gm = gram(D)
    L, ratio, at = cholesky(Gm)
    Y, t = responses(P, E, A, members)
    beta, r2, sigma2 = fit_samples(Y, D, L)
    coef, fit, n_credible = reduce(beta, r2, sigma2, ci)
    return dict(coef=coef, fit=fit, coef_series=np.ascontiguousarray(np.moveaxis(beta, 0, 3)), r2_series=r2, sigma2_series=sigma2, n_used=S, Q=Q,
                n_included=int(m), n_left_out=int(G - m), n_blocks=(m + BLOCK - 1) // BLOCK, min_pivot_at=at, min_pivot_ratio=ratio, n_credible=n_credible,
                credible_interval=ci, Y=Y, L=L, Gm=Gm, t=t, members=members)
