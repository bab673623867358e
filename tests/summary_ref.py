"""DESIGN.md 29 restated in numpy float64, operation for operation: the cohort summary of signatures over a recorded range
(bnmf_summary).  Only + - * /, comparisons and counts, every floating-point sum in the order the spec fixes and every order statistic
exact, so the device is held to this bit for bit.  Test infrastructure only."""
import numpy as np

from contrast_ref import canon64, per_tumour
from map_ref import type7
from regress_ref import BLOCK, Refused, canonB

SCALARS = ("prevalence", "total", "fraction", "mean_present")
FAMILIES = ("load_all", "load_present", "share_all")
ROWS = ("mean", "var", "lower", "upper", "n_valid")
MAX_Q, MAX_M = 8, 1000000


def names(probs):
    return list(SCALARS) + [f"{fam}_{p:g}" for fam in FAMILIES for p in probs]


def quantile(y, p):
    """the type-7 order statistic of the ascending y [k], k >= 1:  h = (k - 1) p, j = floor(h), g = h - j, a = y[j], b = y[min(j + 1, k - 1)],
    a == b ? a : (1 - g) a + g b"""
    k = y.size
    j, g = type7(k, float(p))
    a, b = float(y[j]), float(y[min(j + 1, k - 1)])
    if a == b:
        return a
    with np.errstate(invalid="ignore", over="ignore"):
        return float(np.float64(1.0 - g) * np.float64(a) + np.float64(g) * np.float64(b))


def loads_and_shares(P, E, A, members):
    """x, r [S][N][m]: the loads and the shares of the members with -0.0 turned into +0.0"""
    with np.errstate(invalid="ignore", over="ignore"):
        x, _, _, t = per_tumour(P, E, A, 0.0)
    x = x + 0.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = np.where(t > 0, 1.0 / np.where(t > 0, t, 1.0), 0.0)
        r = x * u[:, None, :] + 0.0
    return x[:, :, members], r[:, :, members]


def sample_stats(x, r, min_load, probs):
    """x, r [N][m] of one sample -> values [NSTAT][N] by factor, bad [N]"""
    N, m = x.shape
    L = len(probs)
    out = np.full((4 + 3 * L, N), np.nan)
    b = x >= min_load
    c = b.sum(axis=1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        total = canonB(x.T)
        pres = canonB(np.where(b, x, 0.0).T)
        den = 0.0
        for n in range(N):
            den = den + total[n]
        out[0] = c.astype(np.float64) / float(m)
        out[1] = total
        out[2] = total / den if den > 0 else np.nan
        out[3] = np.where(c > 0, pres / np.where(c > 0, c, 1).astype(np.float64), np.nan)
    bad = ~(np.isfinite(x).all(axis=1) & np.isfinite(r).all(axis=1))
    for n in range(N):
        if bad[n]:
            continue
        xs, rs = np.sort(x[n]), np.sort(r[n])
        for l, p in enumerate(probs):
            out[4 + l, n] = quantile(xs, p)
            if c[n] > 0:
                out[4 + L + l, n] = quantile(xs[m - c[n]:], p)
            out[4 + 2 * L + l, n] = quantile(rs, p)
    return out, bad


def reduce(series, ci):
    """series [NSTAT][S][N] -> stat [NSTAT][5][N] over the samples whose value is not NaN"""
    Q, S, N = series.shape
    stat = np.full((Q, 5, N), np.nan)
    for q in range(Q):
        for n in range(N):
            v = series[q, :, n]
            v = v[~np.isnan(v)]
            k = v.size
            stat[q, 4, n] = float(k)
            if not k:
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                mean = float(canon64(v)) / float(k)
                stat[q, 0, n] = mean
                if k >= 2:
                    stat[q, 1, n] = float(canon64((v - mean) * (v - mean))) / float(k - 1)
            if ci > 0:
                xs = np.sort(v)
                stat[q, 2, n], stat[q, 3, n] = quantile(xs, (1.0 - ci) / 2.0), quantile(xs, (1.0 + ci) / 2.0)
    return stat


def summary_reference(P, E, A, probs=(0.05, 0.25, 0.5, 0.75, 0.95), include=None, perm=None, min_load=1.0, credible_interval=0.95):
    """P [S][K][N], E [S][N][G], A [S][N]: the USED samples, oldest first; include [G] of 0 / 1 or None; perm [S][N] (a row per USED sample; a
    row of -1 leaves the sample out) or None.  Returns what Engine.summary returns with series=True and x, r (the members' loads and shares,
    [S][N][m]); refuses (Refused) what the call refuses after its arguments' shapes."""
    P, E, A = np.asarray(P, dtype=np.float64), np.asarray(E, dtype=np.float64), np.asarray(A, dtype=np.float64)
    S, N, G = E.shape
    inc = np.ones(G, dtype=np.int64) if include is None else np.asarray(include, dtype=np.int64)
    if ((inc != 0) & (inc != 1)).any():
        raise Refused(-1, "include is neither 0 nor 1")
    members = np.where(inc == 1)[0]
    m = members.size
    pm = np.tile(np.arange(N), (S, 1)) if perm is None else np.asarray(perm, dtype=np.int64)
    left = (pm == -1).all(axis=1)
    for s in range(S):
        if not left[s] and sorted(pm[s].tolist()) != list(range(N)):
            raise Refused(-1, f"perm row {s} is not a permutation")
    ml, ci = float(min_load), float(credible_interval)
    pr = [float(p) for p in probs]
    L = len(pr)
    if not ml >= 0.0 or np.isinf(ml):
        raise Refused(-1, "min_load is not a finite number >= 0")
    if L < 1 or L > MAX_Q:
        raise Refused(-1, f"L = {L}")
    for l, p in enumerate(pr):
        if not (0.0 <= p <= 1.0) or (l > 0 and not p > pr[l - 1]):
            raise Refused(-1, f"probs[{l}]")
    if not ci < 1.0:
        raise Refused(-1, "credible_interval must be below 1")
    if S < 2:
        raise Refused(-2, f"{S} used samples")
    if int((~left).sum()) < 2:
        raise Refused(-2, f"{int((~left).sum())} aligned samples")
    if m < 1 or m > MAX_M:
        raise Refused(-2, f"{m} included tumours")
    x, r = loads_and_shares(P, E, A, members)
    series = np.full((4 + 3 * L, S, N), np.nan)
    nbad = 0
    for s in range(S):
        if left[s]:
            continue
        v, bad = sample_stats(x[s], r[s], ml, pr)
        series[:, s, pm[s]] = v                                                     # the value of factor n at the place of its label
        nbad += int(bad.sum())
    return dict(stat=reduce(series, ci), series=series, names=names(pr), probs=np.asarray(pr), n_used=S, n_aligned=int((~left).sum()),
                n_included=int(m), n_left_out=int(G - m), n_levels=L, n_blocks=(m + BLOCK - 1) // BLOCK, n_nonfinite=nbad, min_load=ml,
                credible_interval=ci, x=x, r=r, members=members)
