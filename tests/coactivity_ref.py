"""DESIGN.md 21 restated in numpy float64, operation for operation: the co-activity of signatures over a recorded range
(bnmf_coactivity).  Only + - * /, sqrt, comparisons and whole numbers, every floating-point sum in the order the spec fixes, so the device
is held to this bit for bit.  Test infrastructure only."""
import numpy as np

from contrast_ref import canon64, per_tumour
from map_ref import interpolate, type7
from regress_ref import BLOCK, Refused, canonB

STATS = ("pearson", "spearman", "copresence", "cosine")
ROWS = ("mean", "var", "lower", "upper", "p_greater", "p_less", "n_valid")
MAX_M = 1000000


def pair_list(N):
    """the pairs a < b, a ascending, then b ascending"""
    return [(a, b) for a in range(N) for b in range(a + 1, N)]


def rank_c(x):
    """x [m] -> c = 2 less + equal - m (int64), less = #(x_j < x_i), equal = #(x_j == x_i) with i itself; the values compared as doubles"""
    x = np.asarray(x, dtype=np.float64)
    xs = np.sort(x)
    less, le = np.searchsorted(xs, x, side="left"), np.searchsorted(xs, x, side="right")
    return (2 * less + (le - less) - x.size).astype(np.int64)


def midranks(x):
    """less + (equal + 1) / 2 = (c + m + 1) / 2"""
    return (rank_c(x) + np.asarray(x).size + 1) / 2.0


def pearson(xm):
    """step 4.  xm [m][N] -> v0 [N][N], S [N][N], mu [N]"""
    m = xm.shape[0]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mu = canonB(xm) / float(m)
        d = xm - mu[None, :]
        S = canonB(d[:, :, None] * d[:, None, :])
        den = np.diag(S)[:, None] * np.diag(S)[None, :]
        v0 = np.where(den > 0, S / np.sqrt(np.where(den > 0, den, 1.0)), np.nan)
    return v0, S, mu


def spearman(xm):
    """step 5.  xm [m][N] -> v1 [N][N], T [N][N] int64, c [m][N]; a factor with a load that is not finite is NaN in all its pairs"""
    m, N = xm.shape
    c = np.stack([rank_c(xm[:, n]) for n in range(N)], axis=1)
    T = c.T @ c                                                                     # int64: |c| < m <= 10^6
    bad = ~np.isfinite(xm).all(axis=0)
    v1 = np.full((N, N), np.nan)
    for a in range(N):
        for b in range(N):
            if T[a, a] > 0 and T[b, b] > 0 and not bad[a] and not bad[b]:
                v1[a, b] = float(T[a, b]) / np.sqrt(float(T[a, a]) * float(T[b, b]))
    return v1, T, c


def copresence(xm, min_load):
    """step 6.  xm [m][N] -> v2 [N][N] and the counts n11 [N][N]"""
    m, N = xm.shape
    b = xm >= min_load
    n11 = b.T.astype(np.int64) @ b.astype(np.int64)
    v2 = np.full((N, N), np.nan)
    for a in range(N):
        for c in range(N):
            k11, k1x, kx1 = int(n11[a, c]), int(n11[a, a]), int(n11[c, c])
            k10, k01, k00, k0x, kx0 = k1x - k11, kx1 - k11, m - k1x - kx1 + k11, m - k1x, m - kx1
            if k1x > 0 and k0x > 0 and kx1 > 0 and kx0 > 0:
                v2[a, c] = (float(k11) * float(k00) - float(k10) * float(k01)) / np.sqrt((float(k1x) * float(k0x)) * (float(kx1) * float(kx0)))
    return v2, n11


def cosine(P, A):
    """step 7.  P [K][N], A [N] -> v3 [N][N]: dot, nn_a, nn_b over k ascending from +0.0"""
    K, N = P.shape
    dot, nn = np.zeros((N, N)), np.zeros(N)
    for k in range(K):
        dot = dot + P[k][:, None] * P[k][None, :]
        nn = nn + P[k] * P[k]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        v3 = dot / np.sqrt(nn[:, None] * nn[None, :])
    inc = A != 0
    return np.where(inc[:, None] & inc[None, :], v3, np.nan)


def reduce(series, ci):
    """steps 9 - 10.  series [4][S][NP] -> pair [4][7][NP], n_credible [3], max_cosine_at, max_cosine"""
    _, S, NP = series.shape
    pair = np.full((4, 7, NP), np.nan)
    for q in range(4):
        for p in range(NP):
            v = series[q, :, p]
            v = v[~np.isnan(v)]
            n = v.size
            pair[q, 6, p] = float(n)
            if not n:
                continue
            mean = float(canon64(v)) / float(n)
            pair[q, 0, p] = mean
            if n >= 2:
                with np.errstate(invalid="ignore", over="ignore"):
                    pair[q, 1, p] = float(canon64((v - mean) * (v - mean))) / float(n - 1)
            if ci > 0:
                xs = np.sort(v)
                pair[q, 2, p] = interpolate(xs, *type7(n, (1.0 - ci) / 2.0))
                pair[q, 3, p] = interpolate(xs, *type7(n, (1.0 + ci) / 2.0))
            pair[q, 4, p], pair[q, 5, p] = float((v > 0).sum()) / float(n), float((v < 0).sum()) / float(n)
    n_credible = [int(((pair[q, 2] > 0) | (pair[q, 3] < 0)).sum()) for q in range(3)]
    at, mx = -1, float("nan")
    for p in range(NP):
        c = pair[3, 0, p]
        if not np.isnan(c) and (at < 0 or c > mx):
            at, mx = p, float(c)
    return pair, n_credible, at, mx


def coactivity_reference(P, E, A, include=None, min_load=1.0, credible_interval=0.95):
    """P [S][K][N], E [S][N][G], A [S][N]: the USED samples, oldest first; include [G] of 0 / 1 or None.  Returns what Engine.coactivity
    returns with series=True and x (the loads of the members, [S][N][m]), c (the rank numbers, [S][m][N]) of the steps in between;
    refuses (Refused) what the call refuses after its arguments' shapes."""
    P, E, A = np.asarray(P, dtype=np.float64), np.asarray(E, dtype=np.float64), np.asarray(A, dtype=np.float64)
    S, N, G = E.shape
    inc = np.ones(G, dtype=np.int64) if include is None else np.asarray(include, dtype=np.int64)
    if ((inc != 0) & (inc != 1)).any():
        raise Refused(-1, "include is neither 0 nor 1")
    members = np.where(inc == 1)[0]
    m = members.size
    ml, ci = float(min_load), float(credible_interval)
    if not ml >= 0.0 or np.isinf(ml):
        raise Refused(-1, "min_load is not a finite number >= 0")
    if not ci < 1.0:
        raise Refused(-1, "credible_interval must be below 1")
    if N < 2:
        raise Refused(-2, f"N = {N}")
    if S < 2:
        raise Refused(-2, f"{S} used samples")
    if m < 3 or m > MAX_M:
        raise Refused(-2, f"{m} included tumours")
    x = per_tumour(P, E, A, ml)[0][:, :, members]                                   # [S][N][m]
    pairs = pair_list(N)
    ia, ib = [a for a, _ in pairs], [b for _, b in pairs]
    series = np.zeros((4, S, len(pairs)))
    cs = []
    for s in range(S):
        xm = np.ascontiguousarray(x[s].T)
        v1, _, c = spearman(xm)
        cs.append(c)
        for q, v in enumerate((pearson(xm)[0], v1, copresence(xm, ml)[0], cosine(P[s], A[s]))):
            series[q, s] = v[ia, ib]
    pair, n_credible, at, mx = reduce(series, ci)
    return dict(pair=pair, series=series, pairs=pairs, n_used=S, n_included=int(m), n_left_out=int(G - m), n_pairs=len(pairs),
                n_blocks=(m + BLOCK - 1) // BLOCK, n_credible=n_credible, max_cosine_at=at, max_cosine=mx, min_load=ml, credible_interval=ci,
                x=x, c=np.stack(cs), members=members)
