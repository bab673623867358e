"""The numerical spec of bnmf_stability restated in numpy float64: every operation in the order the spec names, written
from the document and not from the kernel.  Shared by tests/test_stability_host.py, tests/test_gpu_stability.py and the R shim's test."""
import numpy as np

from contrast_ref import canon64
from regress_ref import Refused, canonB

POINT_ROWS = ("silhouette", "a", "b", "nearest")
FACTOR_ROWS = ("members", "stability", "min_silhouette", "mean_a", "mean_b", "share_negative")
MAX_POINTS = 65536
INFO = ("n_used", "n_points", "n_extra", "n_left_out", "n_clusters", "min_stability_at", "n_negative", "mean_silhouette", "min_stability")


def points_of(P, A, labels=None, extra_P=None, extra_label=None):
    """the points: columns [NPT][K] (ring point (s, n) at s N + n, extra x at S N + x), their squared norms (k ascending from +0.0)
    and labels, -1 for a position that is left out"""
    P, A = np.asarray(P, dtype=np.float64), np.asarray(A, dtype=np.float64)
    S, K, N = P.shape
    lab = np.tile(np.arange(N), (S, 1)) if labels is None else np.asarray(labels, dtype=np.int64).reshape(S, N)
    if ((lab < -1) | (lab >= N)).any():
        raise Refused(-1, "a label outside -1 .. N-1")
    cols = np.ascontiguousarray(np.moveaxis(P, 1, 2)).reshape(S * N, K)
    lab = lab.reshape(S * N).copy()
    X = 0 if extra_P is None else np.asarray(extra_P).shape[1]
    if X:
        ex = np.asarray(extra_P, dtype=np.float64)
        el = np.asarray(extra_label, dtype=np.int64)
        if ((el < 0) | (el >= N)).any():
            raise Refused(-1, "an extra label outside 0 .. N-1")
        if not np.isfinite(ex).all() or (ex == 0).all(axis=0).any():
            raise Refused(-1, "an extra column that is not finite or all zero")
        cols = np.vstack([cols, ex.T])
        lab = np.concatenate([lab, el])
    nn = np.zeros(cols.shape[0])
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(K):
            nn = nn + cols[:, k] * cols[:, k]
    ring_ok = (A.reshape(S * N) != 0) & np.isfinite(nn[:S * N]) & (nn[:S * N] > 0)
    lab[:S * N][~ring_ok] = -1
    return cols, nn, lab, X


def distances(cols, nn):
    """d [M][M]: dot over k ascending from +0.0, multiply and add rounded separately; 1 - dot / sqrt(nn_i nn_i'); the diagonal +0.0"""
    M, K = cols.shape
    dot = np.zeros((M, M))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for k in range(K):
            dot = dot + cols[:, k][:, None] * cols[:, k][None, :]
        d = 1.0 - dot / np.sqrt(nn[:, None] * nn[None, :])
    d[np.arange(M), np.arange(M)] = 0.0
    return d


def finish(d, idx, lab, N, NPT, cols):
    """d [M][M] over the members (idx: their point indices ascending; lab: their labels) -> every output"""
    M = idx.size
    lists = [np.where(lab == j)[0] for j in range(N)]            # ring members ascending, then extras ascending: the index order
    m = np.array([l.size for l in lists])
    D = np.full((M, N), np.nan)
    for j in range(N):
        D[:, j] = canonB(d[lists[j]]) if m[j] else 0.0           # (d is bitwise symmetric: rows of the list, summed along the list)
    sil, a, b, near = np.zeros(M), np.zeros(M), np.full(M, np.nan), np.full(M, -1.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(M):
            c = lab[i]
            a[i] = D[i, c] / float(m[c] - 1) if m[c] >= 2 else 0.0
            for j in range(N):
                if j == c or m[j] < 1:
                    continue
                v = D[i, j] / float(m[j])
                if near[i] < 0 or v < b[i]:
                    b[i], near[i] = v, j
            if m[c] < 2:
                sil[i] = 0.0
            elif near[i] < 0:
                sil[i] = np.nan
            else:
                mx = a[i] if a[i] > b[i] else b[i]
                sil[i] = (b[i] - a[i]) / mx if mx > 0 else 0.0
        point = np.full((4, NPT), np.nan)
        point[3] = -1.0
        point[0, idx], point[1, idx], point[2, idx], point[3, idx] = sil, a, b, near
        K = cols.shape[1]
        factor = np.full((6, N), np.nan)
        between = np.full((N, N), np.nan)
        medoid, medoid_at = np.full((K, N), np.nan), np.full(N, -1, dtype=np.int64)
        for j in range(N):
            factor[0, j] = m[j]
            if not m[j]:
                continue
            l = lists[j]
            factor[1, j] = float(canon64(sil[l])) / float(m[j])
            factor[2, j] = np.nan if np.isnan(sil[l]).any() else sil[l].min()
            factor[3, j] = float(canon64(a[l])) / float(m[j])
            factor[4, j] = float(canon64(b[l])) / float(m[j])
            factor[5, j] = float((sil[l] < 0).sum()) / float(m[j])
            best = l[0]
            for q in l:
                if D[q, j] < D[best, j]:
                    best = q
            col = cols[best]
            tot = 0.0
            for k in range(K):
                tot = tot + col[k]
            medoid[:, j] = col / tot
            medoid_at[j] = idx[best]
        for p in range(N):
            for q in range(N):
                if m[p] and m[q]:
                    between[p, q] = factor[3, p] if p == q else float(canon64(D[lists[p], q] / float(m[q]))) / float(m[p])
    st = factor[1]
    at = -1
    for j in range(N):
        if not np.isnan(st[j]) and (at < 0 or st[j] < st[at]):
            at = j
    info = dict(n_points=M, n_clusters=int((m >= 1).sum()), n_negative=int((sil < 0).sum()), mean_silhouette=float(canon64(sil)) / float(M),
                min_stability=float(st[at]) if at >= 0 else float("nan"), min_stability_at=at)
    return dict(point=point, factor=factor, between=between, medoid=medoid, medoid_at=medoid_at, D=D, **info)


def stability_reference(P, A, labels=None, extra_P=None, extra_label=None):
    """P [S][K][N], A [S][N]: the USED samples, oldest first; labels [S][N] (the rows of the used samples) or None; extra_P [K][X],
    extra_label [X] or None.  Returns what Engine.stability returns, and D [M][N] over the members in index order; refuses (Refused)
    what the call refuses after its arguments' shapes."""
    S, K, N = np.asarray(P).shape
    if N < 2:
        raise Refused(-2, "N < 2")
    if S < 2:
        raise Refused(-2, "fewer than 2 used samples")
    cols, nn, lab, X = points_of(P, A, labels, extra_P, extra_label)
    idx = np.where(lab >= 0)[0]
    if idx.size < 2 or idx.size > MAX_POINTS:
        raise Refused(-2, "fewer than 2 members or more than MAX_POINTS")
    out = finish(distances(cols[idx], nn[idx]), idx, lab[idx], N, cols.shape[0], cols[idx])
    out.update(n_used=S, n_extra=X, n_left_out=cols.shape[0] - idx.size)
    return out
