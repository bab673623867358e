"""The numerical spec of bnmf_reconstruction (include/bnmf.h) restated in numpy float64: the same sample order, the same
association of every product and sum (pre_n up the factors, suf_n down them, every sum over the mutation types ascending from +0.0),
Welford's update over the samples, the canonical W = 1024 sum over the tumours for the series and the canonical W = 64 sum for the
signature rows.  Loops in the stated order, vectorised over the tumours only.  Shared by tests/test_reconstruction_host.py (the
restatement against the matrix form and on a planted case) and tests/test_gpu_reconstruction.py / tests/test_rshim_reconstruction.py
(the device against it, bit for bit).  Test infrastructure only."""
import numpy as np


def canon(v, W):
    """the canonical sum of width W: accumulator l adds elements l, l + W, ... from +0.0, then the halving tree"""
    v = np.asarray(v, dtype=np.float64)
    acc = np.zeros(W)
    for i0 in range(0, len(v), W):
        part = v[i0:i0 + W]
        acc[:len(part)] = acc[:len(part)] + part
    h = W // 2
    while h >= 1:
        acc[:h] = acc[:h] + acc[h:2 * h]
        h //= 2
    return float(acc[0])


def _cosv(dot, cc, mm):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = dot / np.sqrt(mm * cc)
    return np.where(mm > 0.0, np.where(cc > 0.0, q, 0.0), np.nan)


def sample_values(P, E, A, Md):
    """one sample: P [K][N], E [N][G], A [N], Md [K][G] doubles -> cos (G), rel_l1 (G), rmse (G), cos_-n (N x G), drop_n (N x G)"""
    K, N = P.shape
    G = E.shape[1]
    mm, t = np.zeros(G), np.zeros(G)
    dot, cc, l1, sse = np.zeros(G), np.zeros(G), np.zeros(G), np.zeros(G)
    dotm, ccm = np.zeros((N, G)), np.zeros((N, G))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            m = Md[k]
            mm = mm + m * m
            t = t + np.abs(m)
            f = [(P[k, n] * A[n]) * E[n] for n in range(N)]
            pre = [np.zeros(G)]
            for n in range(N):
                pre.append(pre[n] + f[n])
            c = pre[N]
            d = m - c
            dot = dot + m * c
            cc = cc + c * c
            l1 = l1 + np.abs(d)
            sse = sse + d * d
            suf = np.zeros(G)
            for n in range(N - 1, -1, -1):
                cn = pre[n] + suf
                dotm[n] = dotm[n] + m * cn
                ccm[n] = ccm[n] + cn * cn
                suf = suf + f[n]
        cos = _cosv(dot, cc, mm)
        rel = np.where(t > 0.0, l1 / np.where(t > 0.0, t, 1.0), 0.0)
        rmse = np.sqrt(sse / float(K))
        cosm, drop = np.empty((N, G)), np.empty((N, G))
        for n in range(N):
            inc = A[n] != 0.0
            cosm[n] = _cosv(dotm[n], ccm[n], mm) if inc else cos
            drop[n] = cos - cosm[n] if inc else np.zeros(G)
    return cos, rel, rmse, cosm, drop, mm


def reconstruction_reference(P, E, A, M, min_cosine=0.9, min_drop=0.01):
    """P [S][K][N], E [S][N][G], A [S][N], M [K][G] (counts or real values); samples oldest first.  Returns the outputs of
    bnmf_reconstruction: tumour (6 x G), drop (4 x N x G), series (S), signature (3 x N) and the info fields; and for the tests' own
    bookkeeping cos (S x G), loo (S x N x G), drops (S x N x G), mm (G) and sums (S: the series before its division)."""
    P, E, A = (np.asarray(v, dtype=np.float64) for v in (P, E, A))
    S, K, N = P.shape
    G = E.shape[2]
    A = A.reshape(S, N)
    Md = np.asarray(M, dtype=np.float64)
    mu, m2, mn, ml, mr = np.zeros(G), np.zeros(G), np.full(G, np.inf), np.zeros(G), np.zeros(G)
    cnt = np.zeros(G, dtype=np.int64)
    dmu, dm2, cmu = np.zeros((N, G)), np.zeros((N, G)), np.zeros((N, G))
    dcnt = np.zeros((N, G), dtype=np.int64)
    sums = np.empty(S)
    coss, loos, drops = np.empty((S, G)), np.empty((S, N, G)), np.empty((S, N, G))
    mm = None
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(S):
            cos, rel, rmse, cosm, drop, mm = sample_values(P[s], E[s], A[s], Md)
            rs = 1.0 / float(s + 1)
            d = cos - mu
            mu = mu + d * rs
            m2 = m2 + d * (cos - mu)
            mn = np.where(cos < mn, cos, mn)
            ml = ml + (rel - ml) * rs
            mr = mr + (rmse - mr) * rs
            cnt += cos >= min_cosine
            d = drop - dmu
            dmu = dmu + d * rs
            dm2 = dm2 + d * (drop - dmu)
            cmu = cmu + (cosm - cmu) * rs
            dcnt += drop >= min_drop
            sums[s] = canon(np.where(mm > 0.0, cos, 0.0), 1024)
            coss[s], loos[s], drops[s] = cos, cosm, drop
    dS, dS1 = float(S), float(S - 1)
    defined = mm > 0.0
    nan = np.full(G, np.nan)
    tumour = np.stack([np.where(defined, mu, nan), np.where(defined, m2 / dS1, nan), np.where(defined, mn, nan), ml, mr,
                       np.where(defined, cnt.astype(np.float64) / dS, nan)])
    dr = np.stack([np.where(defined[None], v, np.nan) for v in (dmu, dm2 / dS1, cmu, dcnt.astype(np.float64) / dS)])
    ndef = int(defined.sum())
    series = sums / float(ndef) if ndef else np.full(S, np.nan)
    sig = np.full((3, N), np.nan)
    for n in range(N):
        sig[0, n] = float((dr[3, n] >= 0.5).sum())
        if ndef:
            v = dr[0, n][defined]
            sig[1, n] = canon(v, 64) / float(ndef)
            mx = v[0]
            for x in v[1:]:
                mx = x if x > mx else mx
            sig[2, n] = mx
    worst, at = np.nan, -1
    for g in range(G):
        if defined[g] and not np.isnan(tumour[0, g]) and (at < 0 or tumour[0, g] < worst):
            worst, at = float(tumour[0, g]), g
    return dict(tumour=tumour, drop=dr, series=series, signature=sig, n_used=S, n_undefined=G - ndef,
                n_poor=int((tumour[0][defined] < min_cosine).sum()), n_needed=int((dr[3] >= 0.5).sum()), min_cosine=float(min_cosine),
                min_drop=float(min_drop), worst_cosine=worst, worst_at=at, cos=coss, loo=loos, drops=drops, mm=mm, sums=sums)
