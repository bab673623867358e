"""The numerical spec of bnmf_attribution restated in numpy float64: the same sample order, the same association of
every product and sum, the canonical W = 64 row sums in chunks of 128 rows (waic_ref.canon64_colsum) and the oracle's exported
canonical W = 1024 sum over the tumours.  Shared by tests/test_attribution_host.py (the restatement against its laws and on a planted
case) and tests/test_gpu_attribution.py / tests/test_rshim_attribution.py (the device against it, bit for bit).  Test infrastructure only."""
import numpy as np

from waic_ref import canon64_colsum

ROW_CHUNK = 128


def chunked_colsum(x):
    """the sum over the rows of x (K x G) of DESIGN.md 14 / 15: rows in chunks of 128, the canonical W = 64 sum inside a chunk, the
    first chunk's value then + the next chunk's, ascending"""
    t = None
    for k0 in range(0, x.shape[0], ROW_CHUNK):
        r = canon64_colsum(x[k0:k0 + ROW_CHUNK])
        t = r if t is None else t + r
    return t


def attribution_reference(P, E, A, M, likelihood, min_load=1.0, prob=True):
    """P [S][K][N], E [S][N][G], A [S][N], M [K][G]; samples oldest first.  Returns the outputs of bnmf_attribution: load (4 x N x G),
    its rows by name, prob (K x N x G), series (S x N), n_used, n_present, total; and for the tests' own bookkeeping c (S x K x G),
    x (S x K x N x G), a (S x N x G) and shares (S x N x G)."""
    import oracle
    P, E, A = (np.asarray(v, dtype=np.float64) for v in (P, E, A))
    S, K, N = P.shape
    G = E.shape[2]
    A = A.reshape(S, N)
    normal = likelihood == "normal"
    Md = np.asarray(M, dtype=np.float64)
    rsum = np.zeros((K, N, G))
    mu, m2, ssh = np.zeros((N, G)), np.zeros((N, G)), np.zeros((N, G))
    cnt = np.zeros((N, G), dtype=np.int64)
    series = np.empty((S, N))
    cs, xs, as_, shs = np.empty((S, K, G)), np.empty((S, K, N, G)), np.empty((S, N, G)), np.empty((S, N, G))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for s in range(S):
            f = np.empty((N, K, G))
            c = np.zeros((K, G))
            for n in range(N):                                   # n ascending from +0.0, (P * A) * E
                f[n] = (P[s, :, n] * A[s, n])[:, None] * E[s, n, :][None, :]
                c = c + f[n]
            q = np.where(c > 0.0, 1.0 / np.where(c > 0.0, c, 1.0), 0.0)
            a = np.empty((N, G))
            for n in range(N):
                r = f[n] * q
                rsum[:, n, :] = rsum[:, n, :] + r
                x = f[n] if normal else Md * r
                xs[s, :, n, :] = x
                a[n] = chunked_colsum(x)
            t = np.zeros(G)
            for n in range(N):
                t = t + a[n]
            u = np.where(t > 0.0, 1.0 / np.where(t > 0.0, t, 1.0), 0.0)
            share = a * u[None, :]
            d = a - mu
            mu = mu + d * (1.0 / float(s + 1))
            m2 = m2 + d * (a - mu)
            ssh = ssh + share
            cnt += a >= min_load
            for n in range(N):
                series[s, n] = oracle.canon_sum(np.ascontiguousarray(a[n]), 1024)
            cs[s], as_[s], shs[s] = c, a, share
    dS = float(S)
    load = np.stack([mu, m2 / float(S - 1), ssh / dS, cnt.astype(np.float64) / dS])
    tot = 0.0
    for s in range(S):
        for n in range(N):
            tot = tot + float(series[s, n])
    out = dict(load=load, load_mean=load[0], load_var=load[1], share=load[2], p_present=load[3], series=series, n_used=S,
               n_present=int((load[3] >= 0.5).sum()), total=tot / dS, min_load=float(min_load), c=cs, x=xs, a=as_, shares=shs)
    if prob:
        out["prob"] = rsum / dS
    return out
