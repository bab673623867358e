"""The numerical spec of bnmf_project restated in numpy float64: explicit loops over the steps, the rows k and (wherever a
sum runs over them) the factors n, vectorised over (sample, new tumour); the same order and association of every product and sum, k_map_colsum's canonical
W = 64 column sums of P (waic_ref.canon64_colsum), bnmf_attribution's statistics over the samples (tests/attribution_ref.py's) and
the oracle's exported canonical W = 1024 sum over the tumours.  Shared by tests/test_project_host.py (the restatement against its
laws) and tests/test_gpu_project.py / tests/test_rshim_project.py (the device against it, bit for bit).  Test infrastructure only."""
import numpy as np

from waic_ref import canon64_colsum


def renormalise(P, A):
    """x [S][K][N] = P / colsum, and part [S][N]: the factors that take part (A != 0 and colsum > 0)"""
    P, A = np.asarray(P, dtype=np.float64), np.asarray(A, dtype=np.float64)
    S, K, N = P.shape
    A = A.reshape(S, N)
    cs = np.stack([canon64_colsum(P[s]) for s in range(S)])
    part = (A != 0.0) & (cs > 0.0)
    with np.errstate(all="ignore"):
        x = P / cs[:, None, :]
    return x, part


def fitted(x, part, e):
    """c [S][K][J] = sum_n x[k,n] * e_n over the factors that take part, n ascending from +0.0"""
    S, K, N = x.shape
    c = np.zeros((S, K, e.shape[2]))
    with np.errstate(all="ignore"):
        for n in range(N):
            c = np.where(part[:, n][:, None, None], c + x[:, :, n][:, :, None] * e[:, n, :][:, None, :], c)
    return c


def refit(x, part, X, n_steps, trace=None):
    """The KL multiplicative update of DESIGN.md 17, steps 2-4.  x [S][K][N], part [S][N], X [K][J].  Returns e [S][N][J] and the
    change of the last step [S][J]; trace (a list) receives a copy of e after every step."""
    x, X = np.asarray(x, dtype=np.float64), np.asarray(X, dtype=np.float64)
    S, K, N = x.shape
    J = X.shape[1]
    t = np.zeros(J)
    for k in range(K):
        t = t + X[k]
    nin = part.sum(axis=1)
    with np.errstate(all="ignore"):
        e0 = t[None, :] / np.where(nin > 0, nin, 1).astype(np.float64)[:, None]
        e = np.where(part[:, :, None], e0[:, None, :], 0.0)
        d = np.zeros((S, J))
        for _ in range(n_steps):
            g = np.zeros((S, N, J))
            for k in range(K):
                c = np.zeros((S, J))
                for n in range(N):
                    c = np.where(part[:, n][:, None], c + x[:, k, n][:, None] * e[:, n, :], c)
                q = np.where(c > 0.0, X[k][None, :] / np.where(c > 0.0, c, 1.0), 0.0)
                g = g + x[:, k, :][:, :, None] * q[:, None, :]                 # per n: g_n = g_n + x[k,n] * q (read only where n takes part)
            en = np.where(part[:, :, None], e * g, 0.0)
            d = np.zeros((S, J))
            for n in range(N):
                v = np.abs(en[:, n, :] - e[:, n, :])
                d = np.where(v > d, v, d)
            e = en
            if trace is not None:
                trace.append(e.copy())
        change = np.where(t > 0.0, d / np.where(t > 0.0, t, 1.0), 0.0)
    return e, change


def project_reference(P, A, X, n_steps, min_load=1.0):
    """P [S][K][N], A [S][N] (samples oldest first), X [K][J].  Returns the outputs of bnmf_project: load (4 x N x J) and its rows by
    name, fit (3 x J) and its rows by name, series (S x N), exposures (S x N x J), the info fields; and for the tests' own
    bookkeeping cosines, rel_l1s, changes (S x J) and part (S x N)."""
    import oracle
    X = np.asarray(X, dtype=np.float64)
    K, J = X.shape
    x, part = renormalise(P, A)
    S, _, N = x.shape
    e, change = refit(x, part, X, n_steps)
    t = np.zeros(J)
    for k in range(K):
        t = t + X[k]
    c = fitted(x, part, e)
    dot, xx, cc, l1 = np.zeros((S, J)), np.zeros(J), np.zeros((S, J)), np.zeros((S, J))
    with np.errstate(all="ignore"):
        for k in range(K):
            dot = dot + X[k][None, :] * c[:, k, :]
            xx = xx + X[k] * X[k]
            cc = cc + c[:, k, :] * c[:, k, :]
            l1 = l1 + np.abs(X[k][None, :] - c[:, k, :])
        cosine = dot / np.sqrt(xx[None, :] * cc)
        rel_l1 = np.where(t > 0.0, l1 / np.where(t > 0.0, t, 1.0), 0.0)
        # the statistics over the samples: bnmf_attribution's, with G := J
        mu, m2, ssh = np.zeros((N, J)), np.zeros((N, J)), np.zeros((N, J))
        cnt = np.zeros((N, J), dtype=np.int64)
        series = np.empty((S, N))
        sc, sl, mx = np.zeros(J), np.zeros(J), np.zeros(J)
        for s in range(S):
            a = e[s]
            tt = np.zeros(J)
            for n in range(N):
                tt = tt + a[n]
            u = np.where(tt > 0.0, 1.0 / np.where(tt > 0.0, tt, 1.0), 0.0)
            dd = a - mu
            mu = mu + dd * (1.0 / float(s + 1))
            m2 = m2 + dd * (a - mu)
            ssh = ssh + a * u[None, :]
            cnt += a >= min_load
            for n in range(N):
                series[s, n] = oracle.canon_sum(np.ascontiguousarray(a[n]), 1024)
            sc = sc + cosine[s]
            sl = sl + rel_l1[s]
            mx = np.where(change[s] > mx, change[s], mx)
        dS = float(S)
        load = np.stack([mu, m2 / float(S - 1), ssh / dS, cnt.astype(np.float64) / dS])
        fit = np.stack([sc / dS, sl / dS, mx])
    tot = 0.0
    for s in range(S):
        for n in range(N):
            tot = tot + float(series[s, n])
    mrc, mc, mc_at = 0.0, float("nan"), -1
    for j in range(J):
        if fit[2, j] > mrc:
            mrc = float(fit[2, j])
        if not np.isnan(fit[0, j]) and (mc_at < 0 or fit[0, j] < mc):
            mc, mc_at = float(fit[0, j]), j
    return dict(load=load, load_mean=load[0], load_var=load[1], share=load[2], p_present=load[3], fit=fit, cosine=fit[0], rel_l1=fit[1],
                rel_change=fit[2], series=series, exposures=e, n_used=S, n_steps=int(n_steps), n_present=int((load[3] >= 0.5).sum()),
                min_load=float(min_load), total=tot / dS, max_rel_change=mrc, min_cosine=mc, min_cosine_at=mc_at,
                cosines=cosine, rel_l1s=rel_l1, changes=change, part=part)
