"""The numerical spec of bnmf_decompose restated in numpy float64: explicit loops over the steps and the rows k and, inside
every sum over them, the references r; vectorised over (sample, factor) only; the same order and association of every product and sum,
k_map_colsum's canonical W = 64 column sums of P (waic_ref.canon64_colsum) and bnmf_attribution's statistics over the samples
(tests/attribution_ref.py's, with N := R and G := N).  Shared by tests/test_decompose_host.py (the restatement against its laws) and
tests/test_gpu_decompose.py / tests/test_rshim_decompose.py (the device against it, bit for bit).  Test infrastructure only."""
import numpy as np

from waic_ref import canon64_colsum


def normalise_catalogue(ref):
    """z [K][R] = ref / rs, rs[r] = sum_k ref[k,r] with k ascending from +0.0"""
    ref = np.asarray(ref, dtype=np.float64)
    rs = np.zeros(ref.shape[1])
    for k in range(ref.shape[0]):
        rs = rs + ref[k]
    return ref / rs[None, :]


def columns(P, A, keep=None):
    """y [K][S][N] = P_s[k,n] / cs[n] and part [S][N]: the factors that take part (keep != 0, A != 0 and colsum > 0); y is +0.0 for a
    factor that does not (its column is not read)"""
    P, A = np.asarray(P, dtype=np.float64), np.asarray(A, dtype=np.float64)
    S, K, N = P.shape
    A = A.reshape(S, N)
    cs = np.stack([canon64_colsum(P[s]) for s in range(S)])
    part = (A != 0.0) & (cs > 0.0)
    if keep is not None:
        part = part & (np.asarray(keep).reshape(1, N) != 0)
    with np.errstate(all="ignore"):
        y = np.where(part[:, None, :], P / np.where(part, cs, 1.0)[:, None, :], 0.0)
    return np.ascontiguousarray(y.transpose(1, 0, 2)), part


def total(y):
    t = np.zeros(y.shape[1:])
    for k in range(y.shape[0]):
        t = t + y[k]
    return t


def fitted(z, w):
    """c [K][S][N] = sum_r z[k,r] * w_r, r ascending from +0.0"""
    K, R = z.shape
    c = np.zeros((K,) + w.shape[1:])
    tmp = np.empty(w.shape[1:])
    for k in range(K):
        for r in range(R):
            np.multiply(z[k, r], w[r], out=tmp)
            np.add(c[k], tmp, out=c[k])
    return c


def prune(w, t, min_share):
    """the active set [R][S][N] of DESIGN.md 18 step 4: w_r >= min_share * t, else the first largest"""
    R = w.shape[0]
    active = w >= (min_share * t)[None]
    none = ~active.any(axis=0)
    best, bi = w[0].copy(), np.zeros(w.shape[1:], dtype=np.int64)
    for r in range(1, R):
        m = w[r] > best
        best, bi = np.where(m, w[r], best), np.where(m, r, bi)
    for r in range(R):
        active[r] |= none & (bi == r)
    return active


def refit(z, y, n_steps, min_share, trace=None):
    """The two-stage KL multiplicative update of DESIGN.md 18, steps 2-6.  z [K][R], y [K][S][N].  Returns w [R][S][N], the d of the
    last step performed [S][N] and the active set [R][S][N]; trace (a list) receives (stage, a copy of w) after every step."""
    z, y = np.asarray(z, dtype=np.float64), np.asarray(y, dtype=np.float64)
    K, R = z.shape
    shp = y.shape[1:]
    t = total(y)
    w = np.empty((R,) + shp)
    w[:] = t / float(R)
    active = np.ones((R,) + shp, dtype=bool)
    d = np.zeros(shp)
    tmp, tmp3 = np.empty(shp), np.empty((R,) + shp)
    with np.errstate(all="ignore"):
        for stage in range(2 if min_share != 0.0 else 1):
            if stage == 1:
                active = prune(w, t, min_share)
                w = np.where(active, w, 0.0)
            for _ in range(n_steps):
                g = np.zeros((R,) + shp)
                for k in range(K):
                    c = np.zeros(shp)
                    for r in range(R):
                        np.multiply(z[k, r], w[r], out=tmp)
                        np.add(c, tmp, out=c)
                    q = np.where(c > 0.0, y[k] / np.where(c > 0.0, c, 1.0), 0.0)
                    np.multiply(z[k].reshape((R,) + (1,) * len(shp)), q[None], out=tmp3)      # per r: g_r = g_r + z[k,r] * q
                    np.add(g, tmp3, out=g)
                wn = np.where(active, w * g, 0.0)
                d = np.zeros(shp)
                for r in range(R):
                    v = np.abs(wn[r] - w[r])
                    d = np.where(v > d, v, d)
                w = wn
                if trace is not None:
                    trace.append((stage, w.copy()))
    return w, d, active


def decompose_reference(P, A, ref, n_steps, min_share=0.05, keep=None):
    """P [S][K][N], A [S][N] (samples oldest first), ref [K][R].  Returns the outputs of bnmf_decompose: weight (4 x R x N) and its rows
    by name, fit (3 x N) and its rows by name, nactive (S x N), included (N), weights (S x R x N), the info fields; and for the tests'
    own bookkeeping cosines, rel_l1s, changes (S x N) and part (S x N)."""
    z = normalise_catalogue(ref)
    K, R = z.shape
    y, part = columns(P, A, keep)
    S, N = part.shape
    w, d, active = refit(z, y, n_steps, min_share)
    t = total(y)
    c = fitted(z, w)
    dot, yy, cc, l1 = np.zeros((S, N)), np.zeros((S, N)), np.zeros((S, N)), np.zeros((S, N))
    with np.errstate(all="ignore"):
        for k in range(K):
            dot = dot + y[k] * c[k]
            yy = yy + y[k] * y[k]
            cc = cc + c[k] * c[k]
            l1 = l1 + np.abs(y[k] - c[k])
        cosine = np.where(part, dot / np.sqrt(yy * cc), np.nan)
        rel_l1 = np.where(part, l1 / np.where(part, t, 1.0), 0.0)
        change = np.where(part, d / np.where(part, t, 1.0), 0.0)
        ws = np.where(part[:, None, :], w.transpose(1, 0, 2), 0.0)                    # [S][R][N]
        nactive = np.where(part, active.sum(axis=0), 0).astype(np.int32)
        # the statistics over the samples: bnmf_attribution's, with N := R and G := N
        mu, m2, ssh = np.zeros((R, N)), np.zeros((R, N)), np.zeros((R, N))
        cnt = np.zeros((R, N), dtype=np.int64)
        sc, sl, mx = np.zeros(N), np.zeros(N), np.zeros(N)
        for s in range(S):
            a = ws[s]
            tt = np.zeros(N)
            for r in range(R):
                tt = tt + a[r]
            u = np.where(tt > 0.0, 1.0 / np.where(tt > 0.0, tt, 1.0), 0.0)
            dd = a - mu
            mu = mu + dd * (1.0 / float(s + 1))
            m2 = m2 + dd * (a - mu)
            ssh = ssh + a * u[None, :]
            cnt += a >= min_share
            sc = sc + cosine[s]
            sl = sl + rel_l1[s]
            mx = np.where(change[s] > mx, change[s], mx)
        dS = float(S)
        weight = np.stack([mu, m2 / float(S - 1), ssh / dS, cnt.astype(np.float64) / dS])
        fit = np.stack([sc / dS, sl / dS, mx])
    mrc, mc, mc_at = 0.0, float("nan"), -1
    for n in range(N):
        if fit[2, n] > mrc:
            mrc = float(fit[2, n])
        if not np.isnan(fit[0, n]) and (mc_at < 0 or fit[0, n] < mc):
            mc, mc_at = float(fit[0, n]), n
    return dict(weight=weight, weight_mean=weight[0], weight_var=weight[1], share=weight[2], p_present=weight[3], fit=fit, cosine=fit[0],
                rel_l1=fit[1], rel_change=fit[2], nactive=nactive, included=part.sum(axis=0).astype(np.int32), weights=ws, n_used=S,
                n_steps=int(n_steps), R=R, n_present=int((weight[3] >= 0.5).sum()), min_share=float(min_share), max_rel_change=mrc,
                min_cosine=mc, min_cosine_at=mc_at, cosines=cosine, rel_l1s=rel_l1, changes=change, part=part)
