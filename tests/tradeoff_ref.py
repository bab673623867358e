"""The numerical spec of bnmf_tradeoff (include/bnmf.h) restated in numpy float64, operation for operation: bnmf_contrast's
renormalised exposures, their alignment by perm, the mean over the matched samples (t ascending from +0.0), the co-moments (the product
rounded before it is added, t ascending), the correlations and what follows from them per tumour (the smallest defined correlation, the
variance ratio of the total, the sets), bnmf_regress's blocked canonical sum over the positions of the member list for the pair rows.
Explicit ascending loops over the samples, the factors and the sets in the stated order, vectorised over the tumours (an
order-preserving form: every element sees the scalar sequence of operations).  Shared by tests/test_tradeoff_host.py and
tests/test_gpu_tradeoff.py / tests/test_rshim_tradeoff.py (the device against it, bit for bit).  Test infrastructure only."""
import numpy as np

from contrast_ref import canon64
from regress_ref import BLOCK, canonB
from subtypes_ref import Refused, loads

MAX_C, MAX_N = 32, 128
assert BLOCK == 1024


def aligned(x, perm):
    """x [S'][N][m] and the perm rows of the matched samples (or None) -> q [S'][N][m]: q_t[perm[t][n]] = x_t[n]"""
    if perm is None:
        return x
    q = np.empty_like(x)
    for t in range(x.shape[0]):
        for n in range(x.shape[1]):
            q[t, int(perm[t][n])] = x[t, n]
    return q


def covariances(q):
    """q [S'][N][m] -> mu [N][m], cov [N][N][m] (bitwise symmetric)"""
    Sm, N, m = q.shape
    with np.errstate(invalid="ignore", over="ignore"):
        tot = np.zeros((N, m))
        for t in range(Sm):
            tot = tot + q[t]
        mu = tot / float(Sm)
        d = q - mu[None]
        cov = np.zeros((N, N, m))
        for j in range(N):
            for l in range(j + 1):
                acc = np.zeros(m)
                for t in range(Sm):
                    acc = acc + d[t, j] * d[t, l]
                cov[j, l] = cov[l, j] = acc / float(Sm - 1)
    return mu, cov


def correlations(cov):
    """cov [N][N][m] -> r [N][N][m] (NaN where undefined and on the diagonal), defined [N][N][m]"""
    N = cov.shape[0]
    r, ok = np.full(cov.shape, np.nan), np.zeros(cov.shape, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        for j in range(N):
            for l in range(N):
                if j == l:
                    continue
                pr = cov[j, j] * cov[l, l]
                ok[j, l] = (pr > 0) & (pr < np.inf)
                r[j, l] = np.where(ok[j, l], cov[j, l] / np.sqrt(np.where(ok[j, l], pr, 1.0)), np.nan)
    return r, ok


def per_tumour(mu, cov, r, ok, sets, C):
    """tum [3][m], pair_at [m], setstat [4][C][m] in member order"""
    N, _, m = cov.shape
    best, at, ndef = np.full(m, np.nan), np.full(m, -1, dtype=np.int32), np.zeros(m)
    vt, sv = np.zeros(m), np.zeros(m)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(N):
            inner = np.zeros(m)
            for l in range(N):
                inner = inner + cov[j, l]
                if l < j:
                    win = ok[j, l] & ((at < 0) | (r[j, l] < best))
                    best = np.where(win, r[j, l], best)
                    at = np.where(win, j * N + l, at).astype(np.int32)
                    ndef = ndef + ok[j, l]
            vt = vt + inner
            sv = sv + cov[j, j]
        good = (sv > 0) & (sv < np.inf)
        tum = np.stack([best, ndef, np.where(good, vt / np.where(good, sv, 1.0), np.nan)])
        sst = np.full((4, C, m), np.nan)
        for c in range(C):
            s0, s1, s2 = np.zeros(m), np.zeros(m), np.zeros(m)
            for j in range(N):
                if sets[j] != c:
                    continue
                s0 = s0 + mu[j]
                inner = np.zeros(m)
                for l in range(N):
                    if sets[l] == c:
                        inner = inner + cov[j, l]
                s1 = s1 + inner
                s2 = s2 + cov[j, j]
            good = (s2 > 0) & (s2 < np.inf)
            sst[:, c] = s0, s1, s2, np.where(good, s1 / np.where(good, s2, 1.0), np.nan)
    return tum, at, sst


def pairs(cov, r, ok, min_corr):
    """pair [5][N][N] over the members, strongest_pair, strongest_pair_at"""
    N, _, m = cov.shape
    pair = np.full((5, N, N), np.nan)
    strongest, at = np.nan, -1
    for j in range(N):
        for l in range(j):
            nd = int(ok[j, l].sum())
            row = [float(canonB(np.where(ok[j, l], r[j, l], 0.0))) / float(nd) if nd else np.nan, float(nd),
                   float((ok[j, l] & (r[j, l] <= -min_corr)).sum()) / float(nd) if nd else np.nan,
                   float((ok[j, l] & (r[j, l] >= min_corr)).sum()) / float(nd) if nd else np.nan, float(canonB(cov[j, l])) / float(m)]
            pair[:, j, l] = pair[:, l, j] = row
            if not np.isnan(row[0]) and (at < 0 or row[0] < strongest):
                strongest, at = row[0], j * N + l
    return pair, strongest, at


def tradeoff_reference(P, E, A, include=None, perm=None, sets=None, query=None, min_corr=0.5):
    """P [S][K][N], E [S][N][G], A [S][N]: the USED samples, oldest first; perm [S][N] (the rows of the used samples) or None; sets [N]
    or None.  Returns the outputs of bnmf_tradeoff as Engine.tradeoff returns them (pair 5 x N x N, setstat 4 x C x G, dense Q x 2 x N x
    N), the info fields, and mu, cov, r in member order; refuses (Refused) what the call refuses after its arguments' shapes."""
    E = np.asarray(E, dtype=np.float64)
    S, N, G = E.shape
    inc = np.ones(G, dtype=np.int64) if include is None else np.asarray(include, dtype=np.int64)
    if ((inc != 0) & (inc != 1)).any():
        raise Refused(-1, "include is neither 0 nor 1")
    members = np.where(inc == 1)[0]
    m = len(members)
    st = None if sets is None else np.asarray(sets, dtype=np.int64)
    C = 0 if st is None else int(st.max()) + 1
    if C > MAX_C or (st is not None and ((st < -1).any() or any((st == c).sum() == 0 for c in range(C)))):
        raise Refused(-1, "sets")
    q_ = np.zeros(0, dtype=np.int64) if query is None else np.asarray(query, dtype=np.int64).reshape(-1)
    if ((q_ < 0) | (q_ >= G)).any() or (inc[q_] == 0).any():
        raise Refused(-1, "query")
    if not (0.0 <= min_corr <= 1.0):
        raise Refused(-1, "min_corr")
    matched = []
    for s in range(S):
        if perm is not None:
            row = np.asarray(perm[s])
            if (row == -1).all():
                continue
            if sorted(row.tolist()) != list(range(N)):
                raise Refused(-1, f"perm row {s}")
        matched.append(s)
    if S < 2 or len(matched) < 2 or m < 1 or N > MAX_N:
        raise Refused(-2, "size")
    x = loads(P, E, A)[:, :, members][matched]
    q = aligned(x, None if perm is None else [perm[s] for s in matched])
    mu, cov = covariances(q)
    r, ok = correlations(cov)
    tum, at, sst = per_tumour(mu, cov, r, ok, st, C)
    pair, strongest, strongest_at = pairs(cov, r, ok, min_corr)
    tumour, pair_at, setstat = np.full((3, G), np.nan), np.full(G, -1, dtype=np.int32), np.full((4, C, G), np.nan)
    tumour[:, members], pair_at[members], setstat[:, :, members] = tum, at, sst
    place = {int(g): i for i, g in enumerate(members)}
    dense = np.empty((len(q_), 2, N, N))
    for k, g in enumerate(q_):
        dense[k, 0], dense[k, 1] = cov[:, :, place[int(g)]], r[:, :, place[int(g)]]
    ratio = tum[2][~np.isnan(tum[2])]
    with np.errstate(invalid="ignore"):
        traded = int((tum[0] <= -min_corr).sum())
    return dict(tumour=tumour, pair_at=pair_at, pair=pair, setstat=setstat, dense=dense, n_used=S, n_matched=len(matched), n_unmatched=S - len(matched),
                n_included=m, n_left_out=G - m, n_sets=C, n_query=len(q_), n_traded=traded, strongest_pair_at=strongest_at, strongest_pair=strongest,
                mean_ratio=float(canon64(ratio)) / float(len(ratio)) if len(ratio) else np.nan, min_corr=float(min_corr), members=members, mu=mu, cov=cov, r=r)
