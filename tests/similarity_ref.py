"""The numerical spec of bnmf_similarity (include/bnmf.h) restated in numpy float64, operation for operation: bnmf_contrast's
renormalised exposures, nn and dot over the factors ascending from +0.0 with the multiply and the add rounded separately, the cosine with
its +0.0 convention, Welford's update over the samples, the top-k under the total order (mean descending, lower tumour first, a NaN never
listed), bnmf_regress's blocked canonical sum over the member list for the typicality and the canonical W = 64 sum for the mean
similarity.  Loops over the samples and the factors in the stated order, vectorised over the pairs (an order-preserving form: every
element sees the scalar sequence of operations).  Shared by tests/test_similarity_host.py (the restatement against the matrix form and on
planted cases) and tests/test_gpu_similarity.py / tests/test_rshim_similarity.py (the device against it, bit for bit).  Test
infrastructure only."""
import numpy as np

from contrast_ref import canon64
from regress_ref import canonB
from waic_ref import canon64_colsum

MAX_K = 32


def loads(P, E, A):
    """x [S][N][G]: bnmf_contrast's renormalised exposures"""
    P, E, A = np.asarray(P, dtype=np.float64), np.asarray(E, dtype=np.float64), np.asarray(A, dtype=np.float64)
    S = E.shape[0]
    A = A.reshape(S, -1)
    cs = np.stack([canon64_colsum(P[s]) for s in range(S)])                       # k_map_colsum
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where((A != 0)[:, :, None], E * cs[:, :, None], 0.0)


def sample_cosines(x):
    """one sample: x [N][m] -> c [m][m]"""
    N, m = x.shape
    nn, dot = np.zeros(m), np.zeros((m, m))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for n in range(N):
            nn = nn + x[n] * x[n]
            dot = dot + x[n][:, None] * x[n][None, :]
        pr = nn[:, None] * nn[None, :]
        return np.where(pr == 0.0, 0.0, dot / np.sqrt(np.where(pr == 0.0, 1.0, pr)))


def pair_statistics(x, min_cosine):
    """x [S][N][m] -> mean, var, p_similar (m x m each; the diagonal is computed like any pair and ignored by the callers), c (S x m x m)"""
    S, N, m = x.shape
    mu, m2 = np.zeros((m, m)), np.zeros((m, m))
    cnt = np.zeros((m, m), dtype=np.int64)
    cs = np.empty((S, m, m))
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(S):
            c = sample_cosines(x[s])
            rs = 1.0 / float(s + 1)
            d = c - mu
            mu = mu + d * rs
            m2 = m2 + d * (c - mu)
            cnt += c >= min_cosine
            cs[s] = c
        return mu, m2 / float(S - 1), cnt.astype(np.float64) / float(S), cs


def top_neighbours(mean, i, k):
    """the places of the k members ahead of all others for member i: mean descending, the lower place first; a NaN is no candidate"""
    cand = [j for j in range(len(mean)) if j != i and not np.isnan(mean[j])]
    cand.sort(key=lambda j: (-mean[j], j))                                         # (-0.0 and +0.0 compare equal: the place decides)
    return cand[:k]


def similarity_reference(P, E, A, include=None, query=None, top_k=10, min_cosine=0.9, tumour=True):
    """P [S][K][N], E [S][N][G], A [S][N]; samples oldest first.  Returns the outputs of bnmf_similarity: neighbour_at (G x top_k),
    neighbour (3 x G x top_k), dense (3 x Q x G), tumour (3 x G) and the info fields; and for the tests' own bookkeeping members, mean,
    var, p (m x m) and c (S x m x m)."""
    E = np.asarray(E, dtype=np.float64)
    S, N, G = E.shape
    members = np.arange(G) if include is None else np.where(np.asarray(include) != 0)[0]
    m = len(members)
    q = np.zeros(0, dtype=np.int64) if query is None else np.asarray(query, dtype=np.int64).reshape(-1)
    Q, k = len(q), int(top_k)
    x = loads(P, E, A)[:, :, members]
    mean, var, p, c = pair_statistics(x, min_cosine)
    place = {int(g): i for i, g in enumerate(members)}
    out = dict(n_used=S, n_included=m, n_left_out=G - m, top_k=k, n_query=Q, n_pairs=m * (m - 1) // 2, min_cosine=float(min_cosine),
               n_similar_pairs=-1, n_isolated=-1, mean_similarity=np.nan, least_typical=np.nan, least_typical_at=-1,
               members=members, mean=mean, var=var, p=p, c=c)
    dense = np.full((3, Q, G), np.nan)
    for qi, g in enumerate(q):
        i = place[int(g)]
        for r, tab in enumerate((mean, var, p)):
            row = tab[i].copy()
            row[i] = np.nan
            dense[r, qi, members] = row
    out["dense"] = dense
    if k == 0 and not tumour and Q > 0:                                            # the queries alone: the pass over all pairs does not run
        return out
    nat, nb, tum = np.full((G, k), -1, dtype=np.int32), np.full((3, G, k), np.nan), np.full((3, G), np.nan)
    deg_total, iso, least, at = 0, 0, np.nan, -1
    typ = np.empty(m)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, g in enumerate(members):
            best = top_neighbours(mean[i], i, max(k, 1))
            for t, j in enumerate(best[:k]):
                nat[g, t] = members[j]
                nb[:, g, t] = mean[i, j], var[i, j], p[i, j]
            v = mean[i].copy()
            v[i] = 0.0                                                             # the self term entered as +0.0
            typ[i] = float(canonB(v)) / float(m - 1)
            deg = int(sum(1 for j in range(m) if j != i and p[i, j] >= 0.5))
            tum[:, g] = typ[i], (mean[i, best[0]] if best else np.nan), float(deg)
            deg_total += deg
            iso += deg == 0
            if not np.isnan(typ[i]) and (at < 0 or typ[i] < least):
                least, at = float(typ[i]), int(g)
        out.update(neighbour_at=nat, neighbour=nb, tumour=tum, n_similar_pairs=deg_total // 2, n_isolated=int(iso),
                   mean_similarity=float(canon64(typ)) / float(m), least_typical=least, least_typical_at=at)
    return out
