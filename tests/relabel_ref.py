"""The numerical spec of bnmf_relabel restated in numpy float64, operation for operation: the cosines with explicit loops
over k (vectorised over the N x N pairs), the assignment by the sequential shortest-augmenting-path algorithm with potentials and the
lowest column among equal reduced costs (what hungarian_wave computes with its columns spread over the lanes), the canonical W = 64 order
for every sum.  Only + - * / and sqrt, which numpy rounds correctly as the device does, so the device must give these bits.  Shared by
tests/test_relabel_host.py, tests/test_gpu_relabel.py and tests/test_rshim_relabel.py.  Test infrastructure only."""
import numpy as np

from waic_ref import canon64_colsum

INF = 1e300
INFO = ("n_used", "n_aligned", "n_unmatched", "rounds", "converged", "n_switched", "n_changed_last", "mean_cosine", "min_cosine", "min_cosine_at")


def cosine_matrix(P, pivot):
    """C[n][j] = dot / sqrt(nn * refnorm2[j]) of the raw P (K x N) against the pivot (K x N; or a catalogue, K x R: bnmf_assign's cosines,
    tests/map_ref.py): k ascending from +0.0 (k_ref_cosine; refnorm2 as the host sums it)"""
    P, pivot = np.asarray(P, dtype=np.float64), np.asarray(pivot, dtype=np.float64)
    K, N = P.shape
    R = pivot.shape[1]
    dot, nn, rn2 = np.zeros((N, R)), np.zeros(N), np.zeros(R)
    for k in range(K):
        dot = dot + P[k][:, None] * pivot[k][None, :]
        nn = nn + P[k] * P[k]
        rn2 = rn2 + pivot[k] * pivot[k]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return dot / np.sqrt(nn[:, None] * rn2[None, :])


def hungarian(C):
    """The assignment row -> column of C (n rows <= m columns) that maximises the total (cost = -C): rows inserted in order, shortest
    augmenting path with potentials, strict comparisons over ascending columns, so the lowest column wins among equals.  None when no
    finite reduced cost is left (a NaN in C).  With more rows than columns hungarian_wave takes the transposed matrix: so does the caller."""
    C = np.asarray(C, dtype=np.float64)
    n, m = C.shape
    assert n <= m
    u, v = np.zeros(n + 1), np.zeros(m + 1)
    p, way = np.zeros(m + 1, dtype=int), np.zeros(m + 1, dtype=int)
    for i in range(1, n + 1):
        p[0] = i
        minv = np.full(m + 1, INF)
        used = np.zeros(m + 1, dtype=bool)
        j0 = 0
        while True:
            used[j0] = True
            i0 = p[j0]
            free = ~used[1:]
            with np.errstate(invalid="ignore", over="ignore"):
                cur = ((-C[i0 - 1]) - u[i0]) - v[1:]
                upd = free & (cur < minv[1:])
            minv[1:][upd] = cur[upd]
            way[1:][upd] = j0
            cand = np.where(free, minv[1:], np.inf)
            j1 = None
            delta = INF
            if (cand < INF).any():
                j1 = int(np.argmin(cand)) + 1                  # the first of equals
                delta = cand[j1 - 1]
            with np.errstate(over="ignore", invalid="ignore"):
                uj = np.where(used)[0]
                u[p[uj]] = u[p[uj]] + delta
                v[uj] = v[uj] - delta
                minv[~used] = minv[~used] - delta
            if j1 is None:
                return None
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            jn = way[j0]
            p[j0] = p[jn]
            j0 = jn
    perm = np.empty(n, dtype=np.int32)
    matched = p[1:] > 0                                        # (m - n columns stay free)
    perm[p[1:][matched] - 1] = np.arange(m, dtype=np.int32)[matched]
    return perm


def hungarian_scalar(C):
    """the same algorithm with a Python loop over the columns (the text-book form): the vectorised one above must agree with it"""
    C = np.asarray(C, dtype=np.float64)
    n, m = C.shape
    assert n <= m
    u, v, p, way = [0.0] * (n + 1), [0.0] * (m + 1), [0] * (m + 1), [0] * (m + 1)
    for i in range(1, n + 1):
        p[0] = i
        minv, used, j0 = [INF] * (m + 1), [False] * (m + 1), 0
        while True:
            used[j0] = True
            i0, delta, j1 = p[j0], INF, None
            for j in range(1, m + 1):
                if not used[j]:
                    cur = ((-float(C[i0 - 1, j - 1])) - u[i0]) - v[j]
                    if cur < minv[j]:
                        minv[j], way[j] = cur, j0
                    if minv[j] < delta:
                        delta, j1 = minv[j], j
            for j in range(m + 1):
                if used[j]:
                    u[p[j]] = u[p[j]] + delta
                    v[j] = v[j] - delta
                else:
                    minv[j] = minv[j] - delta
            if j1 is None:
                return None
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            jn = way[j0]
            p[j0] = p[jn]
            j0 = jn
    perm = np.empty(n, dtype=np.int32)
    for j in range(1, m + 1):
        if p[j]:
            perm[p[j] - 1] = j - 1
    return perm


def renormalised(Pw, Ew):
    """cs_s = k_map_colsum, x = P / cs, e = E * cs: [S][K][N], [S][N][G]"""
    Pw, Ew = np.asarray(Pw, dtype=np.float64), np.asarray(Ew, dtype=np.float64)
    cs = np.stack([canon64_colsum(Pw[s]) for s in range(Pw.shape[0])])
    with np.errstate(divide="ignore", invalid="ignore"):
        return Pw / cs[:, None, :], Ew * cs[:, :, None]


def _moments(series):
    """series [S'][L] -> mean, var by mixing.h's expressions"""
    Sa = series.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        mu = canon64_colsum(series) / float(Sa)
        d = series - mu[None, :]
        return mu, canon64_colsum(d * d) / float(Sa - 1)


def relabel_reference(Pw, Ew, pivot=None, max_rounds=10, solver=hungarian):
    """Pw [S][K][N], Ew [S][N][G]: the used samples, oldest first.  Returns every output of bnmf_relabel by name (P_mean, P_var K x N;
    E_mean, E_var N x G; aligned_P [S][K][N], aligned_E [S][N][G]; perm, cosine [S][N]; confusion [N][N]), the info fields, and
    history: the permutations after every round."""
    Pw, Ew = np.asarray(Pw, dtype=np.float64), np.asarray(Ew, dtype=np.float64)
    S, K, N = Pw.shape
    G = Ew.shape[2]
    assert max_rounds >= 1 and S >= 2
    x, e = renormalised(Pw, Ew)
    piv = Pw[S - 1] if pivot is None else np.asarray(pivot, dtype=np.float64)
    prev = np.tile(np.arange(N, dtype=np.int32), (S, 1))
    history = []
    rounds = converged = changed = 0
    for r in range(1, max_rounds + 1):
        perm, cosv = np.full((S, N), -1, dtype=np.int32), np.full((S, N), np.nan)
        for s in range(S):
            C = cosine_matrix(Pw[s], piv)
            pm = solver(C)
            if pm is not None:
                perm[s], cosv[s] = pm, C[np.arange(N), pm]
        al = np.where(perm[:, 0] >= 0)[0]
        if al.size < 2:
            raise ValueError(f"{al.size} aligned samples in round {r}")
        changed = int((perm[al] != prev[al]).any(axis=1).sum())
        prev = perm
        history.append(perm.copy())
        rounds = r
        inv = np.full((S, N), -1, dtype=np.int32)
        for s in al:
            inv[s, perm[s]] = np.arange(N, dtype=np.int32)
        if changed == 0:
            converged = 1
            break
        if r == max_rounds:
            break
        xa = np.stack([x[s][:, inv[s]] for s in al])
        piv = _moments(xa.transpose(0, 2, 1).reshape(al.size, -1))[0].reshape((K, N), order="F")
    aP, aE = np.full((S, K, N), np.nan), np.full((S, N, G), np.nan)
    for s in al:
        aP[s], aE[s] = x[s][:, inv[s]], e[s][inv[s], :]
    Pm, Pv = _moments(aP[al].transpose(0, 2, 1).reshape(al.size, -1))
    Em, Ev = _moments(aE[al].transpose(0, 2, 1).reshape(al.size, -1))
    conf = np.zeros((N, N), dtype=np.int64)
    for s in al:
        conf[np.arange(N), perm[s]] += 1
    fc = cosv[al].reshape(-1)
    with np.errstate(invalid="ignore"):
        mean_cos = float(canon64_colsum(fc[:, None])[0] / float(al.size * N))
    at = int(np.argmin(fc))                                    # the first of equals
    return dict(perm=perm, cosine=cosv, confusion=conf, P_mean=Pm.reshape((K, N), order="F"), P_var=Pv.reshape((K, N), order="F"),
                E_mean=Em.reshape((N, G), order="F"), E_var=Ev.reshape((N, G), order="F"), aligned_P=aP, aligned_E=aE,
                n_used=S, n_aligned=int(al.size), n_unmatched=int(S - al.size), rounds=rounds, converged=converged,
                n_switched=int((perm[al] != np.arange(N)[None, :]).any(axis=1).sum()), n_changed_last=changed,
                mean_cosine=mean_cos, min_cosine=float(fc[at]), min_cosine_at=int(al[at // N]) * N + at % N, history=history)
