"""The numerical spec of bnmf_map and bnmf_assign (map_impl / assign_impl in csrc/api.hip, k_map_colsum, k_map_stats, k_map_quant,
k_map_fit, k_ref_cosine and hungarian_wave in csrc/kernels.h; DESIGN.md "bnmf_map" and "Posterior ranges") restated in numpy float64,
operation for operation and with no operation fused: + - * / sqrt, compare and sort, which numpy rounds as the device does, and the
project's log (the oracle's vec("log", .), which the device matches bit for bit).  The device must give these bits.  Shared by
tests/test_map_host.py, tests/test_gpu_map_bits.py and tests/test_gpu_assign_bits.py.  Test infrastructure only."""
from collections import Counter

import numpy as np

from relabel_ref import cosine_matrix, hungarian
from waic_ref import canon64_colsum, seq_sum

MAP_ARRAYS = ("P", "E", "A", "used", "top_A", "P_lower", "P_upper", "E_lower", "E_upper")
MAP_INFO = ("n_used", "n_patterns", "top_counts", "rmse", "kl")
ASSIGN_ARRAYS = ("votes", "assigned", "MAP_cosine", "lower_cosine", "upper_cosine")
TINY = 1e-6


def oracle_log(x):
    """the project's log: dlog on the device, orc_log in the oracle (tests/test_gpu_parity.py::test_math_bitexact_vs_oracle)"""
    import oracle
    return oracle.vec("log", x)


def mode_of_A(Aw):
    """Aw [last_n][N].  The patterns as '0' / '1' strings, most frequent first, ties alphabetical (get_mode): returns the table
    [(pattern, count)] and used [last_n] (the samples at the mode)"""
    Aw = np.asarray(Aw, dtype=np.float64)
    keys = ["".join("1" if v != 0.0 else "0" for v in a) for a in Aw]
    tab = sorted(Counter(keys).items(), key=lambda kv: (-kv[1], kv[0]))
    return tab, np.array([k == tab[0][0] for k in keys])


def type7(nu, p):
    """h = (nu - 1) p, j = floor(h), g = h - j"""
    h = (nu - 1) * p
    j = int(np.floor(h))
    return j, h - j


def order_stats(nu, ci):
    """jlo, glo, jhi, ghi and kt = min(nu, max(jlo + 2, nu - jhi)): the order statistics k_map_stats keeps per element and end"""
    jlo, glo = type7(nu, 0.5 - ci / 2.0)
    jhi, ghi = type7(nu, 0.5 + ci / 2.0)
    return jlo, glo, jhi, ghi, min(nu, max(jlo + 2, nu - jhi))


def interpolate(xs, j, g):
    """(1 - g) x_(j) + g x_(min(j + 1, nu - 1)) over xs sorted along axis 0: two products and one sum; where the two order statistics
    are equal, that value itself (map_interp: stats::quantile interpolates only where they differ)"""
    nu = xs.shape[0]
    a, b = xs[j], xs[min(j + 1, nu - 1)]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(a == b, a, (1.0 - g) * a + g * b)


def renormalised(P, E):
    """P [S][K][N], E [S][N][G] -> cs [S][N] (k_map_colsum), x = P / cs, e = E * cs"""
    cs = np.stack([canon64_colsum(P[s]) for s in range(P.shape[0])])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return cs, P / cs[:, None, :], E * cs[:, :, None]


def series_mean(x):
    """the sequential sum over the samples (axis 0), oldest first, from +0.0, divided by their number; an element that holds one value
    in every sample has that value as its mean"""
    acc = np.zeros(x.shape[1:])
    for s in range(x.shape[0]):
        acc = acc + x[s]
    return np.where((x == x[0]).all(axis=0), x[0], acc / float(x.shape[0]))


def fit(Pm, Am, Em, M, log=oracle_log):
    """k_map_fit and the host's totals: c = sum_n (P[k,n] * A[n]) * E[n,g], n ascending from +0.0; per column the canonical W = 64 sums
    over k of (c - m)^2 and of mt * log(mt / mh); then the sequential sums over g.  Returns rmse, kl, and the per-column sums"""
    K, N = Pm.shape
    G = Em.shape[1]
    m = np.asarray(M, dtype=np.float64)
    c = np.zeros((K, G))
    for n in range(N):
        c = c + (Pm[:, n] * Am[n])[:, None] * Em[n, :][None, :]
    d = c - m
    mt, mh = np.where(m < TINY, TINY, m), np.where(c < TINY, TINY, c)
    colsse, colkl = canon64_colsum(d * d), canon64_colsum(mt * log(mt / mh))
    return float(np.sqrt(seq_sum(colsse) / (float(K) * float(G)))), seq_sum(colkl), colsse, colkl


def map_reference(Pw, Ew, Aw, M, ci=0.95, log=oracle_log, mean=series_mean, bound=interpolate):
    """Pw [last_n][K][N], Ew [last_n][N][G], Aw [last_n][N]: EVERY sample of the range, oldest first; M the data (K x G); ci None or 0:
    no bounds.  Returns every output of bnmf_map by name (P, P_lower, P_upper K x N; E, E_lower, E_upper N x G; A [N]; used [last_n];
    top_A 5 x N, NaN rows past the number of patterns; n_used, n_patterns, top_counts[5], rmse, kl).  `mean` and `bound` are there so
    that tests/test_map_host.py can show that another expression gives other bits."""
    Pw, Ew, Aw = (np.asarray(a, dtype=np.float64) for a in (Pw, Ew, Aw))
    last_n, K, N = Pw.shape
    Aw = Aw.reshape(last_n, N)
    tab, used = mode_of_A(Aw)
    nu = int(used.sum())
    Am = np.array([1.0 if ch == "1" else 0.0 for ch in tab[0][0]])
    top_A = np.full((5, N), np.nan)
    for i, (k, _) in enumerate(tab[:5]):
        top_A[i] = [1.0 if ch == "1" else 0.0 for ch in k]
    cs, x, e = renormalised(Pw[used], Ew[used])
    out = dict(P=mean(x), E=mean(e), A=Am, used=used.astype(np.int32), top_A=top_A, n_used=nu, n_patterns=len(tab),
               top_counts=[c for _, c in tab[:5]] + [0] * (5 - min(5, len(tab))), cs=cs,
               P_lower=None, P_upper=None, E_lower=None, E_upper=None)
    if ci:
        jlo, glo, jhi, ghi, out["kt"] = order_stats(nu, ci)
        xs, es = np.sort(x, axis=0), np.sort(e, axis=0)
        out.update(P_lower=bound(xs, jlo, glo), P_upper=bound(xs, jhi, ghi), E_lower=bound(es, jlo, glo), E_upper=bound(es, jhi, ghi))
    out["rmse"], out["kl"], out["colsse"], out["colkl"] = fit(out["P"], Am, out["E"], M, log)
    return out


def quantile7(x, prob):
    """assign_impl's quantile7 of the vector x"""
    xs = np.sort(np.asarray(x, dtype=np.float64))
    j, g = type7(xs.size, prob)
    return float(interpolate(xs, j, g))


def assign_reference(Pw, ref, keep=None, MAP_P=None, ci=0.95, solver=hungarian):
    """Pw [S][K][N]: the USED samples, oldest first; ref the catalogue (K x R); keep [N] (None: every factor); MAP_P (K x N) or None.
    Returns votes (N x R), assigned [N] (int32), MAP_cosine, lower_cosine, upper_cosine [N] (NaN where the device leaves NaN), and
    cosines [S][nk][R], cols [S][min(nk, R)]: what k_ref_cosine and k_hungarian leave.  Raises where the device refuses (a sample with a
    cosine that is not finite)."""
    Pw, ref = np.asarray(Pw, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    S, K, N = Pw.shape
    R = ref.shape[1]
    sig = np.arange(N) if keep is None else np.where(np.asarray(keep) != 0)[0]
    nk = sig.size
    votes = np.zeros((N, R))
    out = dict(votes=votes, assigned=np.full(N, -1, dtype=np.int32), MAP_cosine=np.full(N, np.nan), lower_cosine=np.full(N, np.nan),
               upper_cosine=np.full(N, np.nan), cosines=np.zeros((S, nk, R)), cols=None)
    if S == 0 or nk == 0:
        return out
    rn2 = np.zeros(R)
    for k in range(K):
        rn2 = rn2 + ref[k] * ref[k]
    tr = nk > R                                                # more signatures than references: the references are the rows
    cols = np.empty((S, R if tr else nk), dtype=np.int32)
    for s in range(S):
        C = cosine_matrix(Pw[s][:, sig], ref)
        a = solver(C.T if tr else C)
        if a is None:
            raise ValueError(f"sample {s} has no assignment (a cosine is not finite)")
        out["cosines"][s], cols[s] = C, a
        if not tr:                                             # the votes are added in sample order
            for i in range(nk):
                votes[sig[i], a[i]] = votes[sig[i], a[i]] + C[i, a[i]]
        else:
            for j in range(R):
                votes[sig[a[j]], j] = votes[sig[a[j]], j] + C[a[j], j]
    out["cols"] = cols
    for i, n in enumerate(sig):
        best, bv = -1, 0.0
        for j in range(R):                                     # the first maximum that is > 0
            if votes[n, j] > bv:
                bv, best = votes[n, j], j
        out["assigned"][n] = best
        if best < 0:
            continue
        if MAP_P is not None:
            p, q = np.asarray(MAP_P, dtype=np.float64)[:, n], ref[:, best]
            dot = nn = 0.0
            for k in range(K):
                dot = dot + p[k] * q[k]
                nn = nn + p[k] * p[k]
            with np.errstate(divide="ignore", invalid="ignore"):
                out["MAP_cosine"][n] = dot / np.sqrt(nn * rn2[best])
        if ci is not None and 0.0 < ci < 1.0:
            xs = out["cosines"][:, i, best]
            out["lower_cosine"][n], out["upper_cosine"][n] = quantile7(xs, (1.0 - ci) / 2.0), quantile7(xs, 1.0 - (1.0 - ci) / 2.0)
    return out
