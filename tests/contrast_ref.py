"""DESIGN.md 19 restated in numpy float64, operation for operation: the group contrasts of exposures over a recorded range
(bnmf_contrast).  Only + - * /, comparisons and integer counts, every sum in the order the spec fixes, so the device is held to this bit
for bit.  Test infrastructure only."""
import numpy as np

from map_ref import interpolate, type7
from waic_ref import canon64_colsum

STATS = ("load", "share", "prevalence")


def canon64(v):
    """the canonical W = 64 sum along axis 0"""
    v = np.asarray(v, dtype=np.float64)
    return canon64_colsum(v.reshape(v.shape[0], -1)).reshape(v.shape[1:])


def per_tumour(P, E, A, min_load):
    """steps 1 - 3.  P [S][K][N], E [S][N][G], A [S][N] -> x, r (float64 [S][N][G]), b (bool), t [S][G]"""
    P, E, A = np.asarray(P, dtype=np.float64), np.asarray(E, dtype=np.float64), np.asarray(A, dtype=np.float64)
    S, N, G = E.shape
    cs = np.stack([canon64_colsum(P[s]) for s in range(S)])                       # k_map_colsum
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.where((A != 0)[:, :, None], E * cs[:, :, None], 0.0)
    t = np.zeros((S, G))
    for n in range(N):
        t = t + x[:, n, :]
    with np.errstate(divide="ignore"):
        u = np.where(t > 0, 1.0 / np.where(t > 0, t, 1.0), 0.0)
    r = x * u[:, None, :]
    return x, r, x >= min_load, t


def moments(v, ci):
    """step 5 over axis 0 of v [S][...]: mean, var, lower, upper"""
    S = v.shape[0]
    mean = canon64(v) / float(S)
    var = canon64((v - mean) * (v - mean)) / float(S - 1)
    if not ci > 0:
        return mean, var, np.full(mean.shape, np.nan), np.full(mean.shape, np.nan)
    xs = np.sort(v, axis=0)
    return mean, var, interpolate(xs, *type7(S, (1.0 - ci) / 2.0)), interpolate(xs, *type7(S, (1.0 + ci) / 2.0))


def contrast_reference(P, E, A, groups, min_load=1.0, credible_interval=0.95):
    """P [S][K][N], E [S][N][G], A [S][N]: the USED samples, oldest first; groups [G]: 0 .. C-1, -1 = left out.  Returns what
    Engine.contrast returns with series=True (group 3 x 4 x N x C, pair 3 x 6 x N x NP, series 3 x S x N x C, sizes, pairs, the info
    fields) and x, r, b, t of steps 2 - 3."""
    groups = np.asarray(groups, dtype=np.int64)
    x, r, b, t = per_tumour(P, E, A, min_load)
    S, N, G = x.shape
    C = int(groups.max()) + 1
    members = [np.where(groups == c)[0] for c in range(C)]                         # ascending tumour order
    sizes = np.array([m.size for m in members], dtype=np.int32)
    series = np.zeros((3, S, N, C))
    for c, m in enumerate(members):
        dm = float(m.size)
        for s in range(S):
            series[0, s, :, c] = canon64(x[s][:, m].T) / dm
            series[1, s, :, c] = canon64(r[s][:, m].T) / dm
            series[2, s, :, c] = b[s][:, m].sum(axis=1).astype(np.float64) / dm
    ci = float(credible_interval)
    pairs = [(a, c) for a in range(C) for c in range(a + 1, C)]
    group = np.zeros((3, 4, N, C))
    pair = np.zeros((3, 6, N, len(pairs)))
    n_credible = []
    for q in range(3):
        group[q] = np.stack(moments(series[q], ci))
        cred = 0
        for p, (a, c) in enumerate(pairs):
            d = series[q, :, :, a] - series[q, :, :, c]
            mean, var, lo, hi = moments(d, ci)
            pair[q, :, :, p] = np.stack([mean, var, lo, hi, (d > 0).sum(axis=0) / float(S), (d < 0).sum(axis=0) / float(S)])
            cred += int(((lo > 0) | (hi < 0)).sum())
        n_credible.append(cred)
    return dict(group=group, pair=pair, series=series, sizes=sizes, pairs=pairs, n_used=S, n_groups=C, n_pairs=len(pairs),
                n_left_out=int((groups < 0).sum()), n_credible=n_credible, min_load=float(min_load), credible_interval=ci, x=x, r=r, b=b, t=t)
