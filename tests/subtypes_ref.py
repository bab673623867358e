"""The numerical spec of bnmf_subtypes (include/bnmf.h) restated in numpy float64, operation for operation: bnmf_contrast's
renormalised exposures, the total over the factors ascending from +0.0, the share profile, its alignment by perm, the Lloyd steps (the
squared distance summed j ascending with subtract, multiply and add rounded separately; the lowest c wins a tie; bnmf_regress's blocked
canonical sum over the positions of the member list for the centres and the inertia; an empty cluster keeps its centre; the stop rule),
and over the matched samples the membership counts, the labels, the consensus rows and bnmf_contrast's moments at the fixed interval
0.95.  Loops over the samples, the steps, the clusters and the factors in the stated order, vectorised over the tumours (an
order-preserving form: every element sees the scalar sequence of operations).  Shared by tests/test_subtypes_host.py and
tests/test_gpu_subtypes.py / tests/test_rshim_subtypes.py (the device against it, bit for bit).  Test infrastructure only."""
import numpy as np

from contrast_ref import canon64, moments
from regress_ref import BLOCK, canonB
from waic_ref import canon64_colsum

MAX_C, MAX_N, MAX_STEPS, CI = 32, 128, 1000, 0.95
assert BLOCK == 1024


class Refused(ValueError):
    """the restatement's refusals: .code is the ABI's (-1 BNMF_EINVAL, -2 BNMF_ESIZE)"""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def loads(P, E, A):
    """x [S][N][G]: bnmf_contrast's renormalised exposures"""
    P, E, A = np.asarray(P, dtype=np.float64), np.asarray(E, dtype=np.float64), np.asarray(A, dtype=np.float64)
    S = E.shape[0]
    A = A.reshape(S, -1)
    cs = np.stack([canon64_colsum(P[s]) for s in range(S)])                       # k_map_colsum
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where((A != 0)[:, :, None], E * cs[:, :, None], 0.0)


def profiles(x, perm=None):
    """one sample: x [N][m] -> q [N][m] (the aligned share profiles, +0.0 for an unassigned tumour), ok [m]"""
    N, m = x.shape
    t = np.zeros(m)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for n in range(N):
            t = t + x[n]
        ok = (t > 0) & (t < np.inf)
        u = 1.0 / np.where(ok, t, 1.0)
        r = np.where(ok[None, :], x * u[None, :], 0.0)
    q = np.zeros((N, m))
    for n in range(N):
        q[n if perm is None else int(perm[n])] = r[n]
    return q, ok


def assign(q, ok, mu):
    """labels [m] (-1 = unassigned) and dmin [m] (+0.0 for an unassigned tumour)"""
    N, m = q.shape
    C = mu.shape[1]
    label, dmin = np.zeros(m, dtype=np.int64), None
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(C):
            d = np.zeros(m)
            for j in range(N):
                df = q[j] - mu[j, c]
                d = d + df * df
            if c == 0:
                dmin = d
            else:
                win = d < dmin
                label = np.where(win, c, label)
                dmin = np.where(win, d, dmin)
    return np.where(ok, label, -1), np.where(ok, dmin, 0.0)


def update(q, label, mu):
    """the new centres and the sizes n_c: an empty cluster keeps its centre"""
    N, C = mu.shape
    new, sizes = mu.copy(), np.zeros(C, dtype=np.int64)
    for c in range(C):
        sizes[c] = int((label == c).sum())
        if sizes[c] > 0:
            new[:, c] = canonB(np.where((label == c)[:, None], q.T, 0.0)) / float(sizes[c])
    return new, sizes


def lloyd(q, ok, centres0, n_steps):
    """one sample's steps -> label, centres, sizes, inertia, steps, changed in the last step"""
    mu = np.array(centres0, dtype=np.float64)
    label = np.full(q.shape[1], -1, dtype=np.int64)
    steps, changed = 0, False
    for _ in range(n_steps):
        new, dmin = assign(q, ok, mu)
        changed = bool((new != label).any())
        label = new
        mu, sizes = update(q, label, mu)
        steps += 1
        if not changed:
            break
    return label, mu, sizes, float(canonB(dmin)), steps, changed


def finish(members, G, labs, cens, sizes, query, min_certainty):
    """over the matched samples: labs [S'][m], cens [S'][N][C], sizes [S'][C] -> the outputs by tumour and the info fields"""
    Sm, m = labs.shape
    N, C = cens.shape[1:]
    cnt = np.stack([(labs == c).sum(axis=0) for c in range(C)])                   # [C][m]
    a = (labs >= 0).sum(axis=0)
    membership, label, tumour = np.full((C, G), np.nan), np.full(G, -1, dtype=np.int32), np.full((3, G), np.nan)
    cert = []
    least, at = np.nan, -1
    for i, g in enumerate(members):
        tumour[1, g] = float(a[i]) / float(Sm)
        if a[i] == 0:
            continue
        best = int(np.argmax(cnt[:, i]))                                           # (the first of the largest)
        rest = [c for c in range(C) if c != best]
        membership[:, g] = cnt[:, i].astype(np.float64) / float(a[i])
        label[g] = best
        tumour[0, g] = membership[best, g]
        tumour[2, g] = max(membership[c, g] for c in rest)
        cert.append(tumour[0, g])
        if at < 0 or tumour[0, g] < least:
            least, at = float(tumour[0, g]), int(g)
    Q = len(query)
    together = np.full((Q, G), np.nan)
    place = {int(g): i for i, g in enumerate(members)}
    for qi, g in enumerate(query):
        lq = labs[:, place[int(g)]]
        both = ((lq >= 0)[:, None] & (labs >= 0)).sum(axis=0)
        tog = ((lq >= 0)[:, None] & (labs == lq[:, None])).sum(axis=0)
        for i, gi in enumerate(members):
            if gi != g and both[i] > 0:
                together[qi, gi] = float(tog[i]) / float(both[i])
    centre = np.stack(moments(cens, CI))                                           # [4][N][C]
    size = np.stack(moments(sizes.astype(np.float64), CI))                         # [4][C]
    small = int(np.argmin(size[0]))
    cert = np.array(cert)
    return dict(membership=membership, label=label, tumour=tumour, centre=centre, size=size, together=together, n_included=m, n_left_out=G - m,
                n_certain=int((cert >= min_certainty).sum()), n_never_assigned=int((a == 0).sum()),
                mean_certainty=float(canon64(cert)) / float(len(cert)) if len(cert) else np.nan, least_certain=least, least_certain_at=at,
                smallest_subtype=float(size[0, small]), smallest_subtype_at=small)


def subtypes_reference(P, E, A, centres0, include=None, perm=None, n_steps=50, query=None, min_certainty=0.9):
    """P [S][K][N], E [S][N][G], A [S][N]: the USED samples, oldest first; perm [S][N] (the rows of the used samples) or None; centres0
    N x C.  Returns the outputs of bnmf_subtypes (centre as 4 x N x C, labels S x G, series 3 x S, as Engine.subtypes returns them) and
    the info fields; refuses (Refused) what the call refuses after its arguments' shapes."""
    E = np.asarray(E, dtype=np.float64)
    S, N, G = E.shape
    c0 = np.asarray(centres0, dtype=np.float64)
    C = c0.shape[1]
    inc = np.ones(G, dtype=np.int64) if include is None else np.asarray(include, dtype=np.int64)
    if ((inc != 0) & (inc != 1)).any():
        raise Refused(-1, "include is neither 0 nor 1")
    members = np.where(inc == 1)[0]
    m = len(members)
    if C < 2 or C > MAX_C:
        raise Refused(-1, f"C = {C}")
    if n_steps < 1 or n_steps > MAX_STEPS:
        raise Refused(-1, f"n_steps = {n_steps}")
    q_ = np.zeros(0, dtype=np.int64) if query is None else np.asarray(query, dtype=np.int64).reshape(-1)
    if ((q_ < 0) | (q_ >= G)).any() or (inc[q_] == 0).any():
        raise Refused(-1, "query")
    if not (np.isfinite(c0).all() and (c0 >= 0).all()):
        raise Refused(-1, "centres0")
    if not (0.0 <= min_certainty <= 1.0):
        raise Refused(-1, "min_certainty")
    matched = []
    for s in range(S):
        if perm is not None:
            row = np.asarray(perm[s])
            if (row == -1).all():
                continue
            if sorted(row.tolist()) != list(range(N)):
                raise Refused(-1, f"perm row {s}")
        matched.append(s)
    if S < 2 or len(matched) < 2 or m < C or N > MAX_N:
        raise Refused(-2, "size")
    x = loads(P, E, A)[:, :, members]
    labels, series = np.full((S, G), -2, dtype=np.int32), np.full((3, S), np.nan)
    labs, cens, sizes, n_not = [], [], [], 0
    for s in matched:
        q, ok = profiles(x[s], None if perm is None else perm[s])
        lab, mu, sz, inertia, steps, changed = lloyd(q, ok, c0, n_steps)
        labels[s, members] = lab
        series[:, s] = inertia, float(steps), float((lab >= 0).sum())
        n_not += int(steps == n_steps and changed)
        labs.append(lab); cens.append(mu); sizes.append(sz)
    out = finish(members, G, np.stack(labs), np.stack(cens), np.stack(sizes), q_, min_certainty)
    out.update(labels=labels, series=series, n_used=S, n_matched=len(matched), n_unmatched=S - len(matched), C=C, n_steps=n_steps, n_query=len(q_),
               n_not_converged=n_not, min_certainty=float(min_certainty), members=members, sample_centres=np.stack(cens), sample_sizes=np.stack(sizes))
    return out
