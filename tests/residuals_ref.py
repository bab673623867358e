"""The numerical spec of bnmf_residuals (include/bnmf.h) restated in numpy float64, operation for operation: the fit of a
cell in reconstruction_ref's expression ((P[k, n] * A[n]) * E[n], n ascending from +0.0), the 1e-6 clip and the sigmasq of bnmf_ppc, the
standardised residuals, bnmf_regress's blocked canonical sum over the positions of the member list for b and for the K x K matrix (the
product rounded, then added; k' <= k computed, then mirrored), the leading component by power iteration with every sum over k as a scalar
loop, the flat rule, the scores, and over the samples that are not flat bnmf_contrast's moments, the mean matrix, the alignment and the
info fields.  Loops in the stated order, vectorised over the tumours and, in the matrix-vector product, over the rows (every element
sees the scalar sequence of operations).  Shared by tests/test_residuals_host.py and tests/test_gpu_residuals.py /
tests/test_rshim_residuals.py (the device against it, bit for bit).  Test infrastructure only."""
import math

import numpy as np

from contrast_ref import canon64, moments
from regress_ref import BLOCK, canonB

MAX_K, MAX_STEPS = 2048, 10000
assert BLOCK == 1024


class Refused(ValueError):
    """the restatement's refusals: .code is the ABI's (-1 BNMF_EINVAL, -2 BNMF_ESIZE)"""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def residuals_z(P, E, A, Md, members, sigmasq=None):
    """one sample: P [K][N], E [N][G], A [N], Md [K][G] doubles, sigmasq [G] (Normal) or None -> z [K][m], chi [m]"""
    K, N = P.shape
    Em = E[:, members]
    m = len(members)
    z, chi = np.empty((K, m)), np.zeros(m)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(K):
            c = np.zeros(m)
            for n in range(N):
                c = c + (P[k, n] * A[n]) * Em[n]                                   # reconstruction_ref's f_n, pre_N
            M = Md[k, members]
            if sigmasq is None:
                lam = np.where(c < 1e-6, 1e-6, c)
                z[k] = (M - lam) / np.sqrt(lam)
            else:
                z[k] = (M - c) / np.sqrt(sigmasq[members])
            chi = chi + z[k] * z[k]
    return z, chi / float(K)


def second_moments(z):
    """z [K][m] -> C [K][K] (k' <= k computed, mirrored), b [K]"""
    K, m = z.shape
    C = np.empty((K, K))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            row = canonB((z[:k + 1] * z[k][None, :]).T) / float(m)
            C[k, :k + 1] = row
            C[:k + 1, k] = row
        b = canonB(z.T) / float(m)
    return C, b


def lead(C, n_steps):
    """the leading component of the symmetric C [K][K]: dict(flat, trace, lambda, share, move, v)"""
    K = C.shape[0]
    tr, best, ks = 0.0, float(C[0, 0]), 0
    for k in range(K):
        d = float(C[k, k])
        tr = tr + d
        if d > best:
            best, ks = d, k
    nanv = np.full(K, np.nan)
    flat = dict(flat=True, trace=tr, lam=np.nan, share=np.nan, move=np.nan, v=nanv)
    if not (tr > 0.0 and math.isfinite(tr)):
        return flat
    y = np.array(C[:, ks], dtype=np.float64)
    v = None
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for step in range(n_steps + 2):
            nn = 0.0
            for k in range(K):
                nn = nn + float(y[k]) * float(y[k])
            if not (nn > 0.0 and math.isfinite(nn)):
                return flat
            r = math.sqrt(nn)
            if step == n_steps + 1:
                lam, mx = 0.0, 0.0
                for k in range(K):
                    lam = lam + float(v[k]) * float(y[k])
                for k in range(K):
                    d = abs(float(y[k]) / r - float(v[k]))
                    mx = d if d > mx else mx
                break
            v = y / r
            acc = np.zeros(K)
            for j in range(K):
                acc = acc + C[:, j] * v[j]
            y = acc
    at, big = 0, abs(float(v[0]))
    for k in range(1, K):
        d = abs(float(v[k]))
        if d > big:
            big, at = d, k
    if v[at] < 0.0:
        v = -v
    return dict(flat=False, trace=tr, lam=lam, share=lam / tr, move=mx, v=v)


def scores(v, z):
    t = np.zeros(z.shape[1])
    for k in range(z.shape[0]):
        t = t + v[k] * z[k]
    return t


def finish(G, members, n_steps, max_dispersion, Cs, bs, leads, ts, chis):
    """the statistics over the samples: Cs [S][K][K], bs [S][K], leads [S] (lead's dicts), ts / chis [S][m] -> the outputs"""
    S, K = bs.shape
    m = len(members)
    live = [s for s in range(S) if not leads[s]["flat"]]
    Sp = len(live)
    if Sp < 2:
        raise Refused(-2, f"{Sp} samples that are not flat")
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        gram = canon64(Cs[live]) / float(Sp)
        top = lead(gram, n_steps)
        vbar = top["v"]
        a, sgn = np.full(S, np.nan), np.ones(S)
        amin, amin_at = np.nan, -1
        for s in live:
            d = 0.0
            for k in range(K):
                d = d + float(leads[s]["v"][k]) * float(vbar[k])
            a[s], sgn[s] = d, (-1.0 if d < 0.0 else 1.0)
            if amin_at < 0 or abs(d) < amin:
                amin, amin_at = abs(d), s
        V = np.stack([leads[s]["v"] for s in live]) * sgn[live][:, None]
        q = np.stack([np.diag(Cs[s]) for s in live])
        bl = bs[live]
        bm, bv, _, _ = moments(bl, 0.0)
        qm, qv, _, _ = moments(q, 0.0)
        vm, vv, _, _ = moments(V, 0.0)
        pb = (bl > 0).sum(axis=0) / float(Sp)
        typ = np.stack([bm, bv, pb, qm, qv])
        comp = np.stack([vbar, vm, vv, (V > 0).sum(axis=0) / float(Sp)])
        tm, tv, _, _ = moments(ts[live] * sgn[live][:, None], 0.0)
        cm = canon64(chis[live]) / float(Sp)
        tumour = np.full((3, G), np.nan)
        tumour[:, members] = np.stack([tm, tv, cm])
        series = np.full((5, S), np.nan)
        for s in live:
            series[:, s] = [leads[s]["trace"], leads[s]["lam"], leads[s]["share"], leads[s]["move"], a[s]]
        mean_share = float(canon64(series[2, live])) / float(Sp)
    worst, worst_at = np.nan, -1
    for k in range(K):
        if not np.isnan(qm[k]) and (worst_at < 0 or qm[k] > worst):
            worst, worst_at = float(qm[k]), k
    out = dict(gram=gram, type=typ, component=comp, tumour=tumour, series=series, n_used=S, n_flat=S - Sp, n_included=m, n_left_out=G - m, n_steps=n_steps,
               n_biased=int(((pb <= 0.025) | (pb >= 0.975)).sum()), n_overdispersed=int((qm > max_dispersion).sum()), worst_type_at=worst_at,
               min_agreement_at=amin_at, share=top["share"], move=top["move"], mean_share=mean_share, min_agreement=amin, worst_type=worst,
               max_dispersion=float(max_dispersion))
    out["lambda"] = top["lam"]
    return out


def residuals_reference(P, E, A, M, include=None, n_steps=100, max_dispersion=2.0, sigmasq=None):
    """P [S][K][N], E [S][N][G], A [S][N], M [K][G] (counts or real values), sigmasq [S][G] for the Normal likelihood (else None): the
    USED samples, oldest first.  Returns the outputs of bnmf_residuals and, for the tests' own bookkeeping, C (S x K x K), b (S x K),
    v (S x K), t and chi (S x m), flat (S) and members; refuses (Refused) what the call refuses after its arguments' shapes."""
    P, E, A = (np.asarray(v, dtype=np.float64) for v in (P, E, A))
    S, K, N = P.shape
    G = E.shape[2]
    A = A.reshape(S, N)
    Md = np.asarray(M, dtype=np.float64)
    inc = np.ones(G, dtype=np.int64) if include is None else np.asarray(include, dtype=np.int64)
    if ((inc != 0) & (inc != 1)).any():
        raise Refused(-1, "include is neither 0 nor 1")
    if not 1 <= n_steps <= MAX_STEPS:
        raise Refused(-1, f"n_steps = {n_steps}")
    if not max_dispersion >= 0.0:
        raise Refused(-1, "max_dispersion is NaN or negative")
    members = np.where(inc == 1)[0]
    m = members.size
    if S < 2:
        raise Refused(-2, f"{S} used samples")
    if m < 2:
        raise Refused(-2, f"{m} included tumours")
    if K > MAX_K:
        raise Refused(-2, f"K = {K}")
    Cs, bs, ts, chis, leads = np.empty((S, K, K)), np.empty((S, K)), np.empty((S, m)), np.empty((S, m)), []
    for s in range(S):
        z, chis[s] = residuals_z(P[s], E[s], A[s], Md, members, None if sigmasq is None else np.asarray(sigmasq[s], dtype=np.float64))
        Cs[s], bs[s] = second_moments(z)
        leads.append(lead(Cs[s], n_steps))
        with np.errstate(invalid="ignore", over="ignore"):
            ts[s] = scores(leads[s]["v"], z)
    out = finish(G, members, n_steps, max_dispersion, Cs, bs, leads, ts, chis)
    out.update(C=Cs, b=bs, v=np.stack([ld["v"] for ld in leads]), t=ts, chi=chis, flat=np.array([ld["flat"] for ld in leads]), members=members)
    return out
