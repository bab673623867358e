"""The numerical spec of bnmf_prune (include/bnmf.h) restated in numpy float64, one problem (sample, tumour) at a time:
every sum is a Python loop in the stated order (the fit c_k over the places ascending, g_i over the mutation types ascending, the
cosine's sums over the mutation types ascending); numpy only carries the independent axis of such a loop elementwise, and there is no
matrix product and no numpy reduction.  k_map_colsum's canonical W = 64 column sums of P (waic_ref.canon64_colsum), Welford's update
over the samples, the canonical W = 1024 sum over the member positions for the series and the canonical W = 64 sum for the signature
rows (reconstruction_ref.canon).  Shared by tests/test_prune_host.py (the restatement on hand-built samples) and
tests/test_gpu_prune.py / tests/test_rshim_prune.py (the device against it, bit for bit).  Test infrastructure only."""
import numpy as np

from reconstruction_ref import canon
from waic_ref import canon64_colsum


def steps(x, mv, e, active, n_steps):
    """n_steps KL steps with the active flags.  x [K][Nin], mv [K], e [Nin] -> (e, d of the last step)"""
    K, Nin = x.shape
    d = 0.0
    with np.errstate(all="ignore"):
        for _ in range(n_steps):
            c = np.zeros(K)
            for i in range(Nin):                                 # c_k = sum_i x[k,i] * e_i, i ascending from +0.0
                c = c + x[:, i] * e[i]
            q = np.where(c > 0.0, mv / np.where(c > 0.0, c, 1.0), 0.0)
            g = np.zeros(Nin)
            for k in range(K):                                   # g_i = g_i + x[k,i] * q_k, k ascending from +0.0
                g = g + x[k] * q[k]
            en = np.where(active, e * g, 0.0)
            d = 0.0
            for i in range(Nin):
                v = abs(float(en[i]) - float(e[i]))
                d = v if v > d else d
            e = en
    return e, d


def cosine(x, mv, e, mm):
    K, Nin = x.shape
    with np.errstate(all="ignore"):
        c = np.zeros(K)
        for i in range(Nin):
            c = c + x[:, i] * e[i]
        dot, cc = 0.0, 0.0
        for k in range(K):
            dot = dot + float(mv[k]) * float(c[k])
            cc = cc + float(c[k]) * float(c[k])
        if not mm > 0.0:
            return float("nan")
        return float(np.float64(dot) / np.sqrt(np.float64(mm) * np.float64(cc))) if cc > 0.0 else 0.0


def prune_problem(x, mv, e0, n_steps, max_loss, order=None):
    """One problem.  x [K][Nin] the renormalised columns that take part, mv [K] the data cells as doubles, e0 [Nin] the warm start.
    Returns dict(e (Nin, by place), cos_0, cos_f, n_kept, trials, change, defined); order (a list) receives every candidate tried."""
    K, Nin = x.shape
    t, mm = 0.0, 0.0
    for k in range(K):
        t = t + float(mv[k])
        mm = mm + float(mv[k]) * float(mv[k])
    active = np.ones(Nin, dtype=bool)
    e, d = steps(x, mv, np.array(e0, dtype=np.float64), active, n_steps)
    cos0 = cosine(x, mv, e, mm)
    change = d / t if t > 0.0 else 0.0
    if not mm > 0.0:
        return dict(e=np.full(Nin, np.nan), cos_0=np.nan, cos_f=np.nan, n_kept=np.nan, trials=0, change=np.nan, defined=False)
    thr = cos0 - max_loss
    cosf, trials = cos0, 0
    while int(active.sum()) > 1:
        cand = sorted((float(e[i]), i) for i in range(Nin) if active[i])
        accepted = False
        for _, i in cand:
            te, ta = e.copy(), active.copy()
            te[i] = 0.0
            ta[i] = False
            te, d = steps(x, mv, te, ta, n_steps)
            ct = cosine(x, mv, te, mm)
            trials += 1
            if order is not None:
                order.append(i)
            if ct >= thr:
                e, active, cosf, change, accepted = te, ta, ct, (d / t if t > 0.0 else 0.0), True
                break
        if not accepted:
            break
    return dict(e=e, cos_0=cos0, cos_f=cosf, n_kept=int(active.sum()), trials=trials, change=change, defined=True)


def prune_reference(P, E, A, M, n_steps=20, max_loss=0.01, include=None):
    """P [S][K][N], E [S][N][G], A [S][N], M [K][G] counts; the used samples oldest first.  Returns the outputs of bnmf_prune: load
    (4 x N x G), tumour (7 x G), series (2 x S), signature (3 x N), exposures (S x N x G) and the info fields; and for the tests' own
    bookkeeping per-sample n_kept, trials, cos_0, cos_f (S x G, NaN where left out) and n_in (S)."""
    P, E, A = (np.asarray(v, dtype=np.float64) for v in (P, E, A))
    S, K, N = P.shape
    G = E.shape[2]
    A = A.reshape(S, N)
    Md = np.asarray(M, dtype=np.float64)
    members = [g for g in range(G) if include is None or include[g]]
    m = len(members)
    mmv = np.zeros(G)
    for k in range(K):
        mmv = mmv + Md[k] * Md[k]
    defined = [bool(mmv[g] > 0.0) for g in members]
    ndef = sum(defined)
    es = np.full((S, N, G), np.nan)
    vals = {k: np.full((S, G), np.nan) for k in ("cos_0", "cos_f", "n_kept", "trials", "change")}
    n_in = np.zeros(S, dtype=np.int64)
    with np.errstate(all="ignore"):
        for s in range(S):
            cs = canon64_colsum(P[s])
            idx = [n for n in range(N) if A[s, n] != 0.0 and cs[n] > 0.0]
            n_in[s] = len(idx)
            x = np.empty((K, len(idx)))
            for i, n in enumerate(idx):
                x[:, i] = P[s][:, n] / cs[n]
            for g in members:
                e0 = np.array([E[s, n, g] * cs[n] for n in idx], dtype=np.float64)
                r = prune_problem(x, Md[:, g], e0, n_steps, max_loss)
                if r["defined"]:
                    es[s, :, g] = 0.0
                    for i, n in enumerate(idx):
                        es[s, n, g] = r["e"][i]
                for k in vals:
                    vals[k][s, g] = r[k]
        # the statistics over the samples, member by member
        load, tumour = np.full((4, N, G), np.nan), np.full((7, G), np.nan)
        total, single, mxc = 0, 0, 0.0
        for g, df in zip(members, defined):
            if not df:
                continue
            mu, m2, sh, cnt = np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N)
            m0, mf, sk, kmin, kmax, cmax, st = 0.0, 0.0, 0.0, np.inf, 0.0, 0.0, 0.0
            for s in range(S):
                a = es[s, :, g]
                tt = 0.0
                for n in range(N):
                    tt = tt + float(a[n])
                u = 1.0 / tt if tt > 0.0 else 0.0
                rs = 1.0 / float(s + 1)
                d = a - mu
                mu = mu + d * rs
                m2 = m2 + d * (a - mu)
                sh = sh + a * u
                cnt = cnt + (a > 0.0)
                m0 = m0 + (vals["cos_0"][s, g] - m0) * rs
                mf = mf + (vals["cos_f"][s, g] - mf) * rs
                nk, ch = vals["n_kept"][s, g], vals["change"][s, g]
                sk = sk + nk
                kmin = nk if nk < kmin else kmin
                kmax = nk if nk > kmax else kmax
                cmax = ch if ch > cmax else cmax
                st = st + vals["trials"][s, g]
            dS = float(S)
            load[:, :, g] = np.stack([mu, m2 / np.float64(S - 1), sh / dS, cnt / dS])
            tumour[:, g] = [m0, mf, sk / dS, kmin, kmax, cmax, st / dS]
            total += int(st)
            single += 1 if kmax == 1.0 else 0
            mxc = float(cmax) if cmax > mxc else mxc
        series = np.full((2, S), np.nan)
        if ndef:
            for s in range(S):
                for r, key in enumerate(("n_kept", "cos_f")):
                    v = [vals[key][s, g] if df else 0.0 for g, df in zip(members, defined)]
                    series[r, s] = canon(v, 1024) / float(ndef)
        sig = np.full((3, N), np.nan)
        dm = [g for g, df in zip(members, defined) if df]
        for n in range(N):
            sig[0, n] = float(sum(1 for g in dm if load[3, n, g] >= 0.5))
            if ndef:
                sig[1, n] = canon([load[3, n, g] for g in dm], 64) / float(ndef)
            sig[2, n] = canon([load[0, n, g] for g in dm], 64)
    return dict(load=load, tumour=tumour, series=series, signature=sig, exposures=es, n_used=S, n_included=m, n_undefined=m - ndef,
                n_single=single, n_steps=int(n_steps), trials=total, max_change=mxc, max_loss=float(max_loss), n_in=n_in, **{"s_" + k: v for k, v in vals.items()})
