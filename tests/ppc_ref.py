"""The Poisson sampler of the stream spec (`rpois`) and the posterior predictive checks of bnmf_ppc
restated from the DESIGN text in Python floats (IEEE fp64, no contraction), built only from the oracle's exported pieces: the Philox
block, the u52 uniform, log / exp / lgamma, the standard normal draw and the canonical sum.  Shared by tests/test_ppc_host.py (the
restatement against the Poisson law and on planted misfits) and tests/test_gpu_ppc.py / tests/test_rshim_ppc.py (the device against
it, bit for bit).  Test infrastructure only."""
import ctypes as C
import math

import numpy as np

V_YREP = 19                 # BNMF_V_YREP
MAX_ATTEMPTS = 2000
RPOIS_CAP = 128.0
ROW_CHUNK = 128

_O = {}


def _orc():
    if not _O:
        import oracle
        L = oracle.lib()
        _O.update(oracle=oracle, L=L, c=(C.c_uint32 * 4)(), k=(C.c_uint32 * 2)(), o=(C.c_uint32 * 4)(),
                  u52=L.orc_t_u52, log=L.orc_t_log, exp=L.orc_t_exp, lgamma=L.orc_t_lgamma)
    return _O


def key(seed, chain):
    """the Philox key of a chain: (seed_lo, seed_hi ^ chain_id)"""
    return int(seed) & 0xFFFFFFFF, ((int(seed) >> 32) ^ int(chain)) & 0xFFFFFFFF


def stream(seed, chain, var, elem, it):
    """the (u52(w.x, w.y), u52(w.z, w.w)) of blocks 0, 1, ... of the stream (variable, element, iteration): one pair per attempt"""
    o = _orc()
    c, k, w = o["c"], o["k"], o["o"]
    k[0], k[1] = key(seed, chain)
    blk = 0
    while True:
        c[0], c[1], c[2], c[3] = blk, elem & 0xFFFFFFFF, it & 0xFFFFFFFF, var
        o["L"].orc_t_philox(c, k, w)
        yield o["u52"](w[0], w[1]), o["u52"](w[2], w[3])
        blk += 1


def rpois_from(uniforms, lam):
    """DESIGN.md 4, rpois: (draw as a float holding a whole number, attempts used); `uniforms` yields one (u1, u2) per attempt"""
    o = _orc()
    lam = float(lam)
    if lam < 10.0:
        u, _ = next(uniforms)
        p = o["exp"](-lam)
        F = p
        x = 0.0
        while u > F and x < RPOIS_CAP:
            x = x + 1.0
            p = (p * lam) / x
            F = F + p
        return x, 1
    sl = math.sqrt(lam)
    ll = o["log"](lam)
    b = 0.931 + 2.53 * sl
    a = -0.059 + 0.02483 * b
    lia = o["log"](1.1239 + 1.1328 / (b - 3.4))
    vr = 0.9277 - 3.6224 / (b - 2.0)
    for it in range(MAX_ATTEMPTS):
        u1, V = next(uniforms)
        U = u1 - 0.5
        us = 0.5 - abs(U)
        k = float(math.floor((((2.0 * a) / us + b) * U + lam) + 0.43))
        if us >= 0.07 and V <= vr:
            return k, it + 1
        if k < 0.0 or (us < 0.013 and V > us):
            continue
        if (o["log"](V) + lia) - o["log"](a / (us * us) + b) <= (k * ll - lam) - o["lgamma"](k + 1.0):
            return k, it + 1
    return float(math.floor(lam)), MAX_ATTEMPTS


def rpois(lam, seed=1, chain=0, var=V_YREP, elem=0, it=1):
    return rpois_from(stream(seed, chain, var, elem, it), lam)


def rpois_vec(lam, seed=1, chain=0, var=V_YREP, elem0=0, it=1):
    """element elem0 + i draws rpois(lam[i]): what probe 8 of bnmf_test_sampler computes.  Returns (draws, attempts)."""
    lam = np.asarray(lam, dtype=np.float64).ravel()
    out, att = np.empty(lam.size), np.empty(lam.size, dtype=np.int64)
    for i, l in enumerate(lam):
        out[i], att[i] = rpois(l, seed, chain, var, elem0 + i, it)
    return out, att


def _chunked_colsum(x):
    """the sum over the rows of x (K x G) of DESIGN.md 14: rows in chunks of 128, the canonical W = 64 sum inside a chunk, the first
    chunk's value then + the next chunk's, ascending"""
    canon = _orc()["oracle"].canon_sum
    K, G = x.shape
    out = np.empty(G)
    for g in range(G):
        t = None
        for k0 in range(0, K, ROW_CHUNK):
            r = canon(np.ascontiguousarray(x[k0:k0 + ROW_CHUNK, g]), 64)
            t = r if t is None else t + r
        out[g] = t
    return out


def ppc_reference(P, E, A, sigmasq, M, likelihood, iters, seed, chain=0):
    """P [S][K][N], E [S][N][G], A [S][N], sigmasq [S][G] (normal; else None), M [K][G]; samples oldest first, iters[s] the iteration
    number of sample s.  Returns the outputs of bnmf_ppc: cell matrices (K x G), col (6 x G), series (4 x S) and the info fields; and
    `attempts` (K x G x S) and `lam` (the Poisson means drawn from), for the tests' own bookkeeping."""
    o = _orc()
    P, E, A = (np.asarray(x, dtype=np.float64) for x in (P, E, A))
    S, K, N = P.shape
    G = E.shape[2]
    A = A.reshape(S, N)
    normal = likelihood == "normal"
    Md = np.asarray(M, dtype=np.float64)
    mu, m2 = np.zeros((K, G)), np.zeros((K, G))
    nl, ne = np.zeros((K, G), dtype=np.int64), np.zeros((K, G), dtype=np.int64)
    T = np.zeros((4, S, G))
    att = np.ones((K, G, S), dtype=np.int64)
    lams = np.zeros((K, G, S))
    for s in range(S):
        it = int(iters[s])
        c = np.zeros((K, G))
        for n in range(N):                                   # n ascending from +0.0, (P * A) * E
            c = c + (P[s, :, n] * A[s, n])[:, None] * E[s, n, :][None, :]
        if normal:
            sd = np.sqrt(np.asarray(sigmasq, dtype=np.float64)[s])[None, :]
            z = o["oracle"].rnorm(K * G, seed=seed, chain=chain, var=V_YREP, elem0=0, it=it).reshape((K, G), order="F")
            y = c + sd * z
            zo, zr = (Md - c) / sd, (y - c) / sd
            T[0, s], T[1, s] = _chunked_colsum(zo * zo), _chunked_colsum(zr * zr)
            for q, v in ((2, np.abs(zo)), (3, np.abs(zr))):
                for g in range(G):
                    t = 0.0
                    for k in range(K):
                        t = v[k, g] if v[k, g] > t else t
                    T[q, s, g] = t
        else:
            lam = np.where(c < 1e-6, 1e-6, c)
            y = np.empty((K, G))
            for g in range(G):
                for k in range(K):
                    y[k, g], att[k, g, s] = rpois(lam[k, g], seed, chain, V_YREP, k + K * g, it)
            lams[:, :, s] = lam
            sl = np.sqrt(lam)
            d0, d1 = np.sqrt(Md) - sl, np.sqrt(y) - sl
            T[0, s], T[1, s] = _chunked_colsum(d0 * d0), _chunked_colsum(d1 * d1)
            T[2, s], T[3, s] = _chunked_colsum((Md == 0.0).astype(np.float64)), _chunked_colsum((y == 0.0).astype(np.float64))
        nl += y < Md
        ne += y == Md
        d = y - mu
        mu = mu + d * (1.0 / float(s + 1))
        m2 = m2 + d * (y - mu)
    dS = float(S)
    var = m2 / float(S - 1)
    pl, pe = nl.astype(np.float64) / dS, ne.astype(np.float64) / dS
    pit = pl + 0.5 * pe
    col = np.empty((6, G))
    for t in range(2):
        for g in range(G):
            so = sr = 0.0
            n = 0
            for s in range(S):
                so = so + float(T[2 * t, s, g])
                sr = sr + float(T[2 * t + 1, s, g])
                n += T[2 * t + 1, s, g] >= T[2 * t, s, g]
            col[3 * t, g], col[3 * t + 1, g], col[3 * t + 2, g] = so / dS, sr / dS, float(n) / dS
    series = np.empty((4, S))
    for q in range(4):
        for s in range(S):
            series[q, s] = T[q, s].max() if (normal and q >= 2) else o["oracle"].canon_sum(np.ascontiguousarray(T[q, s]), 1024)
    tot = [0.0] * 4
    for s in range(S):
        for q in range(4):
            tot[q] = tot[q] + float(series[q, s])
    return dict(mean_cell=mu, var_cell=var, p_less_cell=pl, p_equal_cell=pe, pit=pit, col=col, series=series, T=T,
                n_used=S, n_tail_cells=int(((pit < 0.025) | (pit > 0.975)).sum()),
                p_T1=float((series[1] >= series[0]).sum()) / dS, p_T2=float((series[3] >= series[2]).sum()) / dS,
                mean_T1_obs=tot[0] / dS, mean_T1_rep=tot[1] / dS, mean_T2_obs=tot[2] / dS, mean_T2_rep=tot[3] / dS,
                attempts=att, lam=lams)
