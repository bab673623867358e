"""Time of bnmf_ppc (posterior predictive checks of the recorded window on the device, csrc/ppc.h) at a given shape and window.

    python tools/ppc_time.py --K 96 --G 10000 --N 20 --window 1000 [--calls 9] [--host] [--likelihood poisson|normal]

Creates a Poisson-Gamma (or Normal-Exponential) chain, runs it until the window is full, and times Engine.ppc(window) over all
samples of the window, first with the per-column table and the series only, then with the four cell matrices as well: wall time
around the call, which returns after its own stream synchronisation with its outputs on the host; one untimed call first, then the
median, minimum and maximum of --calls calls.  Prints one JSON line: both times, the draws per second (S K G / median), the ring
bytes the kernel reads (S (N G + K N + N) 8, plus S G 8 of sigmasq for Normal) and, for Poisson, the share of the sampler's attempts
that were rejected, estimated on the host from the cell means of the last sample: cells below 10 take one attempt, the others
alpha(lam) = 1.1239 + 1.1328 / (b - 3.4) on average, b = 0.931 + 2.53 sqrt(lam).  --host also does the same work once
with numpy on the host: the window copied out with bnmf_window, c_s by a matrix product, np.random.poisson (or normal), the same
statistics; copy and compute timed apart.  Not a test."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_ppc(e, M, S, normal):
    """the window copied to the host and the same statistics in numpy float64; returns (seconds: copy, compute; the info fields)"""
    import numpy as np
    t0 = time.perf_counter()
    P, E, A = e.window("P", S), e.window("E", S), e.window("A", S)
    sig = e.window("sigmasq", S) if normal else None
    t1 = time.perf_counter()
    rng = np.random.default_rng(1)
    K, G = M.shape
    Mt = np.asarray(M, dtype=np.float64)
    mu, m2, nl, ne = np.zeros((K, G)), np.zeros((K, G)), np.zeros((K, G)), np.zeros((K, G))
    T = np.empty((4, S, G))
    for s in range(S):
        c = (P[s] * A[s].ravel()[None, :]) @ E[s]
        if normal:
            sd = np.sqrt(sig[s].ravel())[None, :]
            y = c + sd * rng.standard_normal((K, G))
            zo, zr = (Mt - c) / sd, (y - c) / sd
            T[0, s], T[1, s], T[2, s], T[3, s] = (zo * zo).sum(0), (zr * zr).sum(0), np.abs(zo).max(0), np.abs(zr).max(0)
        else:
            lam = np.maximum(c, 1e-6)
            y = rng.poisson(lam).astype(np.float64)
            sl = np.sqrt(lam)
            T[0, s], T[1, s] = ((np.sqrt(Mt) - sl) ** 2).sum(0), ((np.sqrt(y) - sl) ** 2).sum(0)
            T[2, s], T[3, s] = (Mt == 0).sum(0), (y == 0).sum(0)
        nl += y < Mt
        ne += y == Mt
        d = y - mu
        mu = mu + d * (1.0 / (s + 1))
        m2 = m2 + d * (y - mu)
    pit = nl / S + 0.5 * ne / S
    ser = np.stack([T[0].sum(1), T[1].sum(1), T[2].max(1) if normal else T[2].sum(1), T[3].max(1) if normal else T[3].sum(1)])
    col = np.stack([T[0].mean(0), T[1].mean(0), (T[1] >= T[0]).mean(0), T[2].mean(0), T[3].mean(0), (T[3] >= T[2]).mean(0)])
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, dict(p_T1=float((ser[1] >= ser[0]).mean()), p_T2=float((ser[3] >= ser[2]).mean()), mean_T1_obs=float(ser[0].mean()),
                                  mean_T1_rep=float(ser[1].mean()), n_tail_cells=int(((pit < 0.025) | (pit > 0.975)).sum()), col_rows=col.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=96)
    ap.add_argument("--G", type=int, default=10000)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--likelihood", choices=["poisson", "normal"], default="poisson")
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import numpy as np
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    K, G, N, S = a.K, a.G, a.N, a.window
    normal = a.likelihood == "normal"
    M, _, _ = synth_counts(K, G, min(5, N), 20251016)
    prior = "exponential" if normal else "gamma"
    if normal:
        M = np.asfortranarray(M + np.random.default_rng(1).normal(0.0, 0.5, size=M.shape))
    e = Engine(M, N, likelihood=a.likelihood, prior=prior, seed=3, window=S, device=a.device)
    apply_hyperprior_params(e, prior, M, N)
    e.init()
    t0 = time.perf_counter()
    e.run(S, metrics=False)
    fill_s = time.perf_counter() - t0
    out = dict(K=K, G=G, N=N, window=S, likelihood=a.likelihood, calls=a.calls, fill_s=fill_s)
    for name, pw in (("col_series", False), ("with_cell", True)):
        first = e.ppc(S, pointwise=pw)                           # untimed: grows the scratch, loads the kernels
        times = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            w = e.ppc(S, pointwise=pw)
            times.append(time.perf_counter() - t0)
        assert all(np.array_equal(w[k], first[k]) for k in w)
        med = statistics.median(times)
        out.update({f"ppc_ms_median_{name}": 1e3 * med, f"ppc_ms_min_{name}": 1e3 * min(times), f"ppc_ms_max_{name}": 1e3 * max(times)})
        if not pw:
            nbytes = S * (N * G + K * N + N + (G if normal else 0)) * 8
            out.update(draws_per_s=S * K * G / med, ring_bytes=nbytes, ring_GBps=nbytes / med / 1e9, scratch_bytes=4 * S * G * 8)
    out.update({k: w[k] for k in ("n_used", "n_tail_cells", "p_T1", "p_T2", "mean_T1_obs", "mean_T1_rep", "mean_T2_obs", "mean_T2_rep")})
    if not normal:
        lam = np.maximum((e.get("P") * e.get("A").ravel()[None, :]) @ e.get("E"), 1e-6)
        alpha = np.where(lam < 10.0, 1.0, 1.1239 + 1.1328 / np.maximum(0.931 + 2.53 * np.sqrt(lam) - 3.4, 1.0))
        out.update(cells_below_10=float((lam < 10.0).mean()), attempts_per_draw_expected=float(alpha.mean()),
                   share_of_attempts_rejected_expected=float(1.0 - alpha.size / alpha.sum()))
    if a.host:
        tc, tn, tot = host_ppc(e, M, S, normal)
        out.update(host_copy_s=tc, host_numpy_s=tn, host_threads=os.environ.get("OMP_NUM_THREADS"),
                   host_p_T1=tot["p_T1"], host_mean_T1_rep=tot["mean_T1_rep"], host_n_tail_cells=tot["n_tail_cells"])
    e.close()
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
