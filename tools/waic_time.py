"""Time of bnmf_waic (WAIC of the recorded window on the device, csrc/waic.h) at a given shape and window.

    python tools/waic_time.py --K 96 --G 10000 --N 20 --window 1000 [--calls 9] [--host] [--likelihood poisson|normal]

Creates a Poisson-Gamma (or Normal-Exponential) chain, runs it until the window is full, and times Engine.waic(window,
pointwise=False) over all samples of the window: wall time around the call, which returns after its own stream synchronisation with
the totals on the host; one untimed call first, then the median (and minimum) of --calls calls.  Prints one JSON line: the time, the
ring bytes the kernel reads (S (N G + K N + N) 8, plus S G 8 of sigmasq for Normal), the rate that is, and its fraction of the device's
measured copy bandwidth (bnmf_ubench: a device-to-device copy, read + write counted).  --host also evaluates the same window with
numpy on the host (window copied out with bnmf_window, then the same streaming formulas, vectorised over the cells), timed once, and
reports the largest difference of the totals.  Not a test."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_waic(e, M, S, normal):
    """the window copied to the host and the spec's formulas in numpy float64; returns (seconds: copy, compute; totals)"""
    import math
    import numpy as np
    t0 = time.perf_counter()
    P, E, A = e.window("P", S), e.window("E", S), e.window("A", S)
    sig = e.window("sigmasq", S) if normal else None
    t1 = time.perf_counter()
    K, G = M.shape
    Mt = np.asarray(M, dtype=np.float64)
    lgf = None if normal else np.array([math.lgamma(m + 1.0) for m in range(int(M.max()) + 1)])[np.asarray(M, dtype=np.int64)]
    a = np.full((K, G), -np.inf)
    r, mu, m2 = np.zeros((K, G)), np.zeros((K, G)), np.zeros((K, G))
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(S):
            c = (P[s] * A[s].ravel()[None, :]) @ E[s]
            if normal:
                sd = np.sqrt(sig[s].ravel())[None, :]
                z = (Mt - c) / sd
                l = (-0.91893853320467274178 - np.log(sd)) - 0.5 * (z * z)
            else:
                mh = np.maximum(c, 1e-6)
                l = (Mt * np.log(mh) - mh) - lgf
            up = l > a
            ex = np.exp(np.where(up, a - l, l - a))
            r = np.where(up, r * ex + 1.0, r + ex)
            a = np.where(up, l, a)
            d = l - mu
            mu = mu + d * (1.0 / (s + 1))
            m2 = m2 + d * (l - mu)
    lppd, p = a + np.log(r / S), m2 / (S - 1)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, dict(lppd=float(lppd.sum()), p_waic=float(p.sum()), mean_loglik=float(mu.sum()))


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
    from bayesnmf_amd.engine import ubench
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
    first = e.waic(S)                                            # untimed: grows the scratch, loads the kernel
    times = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        w = e.waic(S)
        times.append(time.perf_counter() - t0)
    assert all(w[k] == first[k] for k in w)
    _, copy_gbs = ubench(a.device)
    nbytes = S * (N * G + K * N + N + (G if normal else 0)) * 8
    med = statistics.median(times)
    out = dict(K=K, G=G, N=N, window=S, likelihood=a.likelihood, calls=a.calls, fill_s=fill_s, waic_ms_median=1e3 * med, waic_ms_min=1e3 * min(times),
               ring_bytes=nbytes, ring_GBps=nbytes / med / 1e9, copy_GBps=copy_gbs, fraction_of_copy_bandwidth=nbytes / med / 1e9 / copy_gbs,
               cell_samples_per_s=S * K * G / med, elpd_waic=w["elpd_waic"], p_waic=w["p_waic"], se_elpd=w["se_elpd"], n_high_var=w["n_high_var"])
    if a.host:
        tc, tn, tot = host_waic(e, M, S, normal)
        out.update(host_copy_s=tc, host_numpy_s=tn, host_threads=os.environ.get("OMP_NUM_THREADS"),
                   host_max_rel_diff=max(abs(tot[k] - w[k]) / abs(w[k]) for k in tot))
    e.close()
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
