"""Time of bnmf_attribution (signature attribution of the recorded window on the device, csrc/attribution.h) at a given shape and window.

    python tools/attribution_time.py --K 96 --G 10000 --N 20 --window 1000 [--calls 9] [--host] [--host-samples 50] [--likelihood poisson|normal]

Creates a Poisson-Gamma (or Normal-Exponential) chain, runs it until the window is full, and times Engine.attribution(window) over all
samples of the window, once with load + series only and once with prob: wall time around the call, which returns after its own stream
synchronisation with the results on the host; one untimed call first, then the median, minimum and maximum of --calls calls.  Prints
one JSON line: the times, the ring bytes the kernel reads (S (N G + K N + N) 8), the rate that is, and its fraction of the device's
measured copy bandwidth (bnmf_ubench: a device-to-device copy, read + write counted).  --host also evaluates the spec with numpy on
the host (window copied out with bnmf_window, then the same formulas vectorised over the cells; sums in numpy's own order), the copy
and the compute timed apart; the compute runs over the first --host-samples samples of the window and is scaled to the whole window
(it is linear in the samples), and the largest relative difference of the mean loads over those samples' own device call is reported.
The host is the yardstick, not the code under test.  Not a test."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_attribution(e, M, S, H, normal):
    """the window copied to the host and the spec's formulas in numpy float64 over its first H samples; returns (seconds: copy,
    compute; the mean loads N x G)"""
    import numpy as np
    t0 = time.perf_counter()
    P, E, A = e.window("P", S), e.window("E", S), e.window("A", S)
    t1 = time.perf_counter()
    Mt = np.asarray(M, dtype=np.float64)
    mu = None
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(H):
            f = (P[s] * A[s].ravel()[None, :])[:, :, None] * E[s][None, :, :]          # K x N x G
            c = f.sum(axis=1)
            q = np.where(c > 0.0, 1.0 / c, 0.0)
            x = f if normal else f * (Mt * q)[:, None, :]
            a = x.sum(axis=0)
            mu = a if mu is None else mu + (a - mu) * (1.0 / (s + 1))
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, mu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=96)
    ap.add_argument("--G", type=int, default=10000)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--likelihood", choices=["poisson", "normal"], default="poisson")
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-samples", type=int, default=50)
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
    nbytes = S * (N * G + K * N + N) * 8
    _, copy_gbs = ubench(a.device)
    out = dict(K=K, G=G, N=N, window=S, likelihood=a.likelihood, calls=a.calls, fill_s=fill_s, ring_bytes=nbytes, copy_GBps=copy_gbs)
    for tag, prob in (("load", False), ("prob", True)):
        first = e.attribution(S, prob=prob)                      # untimed: grows the scratch, loads the kernel
        times = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            w = e.attribution(S, prob=prob)
            times.append(time.perf_counter() - t0)
        assert w["total"] == first["total"] and np.array_equal(w["load"], first["load"])
        med = statistics.median(times)
        out.update({f"{tag}_ms_median": 1e3 * med, f"{tag}_ms_min": 1e3 * min(times), f"{tag}_ms_max": 1e3 * max(times),
                    f"{tag}_ring_GBps": nbytes / med / 1e9, f"{tag}_fraction_of_copy_bandwidth": nbytes / med / 1e9 / copy_gbs,
                    f"{tag}_factor_cell_samples_per_s": S * K * N * G / med})
    out.update(total=w["total"], sum_of_data=float(np.sum(M)), n_present=w["n_present"])
    if a.host:
        H = max(2, min(a.host_samples, S))
        tc, tn, mu = host_attribution(e, M, S, H, normal)
        dev = e.attribution(H, end_iter=e.iter - S + H)["load_mean"]
        out.update(host_copy_s=tc, host_samples=H, host_numpy_s_measured=tn, host_numpy_s_scaled_to_window=tn * S / H,
                   host_threads=os.environ.get("OMP_NUM_THREADS"), host_max_rel_diff=float(np.max(np.abs(mu - dev) / np.maximum(np.abs(dev), 1e-300))))
    e.close()
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
