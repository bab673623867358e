"""Time of bnmf_contrast (group contrasts of exposures over the recorded window on the device, csrc/contrast.h) at a given shape and window.

    python tools/contrast_time.py --K 96 --G 10000 --N 20 --window 1000 [--calls 9] [--host] [--form 0|1]

Creates a Poisson-Gamma chain, runs it until the window is full, and times Engine.contrast(window, groups) over all samples of the window
for two group layouts — "balanced": two groups of G / 2, alternating tumours; "unbalanced": 90 % of the tumours against 7 %, 3 % left
out (9,000 against 700 with 300 left out at G = 10,000), in contiguous blocks: wall time around the call, which returns after its own
stream synchronisation with the results on the host; one untimed call first, then the median, minimum and maximum of --calls calls.
Prints one JSON line: the times, the ring bytes the call reads (the grouped columns of E and, for the column sums, P: S (N Gin + K N + N) 8),
the rate that is, and its fraction of the device's measured copy bandwidth (bnmf_ubench: a device-to-device copy, read + write counted).
--host also evaluates the same formulas with numpy on the host over the whole window (copied out with bnmf_window; sums in numpy's own
order), the copy and the compute timed apart, and reports the largest relative difference of the group means of the load to the
device's.  --form 1 forces the tiled form of the kernel (BNMF_CON_FORM).  The host is the yardstick, not the code under test.  Not a test."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def layouts(G):
    import numpy as np
    bal = (np.arange(G) % 2).astype(np.int32)
    unb = np.full(G, -1, dtype=np.int32)
    n0, n1 = (G * 90) // 100, (G * 7) // 100
    unb[:n0] = 0
    unb[n0:n0 + n1] = 1
    return dict(balanced=bal, unbalanced=unb)


def host_contrast(e, S, groups, min_load):
    """the window copied to the host and the spec's formulas in numpy float64; returns (seconds: copy, compute; the mean load N x C)"""
    import numpy as np
    t0 = time.perf_counter()
    P, E, A = np.stack(e.window("P", S)), np.stack(e.window("E", S)), np.stack(e.window("A", S)).reshape(S, -1)
    t1 = time.perf_counter()
    Cn = int(groups.max()) + 1
    cs = P.sum(axis=1)                                                             # S x N
    x = np.where((A != 0)[:, :, None], E * cs[:, :, None], 0.0)
    t = x.sum(axis=1)
    with np.errstate(divide="ignore"):
        r = x * np.where(t > 0, 1.0 / t, 0.0)[:, None, :]
    b = x >= min_load
    v = np.stack([np.stack([a[:, :, groups == c].mean(axis=2) for c in range(Cn)], axis=2) for a in (x, r, b)])   # 3 x S x N x C
    mean = v.mean(axis=1)
    var = v.var(axis=1, ddof=1)
    d = v[:, :, :, 0] - v[:, :, :, 1] if Cn > 1 else v[:, :, :, 0]
    q = np.quantile(d, [0.025, 0.975], axis=1)
    pg = (d > 0).mean(axis=1)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, mean[0], (var, q, pg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=96)
    ap.add_argument("--G", type=int, default=10000)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--form", type=int, choices=[0, 1], default=None)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.form is not None:
        os.environ["BNMF_CON_FORM"] = str(a.form)
    import numpy as np
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import ubench
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    K, G, N, S = a.K, a.G, a.N, a.window
    M, _, _ = synth_counts(K, G, min(5, N), 20251016)
    e = Engine(M, N, likelihood="poisson", prior="gamma", seed=3, window=S, device=a.device)
    apply_hyperprior_params(e, "gamma", M, N)
    e.init()
    t0 = time.perf_counter()
    e.run(S, metrics=False)
    fill_s = time.perf_counter() - t0
    _, copy_gbs = ubench(a.device)
    out = dict(K=K, G=G, N=N, window=S, calls=a.calls, form=a.form, fill_s=fill_s, copy_GBps=copy_gbs)
    for tag, groups in layouts(G).items():
        nbytes = S * (N * int((groups >= 0).sum()) + K * N + N) * 8
        first = e.contrast(S, groups)                            # untimed: grows the scratch, loads the kernel
        times = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            w = e.contrast(S, groups)
            times.append(time.perf_counter() - t0)
        assert np.array_equal(w["group"], first["group"], equal_nan=True) and np.array_equal(w["pair"], first["pair"], equal_nan=True)
        med = statistics.median(times)
        out.update({f"{tag}_sizes": w["sizes"].tolist(), f"{tag}_left_out": w["n_left_out"], f"{tag}_ring_bytes": nbytes, f"{tag}_ms_median": 1e3 * med,
                    f"{tag}_ms_min": 1e3 * min(times), f"{tag}_ms_max": 1e3 * max(times), f"{tag}_ring_GBps": nbytes / med / 1e9,
                    f"{tag}_fraction_of_copy_bandwidth": nbytes / med / 1e9 / copy_gbs, f"{tag}_n_credible": w["n_credible"]})
        if a.host:
            tc, tn, mu, _ = host_contrast(e, S, groups, 1.0)
            dev = w["group"][0, 0]
            out.update({f"{tag}_host_copy_s": tc, f"{tag}_host_numpy_s": tn,
                        f"{tag}_host_max_rel_diff": float(np.max(np.abs(mu - dev) / np.maximum(np.abs(dev), 1e-300)))})
    if a.host:
        out["host_threads"] = os.environ.get("OMP_NUM_THREADS")
    e.close()
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
