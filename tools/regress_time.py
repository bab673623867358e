"""Time of bnmf_regress (regression of exposures on tumour covariates over the recorded window on the device, csrc/regress.h) at a given
shape and window.

    python tools/regress_time.py --K 96 --G 10000 --N 20 --window 1000 [--calls 9] [--host] [--form 0|1]

Creates a Poisson-Gamma chain, runs it until the window is full, and times Engine.regress(window, design) over all samples of the window
for two designs — "q3": an intercept, a continuous covariate (an age in whole years) and a 0 / 1 covariate; "q16": the same and 13
standard normal columns — with 3 % of the tumours left out: wall time around the call, which returns after its own stream
synchronisation with the results on the host; one untimed call first, then the median, minimum and maximum of --calls calls.
Prints one JSON line: the times, the ring bytes the call needs (the included columns of E and, for the column sums, P and A: S (N m + K N
+ N) 8; the two passes each read them), the rate that is, and its fraction of the device's measured copy bandwidth (bnmf_ubench: a
device-to-device copy, read + write counted).
--host also times the host's route: the window copied out with bnmf_window (timed as it is), then the three responses and
numpy.linalg.lstsq over the first --host-samples samples (default 8), that time scaled by window / host-samples (least squares per
sample is independent work: the scaling is linear), and reports the largest relative difference of the mean coefficients of the load
over those samples to the device's.  --form 1 forces the narrow tiles of the kernels (BNMF_REG_FORM).  The host is the yardstick, not
the code under test.  Not a test."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def designs(G):
    import numpy as np
    rng = np.random.default_rng(7)
    cols = [np.ones(G), np.round(60.0 + 12.0 * rng.standard_normal(G)), (rng.uniform(size=G) < 0.4).astype(np.float64)]
    cols += [rng.standard_normal(G) for _ in range(13)]
    D = np.asfortranarray(np.stack(cols, axis=1))
    inc = np.ones(G, dtype=np.int32)
    inc[::33] = 0
    return dict(q3=np.asfortranarray(D[:, :3]), q16=D), inc


def host_regress(e, S, n_fit, D, inc):
    """the window copied to the host, then the spec's responses and lstsq over the first n_fit samples; returns (seconds: copy, fit of
    n_fit samples; the load's coefficients n_fit x N x Q)"""
    import numpy as np
    t0 = time.perf_counter()
    P, E, A = np.stack(e.window("P", S)), np.stack(e.window("E", S)), np.stack(e.window("A", S)).reshape(S, -1)
    t1 = time.perf_counter()
    keep = inc == 1
    Dm = D[keep]
    out = []
    for s in range(n_fit):
        x = np.where((A[s] != 0)[:, None], E[s][:, keep] * P[s].sum(axis=0)[:, None], 0.0)      # N x m
        t = x.sum(axis=0)
        with np.errstate(divide="ignore"):
            Y = np.concatenate([x, x * np.where(t > 0, 1.0 / t, 0.0), np.sqrt(x)]).T             # m x 3 N
        beta, res, _, _ = np.linalg.lstsq(Dm, Y, rcond=None)
        yh = Dm @ beta
        _ = 1.0 - ((Y - yh) ** 2).sum(axis=0) / ((Y - Y.mean(axis=0)) ** 2).sum(axis=0)
        out.append(beta[:, :x.shape[0]].T)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=96)
    ap.add_argument("--G", type=int, default=10000)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-samples", type=int, default=8)
    ap.add_argument("--form", type=int, choices=[0, 1], default=None)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.form is not None:
        os.environ["BNMF_REG_FORM"] = str(a.form)
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
    ds, inc = designs(G)
    m = int(inc.sum())
    nbytes = S * (N * m + K * N + N) * 8
    out.update(n_included=m, ring_bytes=nbytes)
    for tag, D in ds.items():
        first = e.regress(S, D, include=inc)                     # untimed: grows the scratch, loads the kernels
        times = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            w = e.regress(S, D, include=inc)
            times.append(time.perf_counter() - t0)
        assert np.array_equal(w["coef"], first["coef"], equal_nan=True) and np.array_equal(w["fit"], first["fit"], equal_nan=True)
        med = statistics.median(times)
        out.update({f"{tag}_Q": w["Q"], f"{tag}_n_blocks": w["n_blocks"], f"{tag}_min_pivot_ratio": w["min_pivot_ratio"], f"{tag}_ms_median": 1e3 * med,
                    f"{tag}_ms_min": 1e3 * min(times), f"{tag}_ms_max": 1e3 * max(times), f"{tag}_ring_GBps": nbytes / med / 1e9,
                    f"{tag}_fraction_of_copy_bandwidth": nbytes / med / 1e9 / copy_gbs, f"{tag}_n_credible_load": w["n_credible"][0].tolist()})
        if a.host:
            nf = min(a.host_samples, S)
            tc, tf, beta = host_regress(e, S, nf, D, inc)
            dev = e.regress(S, D, include=inc, series=True)["coef_series"][0, :nf]
            scale = np.maximum(np.abs(dev).max(axis=(0, 1)), 1e-300)                 # per column: a coefficient near 0 is compared to its column's size
            out.update({f"{tag}_host_copy_s": tc, f"{tag}_host_lstsq_s_for_samples": tf, f"{tag}_host_samples": nf, f"{tag}_host_lstsq_s_scaled": tf * S / nf,
                        f"{tag}_host_max_rel_diff": float(np.max(np.abs(beta - dev) / scale))})
    if a.host:
        out["host_threads"] = os.environ.get("OMP_NUM_THREADS")
    e.close()
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
