"""Time of bnmf_summary (cohort summary of signatures over the recorded window on the device, csrc/summary.h) at a given shape and
window.

    python tools/summary_time.py --K 96 --G 10000 --N 20 --window 1000 [--levels 5] [--calls 9] [--host] [--chunk C] [--batch B]

Creates a Poisson-Gamma chain, runs it until the window is full, and times Engine.summary(window) over all samples of the window and all
tumours: wall time around the call, which returns after its own stream synchronisation with the results on the host (the host's reduction
over the samples included); one untimed call first, then the median, minimum and maximum of --calls synchronised calls.  Prints one JSON
line.  --host also times the host's route: the window copied out with bnmf_window (timed as it is), then per sample the loads, the shares
and their numpy.sort-based quantiles (numpy.quantile, method "linear", on the loads, the carriers' loads and the shares) over the first
--host-samples samples (default 4), that time scaled by window / host-samples (every sample is independent work: the scaling is linear),
and reports the largest difference between the host's numpy.quantile medians and the device's over those samples.  --chunk and --batch set
BNMF_SUM_CHUNK (doubles of a sorted chunk: the general form) and BNMF_SUM_BATCH (samples per batch).  The host is the yardstick, not the
code under test.  Not a test."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_summary(e, S, n_fit, probs, min_load):
    """the window copied to the host, then per sample the loads, the shares and their quantiles over the first n_fit samples; returns
    (seconds: copy, n_fit samples; the medians of all loads and of the carriers' loads, n_fit x N)"""
    import numpy as np
    t0 = time.perf_counter()
    P, E, A = np.stack(e.window("P", S)), np.stack(e.window("E", S)), np.stack(e.window("A", S)).reshape(S, -1)
    t1 = time.perf_counter()
    med_all, med_present = [], []
    for s in range(n_fit):
        x = np.where((A[s] != 0)[:, None], E[s] * P[s].sum(axis=0)[:, None], 0.0)              # N x G
        t = x.sum(axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            r = x * np.where(t > 0, 1.0 / t, 0.0)[None, :]
        qa = np.quantile(x, probs, axis=1, method="linear")                                  # L x N
        np.quantile(r, probs, axis=1, method="linear")
        qp = np.array([np.quantile(row[row >= min_load], probs, method="linear") if (row >= min_load).any() else np.full(len(probs), np.nan) for row in x]).T
        med_all.append(qa[len(probs) // 2])
        med_present.append(qp[len(probs) // 2])
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, np.stack(med_all), np.stack(med_present)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=96)
    ap.add_argument("--G", type=int, default=10000)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--levels", type=int, default=5, choices=[1, 3, 5, 7])
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-samples", type=int, default=4)
    ap.add_argument("--chunk", type=int, default=None)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    for name, v in (("BNMF_SUM_CHUNK", a.chunk), ("BNMF_SUM_BATCH", a.batch)):
        if v is not None:
            os.environ[name] = str(v)
    import numpy as np
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    K, G, N, S = a.K, a.G, a.N, a.window
    probs = {1: (0.5,), 3: (0.25, 0.5, 0.75), 5: (0.05, 0.25, 0.5, 0.75, 0.95), 7: (0.025, 0.05, 0.25, 0.5, 0.75, 0.95, 0.975)}[a.levels]   # the median is the middle level
    M, _, _ = synth_counts(K, G, min(5, N), 20251016)
    e = Engine(M, N, likelihood="poisson", prior="gamma", seed=3, window=S, device=a.device)
    apply_hyperprior_params(e, "gamma", M, N)
    e.init()
    t0 = time.perf_counter()
    e.run(S, metrics=False)
    fill_s = time.perf_counter() - t0
    out = dict(K=K, G=G, N=N, window=S, levels=len(probs), calls=a.calls, chunk=a.chunk, batch=a.batch, fill_s=fill_s)
    first = e.summary(S, probs=probs)                            # untimed: grows the scratch, loads the kernels
    times = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        w = e.summary(S, probs=probs)
        times.append(time.perf_counter() - t0)
    assert np.array_equal(w["stat"], first["stat"], equal_nan=True)
    med = statistics.median(times)
    L = len(probs)
    out.update(n_included=w["n_included"], n_blocks=w["n_blocks"], n_nonfinite=w["n_nonfinite"], ms_median=1e3 * med, ms_min=1e3 * min(times), ms_max=1e3 * max(times),
               mean_prevalence=[round(float(v), 4) for v in w["stat"][0, 0]], mean_median_present=[round(float(v), 3) for v in w["stat"][4 + L + L // 2, 0]])
    if a.host:
        nf = min(a.host_samples, S)
        tc, tf, ma, mp = host_summary(e, S, nf, probs, 1.0)
        ser = e.summary(S, probs=probs, series=True)["series"]
        d0 = np.abs(ser[4 + L // 2, :nf] - ma)
        d1 = np.abs(ser[4 + L + L // 2, :nf] - mp)
        out.update(host_copy_s=tc, host_s_for_samples=tf, host_samples=nf, host_s_scaled=tf * S / nf, host_max_diff_median_all=float(np.nanmax(d0)),
                   host_max_diff_median_present=float(np.nanmax(d1)), host_threads=os.environ.get("OMP_NUM_THREADS"))
    e.close()
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
