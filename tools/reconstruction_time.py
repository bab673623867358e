"""Time of bnmf_reconstruction (reconstruction quality per tumour over a recorded range on the device, csrc/reconstruction.h) at a given
shape and window.

    python tools/reconstruction_time.py --K 96 --G 10000 --N 20 --window 1000 [--calls 9] [--form 1] [--stage 0|1] [--batch B] [--host]

Creates a Poisson-Gamma chain, runs it until the window is full, and times Engine.reconstruction(window) over all samples of the window:
wall time around the call, which returns after its own stream synchronisation with the results on the host (the finish on the host
included); one untimed call first, then the median, minimum and maximum of --calls synchronised calls, once with all outputs and once
with `tumour` only (drop not copied out).  --form 1: the tiled form of the kernel; --stage: x in the LDS or read through the caches;
--batch: the batch of samples (all the same bits).  Prints one JSON line.  --host also times the host's route: the window copied out
with bnmf_window (timed as it is), then the same formulas in numpy (matrix products per sample for the fit and for each leave-one-out
fit) over the first --host-samples samples (default 5), that time scaled by window / host-samples (every sample is independent work: the
scaling is linear), and reports the largest difference of those samples' mean cosine per tumour from the device's over the same samples.
The host is the yardstick, not the code under test.  Not a test."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_reconstruction(e, S, n_fit, M):
    """the window copied to the host, then cos and the leave-one-out cosines of the first n_fit samples by matrix products; returns
    (seconds: copy, the samples; cos n_fit x G)"""
    import numpy as np
    t0 = time.perf_counter()
    P, E, A = np.stack(e.window("P", S)), np.stack(e.window("E", S)), np.stack(e.window("A", S)).reshape(S, -1)
    t1 = time.perf_counter()
    Md = np.asarray(M, dtype=np.float64)
    nm = np.sqrt((Md * Md).sum(axis=0))
    N = P.shape[2]
    cos = np.empty((n_fit, Md.shape[1]))
    acc = 0.0
    for s in range(n_fit):
        PA = P[s] * A[s][None, :]
        C = PA @ E[s]
        cos[s] = (Md * C).sum(axis=0) / (nm * np.sqrt((C * C).sum(axis=0)))
        acc += float(np.abs(Md - C).sum()) + float(((Md - C) ** 2).sum())
        for n in range(N):
            Cn = C - PA[:, n][:, None] * E[s, n][None, :]
            acc += float(((Md * Cn).sum(axis=0) / (nm * np.sqrt((Cn * Cn).sum(axis=0)))).sum())
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, cos, acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=96)
    ap.add_argument("--G", type=int, default=10000)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--form", type=int, default=0)
    ap.add_argument("--stage", type=int, default=None)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-samples", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.form:
        os.environ["BNMF_REC_FORM"] = "1"
    if a.stage is not None:
        os.environ["BNMF_REC_STAGE"] = str(a.stage)
    if a.batch:
        os.environ["BNMF_REC_BATCH"] = str(a.batch)
    import numpy as np
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    K, G, N, S = a.K, a.G, a.N, a.window
    M, _, _ = synth_counts(K, G, min(5, N), 20251016)
    e = Engine(M, N, likelihood="poisson", prior="gamma", seed=3, window=S, device=a.device)
    apply_hyperprior_params(e, "gamma", M, N)
    e.init()
    t0 = time.perf_counter()
    e.run(S, metrics=False)
    fill_s = time.perf_counter() - t0
    out = dict(K=K, G=G, N=N, window=S, calls=a.calls, form=a.form, stage=a.stage, batch=a.batch, fill_s=fill_s)
    first = e.reconstruction(S)                                     # untimed: grows the scratch, loads the kernels
    for tag, kw in (("all", dict(drop=True)), ("tumour_only", dict(drop=False))):
        times = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            w = e.reconstruction(S, **kw)
            times.append(time.perf_counter() - t0)
        assert np.array_equal(w["tumour"], first["tumour"], equal_nan=True)
        out.update({f"ms_median_{tag}": 1e3 * statistics.median(times), f"ms_min_{tag}": 1e3 * min(times), f"ms_max_{tag}": 1e3 * max(times)})
    out.update(n_undefined=first["n_undefined"], n_poor=first["n_poor"], n_needed=first["n_needed"], worst_cosine=first["worst_cosine"],
               mean_cosine=float(np.nanmean(first["tumour"][0])), ring_bytes=8.0 * S * (K * N + N * G + N),
               fp64_operations=float(S) * G * K * (9.0 * N + 9.0))
    if a.host:
        nf = min(a.host_samples, S)
        tc, tf, cos, _ = host_reconstruction(e, S, nf, M)
        used = np.zeros(S, dtype=np.int32)
        used[:nf] = 1
        dev = e.reconstruction(S, used=used, drop=False)["tumour"][0]
        out.update(host_copy_s=tc, host_s_for_samples=tf, host_samples=nf, host_s_scaled=tf * S / nf, host_threads=os.environ.get("OMP_NUM_THREADS"),
                   host_max_diff_cosine=float(np.nanmax(np.abs(dev - cos.mean(axis=0)))))
    e.close()
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
