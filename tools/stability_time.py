"""Time of bnmf_stability (silhouette stability of the recorded signatures on the device, csrc/stability.h) at a given shape and window.

    python tools/stability_time.py --K 96 --G 10000 --N 20 --window 1000 [--calls 9] [--host]

Creates a Poisson-Gamma chain, runs it until the window is full, and times Engine.stability(window) over all samples of the window:
wall time around the call, which returns after its own stream synchronisation with the results on the host (the finish on the host
included); one untimed call first, then the median, minimum and maximum of --calls synchronised calls.  Prints one JSON line.  --host also
times the host's route: the window copied out with bnmf_window (timed as it is), the columns scaled to unit length, then the
matrix-product form 1 - U_rows U^T and the per-cluster means over the first --host-samples samples' worth of rows (default 50 samples, N
rows each) against all columns, that time scaled by window / host-samples (every row is independent work: the scaling is linear), and
reports the largest difference of those rows' silhouettes from the device's.  The host is the yardstick, not the code under test.  Not a
test."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_stability(e, S, n_fit):
    """the window copied to the host, then the silhouettes of the first n_fit samples' points by matrix products; returns (seconds:
    copy, the rows; silhouettes n_fit x N)"""
    import numpy as np
    t0 = time.perf_counter()
    P, A = np.stack(e.window("P", S)), np.stack(e.window("A", S)).reshape(S, -1)
    t1 = time.perf_counter()
    N = P.shape[2]
    cols = np.moveaxis(P, 1, 2).reshape(S * N, -1)
    Un = cols / np.sqrt((cols * cols).sum(axis=1))[:, None]
    lab = np.tile(np.arange(N), S)
    onehot = np.zeros((S * N, N))
    onehot[np.arange(S * N), lab] = 1.0
    rows = n_fit * N
    d = 1.0 - Un[:rows] @ Un.T                                     # rows x S N
    tot = d @ onehot                                               # the sums per cluster (the self term is 1 - 1)
    own = lab[:rows]
    a = tot[np.arange(rows), own] / (S - 1)
    tot[np.arange(rows), own] = np.inf
    b = (tot / S).min(axis=1)
    sil = (b - a) / np.maximum(a, b)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, sil.reshape(n_fit, N), (A != 0).all()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=96)
    ap.add_argument("--G", type=int, default=10000)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-samples", type=int, default=50)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
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
    out = dict(K=K, G=G, N=N, window=S, calls=a.calls, fill_s=fill_s)
    first = e.stability(S)                                         # untimed: grows the scratch, loads the kernels
    times = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        w = e.stability(S)
        times.append(time.perf_counter() - t0)
    assert np.array_equal(w["point"], first["point"], equal_nan=True)
    med = statistics.median(times)
    out.update(n_points=w["n_points"], n_clusters=w["n_clusters"], n_left_out=w["n_left_out"], ms_median=1e3 * med, ms_min=1e3 * min(times),
               ms_max=1e3 * max(times), mean_silhouette=w["mean_silhouette"], min_stability=w["min_stability"], min_stability_at=w["min_stability_at"],
               multiply_adds=float(w["n_points"]) ** 2 * K)
    if a.host:
        nf = min(a.host_samples, S)
        tc, tf, sil, all_in = host_stability(e, S, nf)
        out.update(host_copy_s=tc, host_s_for_samples=tf, host_samples=nf, host_s_scaled=tf * S / nf, host_threads=os.environ.get("OMP_NUM_THREADS"),
                   host_max_diff_silhouette=float(np.nanmax(np.abs(w["point"][0, :nf * N].reshape(nf, N) - sil))) if all_in else None)
    e.close()
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
