"""Time of bnmf_similarity (similarity of tumours over a recorded range on the device, csrc/similarity.h) at a given shape and window.

    python tools/similarity_time.py --K 96 --G 10000 --N 20 --window 1000 [--calls 9] [--top-k 10] [--queries 16] [--band B] [--host]

Creates a Poisson-Gamma chain, runs it until the window is full, and times Engine.similarity(window) over all samples of the window:
wall time around the call, which returns after its own stream synchronisation with the results on the host (the finish on the host
included); one untimed call first, then the median, minimum and maximum of --calls synchronised calls, once over all pairs with the
neighbours and the per-tumour table, and once for --queries tumours alone (top_k = 0, no table: only those rows are computed).  --band:
the rows of a band (the same bits).  Prints one JSON line with the separate fp64 multiplies and adds the pairs need (2 N per pair and
sample over the m x m pairs of the pass, the square root, the division and Welford's step not counted) and their rate over the call.
--host also times the host's route: the window copied out with bnmf_window (timed as it is), then per sample the normalised profiles and
U^T U by a numpy matrix product for the first --host-rows tumours against all tumours over the first --host-samples samples, mean and
variance accumulated; that time scaled by (window / host-samples) x (G / host-rows) (every sample and every row is independent work of
equal size: the scaling is linear), and the largest difference of those rows' mean cosines from the device's over the same samples.
The host is the yardstick, not the code under test.  Not a test."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_similarity(e, S, n_fit, rows):
    """the window copied to the host, then the mean cosine of the first `rows` tumours against all over the first n_fit samples by matrix
    products; returns (seconds: copy, the samples; mean rows x G)"""
    import numpy as np
    t0 = time.perf_counter()
    P, E, A = np.stack(e.window("P", S)), np.stack(e.window("E", S)), np.stack(e.window("A", S)).reshape(S, -1)
    t1 = time.perf_counter()
    G = E.shape[2]
    mean, m2 = np.zeros((rows, G)), np.zeros((rows, G))
    for s in range(n_fit):
        x = E[s] * (P[s].sum(axis=0) * (A[s] != 0))[:, None]
        U = x / np.sqrt((x * x).sum(axis=0))
        c = U[:, :rows].T @ U
        d = c - mean
        mean += d / (s + 1)
        m2 += d * (c - mean)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, mean


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=96)
    ap.add_argument("--G", type=int, default=10000)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--band", type=int, default=None)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-samples", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=1000)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.band:
        os.environ["BNMF_SIM_BAND"] = str(a.band)
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
    out = dict(K=K, G=G, N=N, window=S, calls=a.calls, top_k=a.top_k, queries=a.queries, band=a.band, fill_s=fill_s)
    q = np.linspace(0, G - 1, a.queries).astype(np.int32)
    forms = (("all", dict(top_k=a.top_k), float(G) * G), ("queries", dict(top_k=0, query=q, tumour=False), float(a.queries) * G))
    first = {}
    for tag, kw, pairs in forms:
        first[tag] = e.similarity(S, **kw)                          # untimed: grows the scratch, loads the kernels
        times = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            w = e.similarity(S, **kw)
            times.append(time.perf_counter() - t0)
        key = "tumour" if tag == "all" else "dense"
        assert np.array_equal(w[key], first[tag][key], equal_nan=True)
        ops = pairs * S * 2.0 * N
        out.update({f"ms_median_{tag}": 1e3 * statistics.median(times), f"ms_min_{tag}": 1e3 * min(times), f"ms_max_{tag}": 1e3 * max(times),
                    f"fp64_operations_{tag}": ops, f"fp64_operations_per_s_{tag}": ops / statistics.median(times)})
    r = first["all"]
    out.update(n_pairs=r["n_pairs"], n_similar_pairs=r["n_similar_pairs"], n_isolated=r["n_isolated"], mean_similarity=r["mean_similarity"],
               least_typical=r["least_typical"], ring_bytes=8.0 * S * (K * N + N * G + N))
    if a.host:
        nf, rows = min(a.host_samples, S), min(a.host_rows, G)
        tc, tf, mean = host_similarity(e, S, nf, rows)
        used = np.zeros(S, dtype=np.int32)
        used[:nf] = 1
        dev = e.similarity(S, used=used, query=np.arange(rows, dtype=np.int32), top_k=0, tumour=False)["dense"][0]
        off = ~np.isnan(dev)
        out.update(host_copy_s=tc, host_s_for_part=tf, host_samples=nf, host_rows=rows, host_s_scaled=tf * (S / nf) * (G / rows),
                   host_threads=os.environ.get("OMP_NUM_THREADS"), host_max_diff_mean=float(np.abs(dev - mean)[off].max()))
    e.close()
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
