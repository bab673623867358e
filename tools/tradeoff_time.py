"""Time of bnmf_tradeoff (trade-offs between signatures within a tumour over a recorded range on the device, csrc/tradeoff.h) at a given
shape and window.

    python tools/tradeoff_time.py --K 96 --G 10000 --N 20 --window 1000 [--sets 3] [--queries 16] [--calls 9] [--form 1] [--band B] [--host]

Creates a Poisson-Gamma chain, runs it until the window is full, and times Engine.tradeoff(window) over all samples of the window and
all tumours, with --sets sets of signatures dealt round-robin and --queries query tumours spread over the cohort: wall time around the
call, which returns after its own stream synchronisation with the results on the host (the finish on the host included); one untimed
call first, then the median, minimum and maximum of --calls synchronised calls.  --form 1: the tile of 8; --band: the members of a band
(the same bits).  Prints one JSON line with the bytes of the E ring that the two passes read (2 x 8 x window x N x G), their rate over
the median, the device-to-device copy rate bnmf_ubench reports for comparison, and the separate fp64 operations of the co-moment pass
(per sample, tumour and pair l <= j one product and one addition, and N subtractions).  --host also times the host's route: the window
copied out with bnmf_window (timed as it is), then numpy.cov and numpy.corrcoef of the renormalised exposures for --host-tumours
tumours spread over the cohort, that time scaled to all G, and the largest difference of those tumours' covariances (relative to the
largest magnitude in the matrix) and correlations from the device's.  The host is the yardstick, not the code under test.  Not a test."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_cov(e, S, which):
    """the window copied to the host, then per tumour of `which` numpy.cov / corrcoef over the samples; returns (seconds: copy, the
    tumours; cov and r len(which) x N x N)"""
    import numpy as np
    t0 = time.perf_counter()
    P, E, A = np.stack(e.window("P", S)), np.stack(e.window("E", S)), np.stack(e.window("A", S)).reshape(S, -1)
    t1 = time.perf_counter()
    f = P.sum(axis=1) * (A != 0)                                        # S x N
    cov, r = [], []
    with np.errstate(invalid="ignore", divide="ignore"):
        for g in which:
            x = E[:, :, g] * f                                          # S x N
            cov.append(np.cov(x.T, ddof=1).reshape(x.shape[1], x.shape[1]))
            r.append(np.corrcoef(x.T).reshape(x.shape[1], x.shape[1]))
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, np.stack(cov), np.stack(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=96)
    ap.add_argument("--G", type=int, default=10000)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--form", type=int, default=None)
    ap.add_argument("--band", type=int, default=None)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-tumours", type=int, default=16)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.form is not None:
        os.environ["BNMF_TRD_FORM"] = str(a.form)
    if a.band:
        os.environ["BNMF_TRD_BAND"] = str(a.band)
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
    C = min(a.sets, N)
    sets = (np.arange(N) % C).astype(np.int32) if C > 0 else None
    q = np.linspace(0, G - 1, a.queries).astype(np.int32) if a.queries > 0 else None
    out = dict(K=K, G=G, N=N, window=S, sets=C, queries=a.queries, calls=a.calls, form=a.form, band=a.band, fill_s=fill_s)
    first = e.tradeoff(S, sets=sets, query=q)                           # untimed: grows the scratch, loads the kernels
    times = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        w = e.tradeoff(S, sets=sets, query=q)
        times.append(time.perf_counter() - t0)
    assert np.array_equal(w["tumour"], first["tumour"], equal_nan=True) and np.array_equal(w["pair"], first["pair"], equal_nan=True)
    med = statistics.median(times)
    reads = 2.0 * 8.0 * S * N * G
    ops = float(S) * G * (N * (N + 1) + N)
    _, copy_gbs = ubench(a.device)
    out.update(ms_median=1e3 * med, ms_min=1e3 * min(times), ms_max=1e3 * max(times), E_bytes_read=reads, E_bytes_per_s=reads / med, ubench_copy_GBps=copy_gbs,
               ms_at_copy_rate=1e3 * reads / (copy_gbs * 1e9), fp64_operations=ops, fp64_operations_per_s=ops / med, n_traded=first["n_traded"],
               mean_ratio=first["mean_ratio"], strongest_pair=first["strongest_pair"], strongest_pair_at=first["strongest_pair_at"],
               ring_bytes=8.0 * S * (K * N + N * G + N))
    if a.host and q is not None:
        which = q[:min(a.host_tumours, len(q))]
        tc, tf, cov, r = host_cov(e, S, which)
        dev = np.asarray(first["dense"])[:len(which)]
        scale = np.abs(cov).max(axis=(1, 2), keepdims=True)
        off = ~np.eye(N, dtype=bool)
        both = off[None] & ~np.isnan(r) & ~np.isnan(dev[:, 1])
        out.update(host_copy_s=tc, host_s_for_part=tf, host_tumours=len(which), host_s_scaled=tf * G / len(which), host_threads=os.environ.get("OMP_NUM_THREADS"),
                   host_max_rel_cov_diff=float((np.abs(dev[:, 0] - cov) / np.where(scale > 0, scale, 1.0)).max()),
                   host_max_corr_diff=float(np.abs(dev[:, 1] - r)[both].max()) if both.any() else None)
    e.close()
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
