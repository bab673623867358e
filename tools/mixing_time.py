"""Time of bnmf_mixing (mixing diagnostics of the recorded window on the device, csrc/mixing.h) at a given shape and window.

    python tools/mixing_time.py --K 96 --G 10000 --N 20 --window 1000 [--calls 9] [--host]
    python tools/mixing_time.py --K 96 --G 64 --N 5 --window 1000 --host

Creates a Poisson-Gamma chain, runs it until the window is full, and times Engine.mixing(window, arrays=False) over all samples of the
window: wall time around the call, which returns after its own stream synchronisation with the summary on the host (the 11 rows of
every element are copied to the host inside the call: the summary is scanned there); one untimed call first, then the median (and
minimum) of --calls calls.  Prints one JSON line: the time, the ring bytes the kernels read (S (K N + N G) 8 for the series and
S K N 8 once more for the column sums), the rate that is, its fraction of the device's measured copy bandwidth (bnmf_ubench: a
device-to-device copy, read + write counted), and the distribution of `pairs` (the Gammas summed per element: two lags each, which
sets the cost).  --host also evaluates the same window with the vectorised restatement of tests/mixing_ref.py on the host (window
copied out with bnmf_window, timed apart from the computation) and reports whether the rows agree bit for bit.  Not a test."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=96)
    ap.add_argument("--G", type=int, default=10000)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import numpy as np
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import ubench, MIX_ROWS
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    K, G, N, S = a.K, a.G, a.N, a.window
    M, _, _ = synth_counts(K, G, min(5, N), 20251016)
    e = Engine(M, N, likelihood="poisson", prior="gamma", seed=3, window=S, device=a.device)
    apply_hyperprior_params(e, "gamma", M, N)
    e.init()
    t0 = time.perf_counter()
    e.run(S, metrics=False)
    fill_s = time.perf_counter() - t0
    first = e.mixing(S, arrays=False)                                # untimed: grows the scratch, loads the kernels
    times = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        w = e.mixing(S, arrays=False)
        times.append(time.perf_counter() - t0)
    assert all(w[k] == first[k] or (w[k] != w[k] and first[k] != first[k]) for k in w)
    full = e.mixing(S)
    pairs = np.concatenate([full["pairs_P"].ravel(), full["pairs_E"].ravel()])
    q = [int(v) for v in np.quantile(pairs, [0.0, 0.25, 0.5, 0.75, 0.95, 0.99, 1.0])]
    _, copy_gbs = ubench(a.device)
    nbytes = S * (2 * K * N + N * G) * 8
    med = statistics.median(times)
    out = dict(K=K, G=G, N=N, window=S, calls=a.calls, fill_s=fill_s, mixing_ms_median=1e3 * med, mixing_ms_min=1e3 * min(times),
               ring_bytes=nbytes, ring_GBps=nbytes / med / 1e9, copy_GBps=copy_gbs, fraction_of_copy_bandwidth=nbytes / med / 1e9 / copy_gbs,
               elements=K * N + N * G, pairs_quantiles_0_25_50_75_95_99_100=q, pairs_mean=float(pairs.mean()),
               **{k: w[k] for k in ("n_const", "n_ran_out", "n_low_ess", "n_high_rhat", "min_ess_P", "min_ess_E", "max_rhat_P", "max_rhat_E")})
    if a.host:
        from mixing_ref import mixing_reference, renormalised_series
        t0 = time.perf_counter()
        Pw, Ew = np.stack(e.window("P", S)), np.stack(e.window("E", S))
        t1 = time.perf_counter()
        xP, xE = renormalised_series(Pw, Ew)
        rP, rE = mixing_reference(xP), mixing_reference(xE)
        t2 = time.perf_counter()
        same = all(np.array_equal(np.nan_to_num(r[k], nan=-1.0).view(np.uint64),
                                  np.nan_to_num(full[f"{k}_{s}"].ravel(order="F"), nan=-1.0).view(np.uint64))
                   for s, r in (("P", rP), ("E", rE)) for k in MIX_ROWS)
        out.update(host_copy_s=t1 - t0, host_numpy_s=t2 - t1, host_threads=os.environ.get("OMP_NUM_THREADS"), host_rows_bit_equal=bool(same))
    e.close()
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
