"""Time of bnmf_relabel (label-switching correction of the recorded window on the device, csrc/relabel.h) at a given shape and window.

    python tools/relabel_time.py --K 96 --G 10000 --N 20 --window 1000 [--calls 9] [--host] [--max-rounds 10]

Creates a Poisson-Gamma chain, runs it until the window is full, and times Engine.relabel(window) over all samples of the window with
the NULL pivot, once with the permutations and the aligned moments only and once with aligned_P / aligned_E as well: wall time around the
call, which returns after its own stream synchronisation with the results on the host; one untimed call first, then the median, minimum
and maximum of --calls calls.  Prints one JSON line: the times, the rounds the call ran, the ring bytes one pass of the accumulation
reads (S (N G + K N) 8), and the rate the whole call amounts to if every round read P once and the last round both rings twice (mean,
then variance).  --host also does the work on the host: the window copied out with bnmf_window, then per round numpy cosines and
scipy.optimize.linear_sum_assignment per sample, the aligned mean as the next pivot, the same stopping rule, and np.mean / np.var of the
aligned samples at the end (sums in numpy's own order); copy and compute timed apart; the permutations are compared with the
device's.  The host is the yardstick, not the code under test.  Not a test."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_relabel(e, S, max_rounds):
    """returns (seconds: copy, compute; perm [S][N], rounds)"""
    import numpy as np
    from scipy.optimize import linear_sum_assignment
    t0 = time.perf_counter()
    P, E = np.stack(e.window("P", S)), np.stack(e.window("E", S))
    t1 = time.perf_counter()
    N = P.shape[2]
    cs = P.sum(axis=1)
    x, ee = P / cs[:, None, :], E * cs[:, :, None]
    piv = P[-1]
    prev = np.tile(np.arange(N), (S, 1))
    rounds = 0
    for r in range(1, max_rounds + 1):
        C = np.einsum("skn,kj->snj", P, piv) / np.sqrt((P * P).sum(axis=1)[:, :, None] * (piv * piv).sum(axis=0)[None, None, :])
        perm = np.stack([linear_sum_assignment(-C[s])[1] for s in range(S)])
        rounds = r
        changed = int((perm != prev).any(axis=1).sum())
        prev = perm
        inv = np.argsort(perm, axis=1)
        if changed == 0 or r == max_rounds:
            break
        piv = np.take_along_axis(x, inv[:, None, :], axis=2).mean(axis=0)
    aP, aE = np.take_along_axis(x, inv[:, None, :], axis=2), np.take_along_axis(ee, inv[:, :, None], axis=1)
    aP.mean(axis=0), aP.var(axis=0, ddof=1), aE.mean(axis=0), aE.var(axis=0, ddof=1)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, perm, rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=96)
    ap.add_argument("--G", type=int, default=10000)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--max-rounds", type=int, default=10)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
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
    pass_bytes = S * (N * G + K * N) * 8
    _, copy_gbs = ubench(a.device)
    out = dict(K=K, G=G, N=N, window=S, calls=a.calls, max_rounds=a.max_rounds, fill_s=fill_s, pass_bytes=pass_bytes, copy_GBps=copy_gbs)
    for tag, aligned in (("moments", False), ("aligned", True)):
        first = e.relabel(S, max_rounds=a.max_rounds, aligned=aligned)         # untimed: grows the scratch, loads the kernels
        times = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            w = e.relabel(S, max_rounds=a.max_rounds, aligned=aligned)
            times.append(time.perf_counter() - t0)
        assert np.array_equal(w["perm"], first["perm"]) and np.array_equal(w["E_var"], first["E_var"])
        med = statistics.median(times)
        read = 2 * pass_bytes + (w["rounds"] - 1) * S * K * N * 8
        out.update({f"{tag}_ms_median": 1e3 * med, f"{tag}_ms_min": 1e3 * min(times), f"{tag}_ms_max": 1e3 * max(times),
                    f"{tag}_ring_GBps": read / med / 1e9, f"{tag}_fraction_of_copy_bandwidth": read / med / 1e9 / copy_gbs})
    out.update({k: w[k] for k in ("rounds", "converged", "n_switched", "n_unmatched", "mean_cosine", "min_cosine")})
    if a.host:
        tc, tn, perm, rounds = host_relabel(e, S, a.max_rounds)
        out.update(host_copy_s=tc, host_numpy_scipy_s=tn, host_rounds=rounds, host_threads=os.environ.get("OMP_NUM_THREADS"),
                   host_samples_with_another_permutation=int((perm != w["perm"]).any(axis=1).sum()))
    e.close()
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
