"""Time of bnmf_prune (sparse per-tumour assignment with refit over a recorded range on the device, csrc/prune.h) at a given shape and
window.

    python tools/prune_time.py --K 96 --G 10000 --N 20 --window 1000 [--calls 9] [--steps 20] [--max-loss 0.01] [--form 1] [--batch B] [--host]

Creates a Poisson-Gamma chain, runs it until the window is full, and times Engine.prune(window) over all samples of the window: wall
time around the call, which returns after its own stream synchronisation with the results on the host (the finish on the host
included); one untimed call first, then the median, minimum and maximum of --calls synchronised calls.  Beside it the mean trials per
problem and the separate fp64 multiplies, adds and divisions of the steps and cosines the trials ran (per state: n_steps steps of
K (4 NT + 1) and one cosine of K (2 NT + 4), NT the places a lane visits) and their rate.  --form 1: the lane's vectors in the LDS;
--batch: the batch of samples (the same bits).  Prints one JSON line.  --host also times the host's route: the window copied out with
bnmf_window (timed as it is), then the same elimination in numpy, all tumours of a sample at once with matrix products for the fit and
the update and masks for the lanes' different candidates, over the first --host-samples samples (default 3), that time scaled by
window / host-samples (every sample is independent work: the scaling is linear), and reports the largest difference of those samples'
p_kept and mean loads from the device's over the same samples.  The host is the yardstick, not the code under test.  Not a test."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_sample(P, E, A, Md, mm, n_steps, max_loss):
    """one sample, every tumour at once: returns e_sparse (N x G)"""
    import numpy as np
    cs = P.sum(axis=0)
    idx = np.where((A != 0) & (cs > 0))[0]
    x = P[:, idx] / cs[idx]
    G = Md.shape[1]

    def steps(e, act):
        for _ in range(n_steps):
            c = x @ e
            q = np.where(c > 0, Md / np.where(c > 0, c, 1.0), 0.0)
            e = np.where(act, e * (x.T @ q), 0.0)
        return e

    def cosine(e):
        c = x @ e
        cc = (c * c).sum(axis=0)
        return np.where(cc > 0, (Md * c).sum(axis=0) / np.sqrt(mm * np.where(cc > 0, cc, 1.0)), 0.0)

    act = np.ones((len(idx), G), dtype=bool)
    e = steps(E[idx] * cs[idx][:, None], act)
    thr = cosine(e) - max_loss
    tried = np.zeros_like(act)
    lanes = np.arange(G)
    while True:
        ok = act & ~tried & (act.sum(axis=0) > 1)[None, :]
        has = ok.any(axis=0)
        if not has.any():
            break
        c = np.where(ok, e, np.inf).argmin(axis=0)                  # the smallest e, the lower place on a tie
        ta = act.copy()
        ta[c[has], lanes[has]] = False
        te = steps(np.where(ta, e, 0.0), ta)
        acc = has & (cosine(te) >= thr)
        e[:, acc], act[:, acc], tried[:, acc] = te[:, acc], ta[:, acc], False
        rej = has & ~acc
        tried[c[rej], lanes[rej]] = True
    out = np.zeros((P.shape[1], G))
    out[idx] = e
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=96)
    ap.add_argument("--G", type=int, default=10000)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--max-loss", type=float, default=0.01)
    ap.add_argument("--form", type=int, default=0)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-samples", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.form:
        os.environ["BNMF_PRN_FORM"] = "1"
    if a.batch:
        os.environ["BNMF_PRN_BATCH"] = str(a.batch)
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
    kw = dict(n_steps=a.steps, max_loss=a.max_loss)
    out = dict(K=K, G=G, N=N, window=S, calls=a.calls, n_steps=a.steps, max_loss=a.max_loss, form=a.form, batch=a.batch, fill_s=fill_s)
    t0 = time.perf_counter()
    first = e.prune(S, **kw)                                        # untimed: grows the scratch, loads the kernels
    out["first_call_s"] = time.perf_counter() - t0
    times = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        w = e.prune(S, **kw)
        times.append(time.perf_counter() - t0)
        assert np.array_equal(w["tumour"], first["tumour"], equal_nan=True)
    problems = float(S) * (first["n_included"] - first["n_undefined"])
    NT = N if (a.form or N > 32) else ((N + 7) // 8) * 8
    states = float(first["trials"]) + problems                      # every trial and every round 0
    out.update(s_median=statistics.median(times), s_min=min(times), s_max=max(times), trials=first["trials"],
               mean_trials_per_problem=first["trials"] / problems, mean_n_kept=float(np.nanmean(first["tumour"][2])), n_single=first["n_single"],
               max_change=first["max_change"], fp64_operations=states * (a.steps * K * (4.0 * NT + 1.0) + K * (2.0 * NT + 4.0)),
               ring_bytes=8.0 * S * (K * N + N * G + N))
    out["fp64_operations_per_s"] = out["fp64_operations"] / out["s_median"]
    if a.host:
        nf = min(a.host_samples, S)
        t0 = time.perf_counter()
        P, E, A = np.stack(e.window("P", S)), np.stack(e.window("E", S)), np.stack(e.window("A", S)).reshape(S, -1)
        t1 = time.perf_counter()
        Md = np.asarray(M, dtype=np.float64)
        mm = (Md * Md).sum(axis=0)
        es = np.stack([host_sample(P[s], E[s], A[s], Md, mm, a.steps, a.max_loss) for s in range(nf)])
        t2 = time.perf_counter()
        used = np.zeros(S, dtype=np.int32)
        used[:nf] = 1
        dev = e.prune(S, used=used, **kw)
        out.update(host_copy_s=t1 - t0, host_s_for_samples=t2 - t1, host_samples=nf, host_s_scaled=(t2 - t1) * S / nf,
                   host_threads=os.environ.get("OMP_NUM_THREADS"), host_max_diff_p_kept=float(np.nanmax(np.abs(dev["p_kept"] - (es > 0).mean(axis=0)))),
                   host_max_diff_load=float(np.nanmax(np.abs(dev["load_mean"] - es.mean(axis=0)))),
                   host_max_rel_diff_load=float(np.nanmax(np.abs(dev["load_mean"] - es.mean(axis=0)) / np.maximum(Md.sum(axis=0), 1.0)[None, :])))
    e.close()
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
