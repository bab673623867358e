"""Time of bnmf_coactivity (co-activity of signatures over the recorded window on the device, csrc/coactivity.h) at a given shape and
window.

    python tools/coactivity_time.py --K 96 --G 10000 --N 20 --window 1000 [--calls 9] [--host] [--form 0|1] [--chunk C] [--width T] [--batch B]

Creates a Poisson-Gamma chain, runs it until the window is full, and times Engine.coactivity(window) over all samples of the window and all
tumours: wall time around the call, which returns after its own stream synchronisation with the results on the host (the host's reduction
over the samples included); one untimed call first, then the median, minimum and maximum of --calls synchronised calls.  Prints one JSON
line.  --host also times the host's route: the window copied out with bnmf_window (timed as it is), then per sample the loads,
scipy.stats.spearmanr and numpy.corrcoef over the first --host-samples samples (default 4), that time scaled by window / host-samples
(every sample is independent work: the scaling is linear), and reports the largest differences of v0 and v1 over those samples from the
host's values.  --form 1 forces the narrow tiles and the ranks through sorted chunks in the scratch (BNMF_COA_FORM); --chunk, --width and
--batch set BNMF_COA_CHUNK (doubles of a sorted chunk), BNMF_COA_WIDTH (threads of the sorting workgroup: 256, 512, 1,024) and
BNMF_COA_BATCH (samples per batch).  The host is the yardstick, not the code under test.  Not a test."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_coactivity(e, S, n_fit):
    """the window copied to the host, then the loads, spearmanr and corrcoef over the first n_fit samples; returns (seconds: copy, n_fit
    samples; pearson and spearman n_fit x N x N)"""
    import numpy as np
    import scipy.stats
    t0 = time.perf_counter()
    P, E, A = np.stack(e.window("P", S)), np.stack(e.window("E", S)), np.stack(e.window("A", S)).reshape(S, -1)
    t1 = time.perf_counter()
    pe, sp = [], []
    for s in range(n_fit):
        x = np.where((A[s] != 0)[:, None], E[s] * P[s].sum(axis=0)[:, None], 0.0)              # N x G
        with np.errstate(invalid="ignore", divide="ignore"):
            pe.append(np.corrcoef(x))
            sp.append(np.asarray(scipy.stats.spearmanr(x, axis=1).statistic))
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, np.stack(pe), np.stack(sp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=96)
    ap.add_argument("--G", type=int, default=10000)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-samples", type=int, default=4)
    ap.add_argument("--form", type=int, choices=[0, 1], default=None)
    ap.add_argument("--chunk", type=int, default=None)
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    for name, v in (("BNMF_COA_FORM", a.form), ("BNMF_COA_CHUNK", a.chunk), ("BNMF_COA_WIDTH", a.width), ("BNMF_COA_BATCH", a.batch)):
        if v is not None:
            os.environ[name] = str(v)
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
    out = dict(K=K, G=G, N=N, window=S, calls=a.calls, form=a.form, chunk=a.chunk, width=a.width, batch=a.batch, fill_s=fill_s)
    first = e.coactivity(S)                                      # untimed: grows the scratch, loads the kernels
    times = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        w = e.coactivity(S)
        times.append(time.perf_counter() - t0)
    assert np.array_equal(w["pair"], first["pair"], equal_nan=True)
    med = statistics.median(times)
    out.update(n_included=w["n_included"], n_pairs=w["n_pairs"], n_blocks=w["n_blocks"], ms_median=1e3 * med, ms_min=1e3 * min(times), ms_max=1e3 * max(times),
               n_credible=w["n_credible"], max_cosine=w["max_cosine"], max_cosine_at=w["max_cosine_at"])
    if a.host:
        nf = min(a.host_samples, S)
        tc, tf, pe, sp = host_coactivity(e, S, nf)
        ser = e.coactivity(S, series=True)["series"]
        ia, ib = [p[0] for p in w["pairs"]], [p[1] for p in w["pairs"]]
        d0 = np.abs(ser[0, :nf] - pe[:, ia, ib])
        d1 = np.abs(ser[1, :nf] - sp[:, ia, ib])
        out.update(host_copy_s=tc, host_s_for_samples=tf, host_samples=nf, host_s_scaled=tf * S / nf, host_max_diff_pearson=float(np.nanmax(d0)),
                   host_max_diff_spearman=float(np.nanmax(d1)), host_threads=os.environ.get("OMP_NUM_THREADS"))
    e.close()
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
