"""Time of bnmf_subtypes (subtypes of tumours over a recorded range on the device, csrc/subtypes.h) at a given shape and window.

    python tools/subtypes_time.py --K 96 --G 10000 --N 20 --window 1000 [--C 8] [--steps 50] [--calls 9] [--form 1] [--batch B] [--host]

Creates a Poisson-Gamma chain, runs it until the window is full, and times Engine.subtypes(window) over all samples of the window from a
farthest-first start over the last sample's share profiles: wall time around the call, which returns after its own stream
synchronisation with the results on the host (the finish on the host included); one untimed call first, then the median, minimum and
maximum of --calls synchronised calls.  --form 1: the tiled form where the other would run; --batch: the samples of a batch (the same
bits).  Prints one JSON line with the Lloyd steps run in all, the separate fp64 operations they need (per step and assigned tumour
3 N C for the distances and N C for the centres' accumulators, the share profile and the divisions not counted), their rate, and the
bytes of E the steps read (per step every member's column once for the total, once per chunk of 8 clusters and once per tile of the
update).  --host also times the host's route: the window copied out with bnmf_window (timed as it is), then over --host-samples
samples spread evenly over the window a plain numpy k-means with matrix products from the same start and the same number of steps as
the device ran for that sample; that time scaled by the steps of the whole window over the steps of those samples (every step is work
of equal size), and the share of labels that agree with the device's.  The host is the yardstick, not the code under test.
Not a test."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_kmeans(e, S, which, c0, steps):
    """the window copied to the host, then per sample of `which` a numpy Lloyd iteration of steps[s] steps from c0; returns
    (seconds: copy, the samples; labels len(which) x G)"""
    import numpy as np
    t0 = time.perf_counter()
    P, E, A = np.stack(e.window("P", S)), np.stack(e.window("E", S)), np.stack(e.window("A", S)).reshape(S, -1)
    t1 = time.perf_counter()
    G = E.shape[2]
    labels = np.zeros((len(which), G), dtype=np.int64)
    for k, s in enumerate(which):
        x = E[s] * (P[s].sum(axis=0) * (A[s] != 0))[:, None]
        q = x / x.sum(axis=0)
        mu = c0.copy()
        for _ in range(int(steps[s])):
            d = (q * q).sum(axis=0)[:, None] - 2.0 * (q.T @ mu) + (mu * mu).sum(axis=0)[None, :]
            lab = d.argmin(axis=1)
            onehot = np.zeros((G, mu.shape[1]))
            onehot[np.arange(G), lab] = 1.0
            cnt = onehot.sum(axis=0)
            mu = np.where(cnt > 0, (q @ onehot) / np.where(cnt > 0, cnt, 1.0), mu)
        labels[k] = lab
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=96)
    ap.add_argument("--G", type=int, default=10000)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--C", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--form", type=int, default=None)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-samples", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.form is not None:
        os.environ["BNMF_SUB_FORM"] = str(a.form)
    if a.batch:
        os.environ["BNMF_SUB_BATCH"] = str(a.batch)
    import numpy as np
    from bayesnmf_amd import Engine
    from bayesnmf_amd.sampler import subtype_seeds
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    K, G, N, S, Cn = a.K, a.G, a.N, a.window, a.C
    M, _, _ = synth_counts(K, G, min(5, N), 20251016)
    e = Engine(M, N, likelihood="poisson", prior="gamma", seed=3, window=S, device=a.device)
    apply_hyperprior_params(e, "gamma", M, N)
    e.init()
    t0 = time.perf_counter()
    e.run(S, metrics=False)
    fill_s = time.perf_counter() - t0
    x = np.asarray(e.get("E"), dtype=np.float64) * np.asarray(e.get("P"), dtype=np.float64).sum(axis=0)[:, None]
    prof = x / x.sum(axis=0)
    c0 = np.asfortranarray(prof[:, subtype_seeds(prof, Cn)])
    out = dict(K=K, G=G, N=N, window=S, C=Cn, n_steps=a.steps, calls=a.calls, form=a.form, batch=a.batch, fill_s=fill_s)
    first = e.subtypes(S, c0, n_steps=a.steps, labels=True)             # untimed: grows the scratch, loads the kernels
    times = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        w = e.subtypes(S, c0, n_steps=a.steps)
        times.append(time.perf_counter() - t0)
    assert np.array_equal(w["membership"], first["membership"], equal_nan=True)
    steps = first["series"][1]
    total = float(steps.sum())
    ops = total * G * 4.0 * N * Cn
    reads = total * G * N * 8.0 * (1 + (Cn + 7) // 8 + ((N + 3) // 4) * ((Cn + 7) // 8))
    med = statistics.median(times)
    out.update(ms_median=1e3 * med, ms_min=1e3 * min(times), ms_max=1e3 * max(times), steps_total=total, steps_mean=total / S, steps_max=float(steps.max()),
               n_not_converged=first["n_not_converged"], fp64_operations=ops, fp64_operations_per_s=ops / med, E_bytes_read=reads, E_bytes_per_s=reads / med,
               n_certain=first["n_certain"], mean_certainty=first["mean_certainty"], sizes=first["size"][0].tolist(), ring_bytes=8.0 * S * (K * N + N * G + N))
    if a.host:
        nf = min(a.host_samples, S)
        which = np.linspace(0, S - 1, nf).astype(int)
        tc, tf, lab = host_kmeans(e, S, which, c0, steps)
        out.update(host_copy_s=tc, host_s_for_part=tf, host_samples=nf, host_steps_for_part=float(steps[which].sum()),
                   host_s_scaled=tf * total / float(steps[which].sum()), host_threads=os.environ.get("OMP_NUM_THREADS"),
                   host_labels_agree=float((lab == first["labels"][which]).mean()))
    e.close()
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
