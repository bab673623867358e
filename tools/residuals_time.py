"""Time of bnmf_residuals (residual structure of a recorded range on the device, csrc/residuals.h) at a given shape and window.

    python tools/residuals_time.py --K 96 --G 10000 --N 20 --window 1000 [--steps 100] [--calls 9] [--form 1] [--batch B] [--host]

Creates a Poisson-Gamma chain, runs it until the window is full, and times Engine.residuals(window) over all samples of the window: wall
time around the call, which returns after its own stream synchronisation with the results on the host (the copies of the scores and the
finish on the host included); one untimed call first, then the median, minimum and maximum of --calls synchronised calls.  --form 1: the
small tile of the Gram pass and the fit without registers; --batch: the samples of a batch (the same bits).  Prints one JSON line with
the separate fp64 operations of the Gram pass (per sample K (K + 1) / 2 products and as many additions per member, the tiles' unused
corner not counted) and of the fit (2 N per cell), their rates, and the bytes of z that the Gram pass reads through the caches (per
pair of tiles 2 T rows of m doubles).  --host also times the host's route: the window copied out with bnmf_window (timed as it is),
then over --host-samples samples spread evenly over the window the numpy restatement in matrix form (the fit and z by a matrix product,
C_s = z z' / m, numpy's symmetric eigensolver for the leading component), scaled to the window; and the largest difference of that
double-precision share_s from the device's over those samples.  The host is the yardstick, not the code under test.
Not a test."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_residuals(e, S, which, M):
    """the window copied to the host, then per sample of `which` z, C_s and its leading share in matrix form; returns (seconds: copy, the
    samples; share len(which))"""
    import numpy as np
    t0 = time.perf_counter()
    P, E, A = np.stack(e.window("P", S)), np.stack(e.window("E", S)), np.stack(e.window("A", S)).reshape(S, -1)
    t1 = time.perf_counter()
    Md = np.asarray(M, dtype=np.float64)
    share = np.zeros(len(which))
    for k, s in enumerate(which):
        lam = np.maximum((P[s] * A[s][None, :]) @ E[s], 1e-6)
        z = (Md - lam) / np.sqrt(lam)
        C = z @ z.T / z.shape[1]
        w = np.linalg.eigvalsh(C)
        share[k] = w[-1] / np.trace(C)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, share


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=96)
    ap.add_argument("--G", type=int, default=10000)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--form", type=int, default=None)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-samples", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.form is not None:
        os.environ["BNMF_RES_FORM"] = str(a.form)
    if a.batch:
        os.environ["BNMF_RES_BATCH"] = str(a.batch)
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
    out = dict(K=K, G=G, N=N, window=S, n_steps=a.steps, calls=a.calls, form=a.form, batch=a.batch, fill_s=fill_s)
    first = e.residuals(S, n_steps=a.steps)                             # untimed: grows the scratch, loads the kernels
    times = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        w = e.residuals(S, n_steps=a.steps)
        times.append(time.perf_counter() - t0)
    assert np.array_equal(w["gram"], first["gram"], equal_nan=True) and np.array_equal(w["tumour"], first["tumour"], equal_nan=True)
    T = 4 if a.form == 1 else 8
    nt = (K + T - 1) // T
    gram_ops = float(S) * G * K * (K + 1)
    fit_ops = float(S) * G * K * 2.0 * N
    z_reads = float(S) * (nt * (nt + 1) // 2) * 2 * T * G * 8.0
    med = statistics.median(times)
    out.update(ms_median=1e3 * med, ms_min=1e3 * min(times), ms_max=1e3 * max(times), gram_fp64_operations=gram_ops, fit_fp64_operations=fit_ops,
               fp64_operations_per_s=(gram_ops + fit_ops) / med, z_bytes_read=z_reads, z_bytes_per_s=z_reads / med, z_bytes_written=8.0 * S * K * G,
               n_flat=first["n_flat"], share=first["share"], mean_share=first["mean_share"], move=first["move"], min_agreement=first["min_agreement"],
               n_overdispersed=first["n_overdispersed"], worst_type=first["worst_type"], ring_bytes=8.0 * S * (K * N + N * G + N))
    if a.host:
        nf = min(a.host_samples, S)
        which = np.linspace(0, S - 1, nf).astype(int)
        tc, tf, share = host_residuals(e, S, which, M)
        out.update(host_copy_s=tc, host_s_for_part=tf, host_samples=nf, host_s_scaled=tf * S / nf, host_threads=os.environ.get("OMP_NUM_THREADS"),
                   host_share_max_abs_diff=float(np.abs(share - first["series"][2][which]).max()),
                   device_move_max=float(np.nanmax(first["series"][3])))
    e.close()
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
