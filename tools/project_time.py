"""Time of bnmf_project (exposures of new tumours under the recorded signatures on the device, csrc/project.h) at a given shape.

    python tools/project_time.py --K 96 --G 10000 --N 20 --window 1000 --J 1000 --steps 200 [--calls 9] [--forms] [--host] [--host-samples 3]

Creates a Poisson-Gamma chain, runs it until the window is full, and times Engine.project(window, X) over all samples of the window
for J new tumours drawn by synth_counts: wall time around the call, which returns after its own stream synchronisation with the
results on the host; one untimed call first, then the median, minimum and maximum of --calls calls.  Prints one JSON line: the
times, the floating-point operations of the spec (S J steps 4 K N, the division per row and the padding of the kernel not counted)
and the rate that is.  --forms times the call with BNMF_PROJ_STAGE=1 (x staged in the LDS) and with BNMF_PROJ_STAGE=0 (x read
through the caches at wave-uniform addresses) instead of the default form, and checks that the bits are the same.  --host also evaluates the refit with numpy on the host (window
copied out with bnmf_window, then per sample C = x e, Q = X / C, e = e * (x' Q) as matrix products; sums in BLAS's own order), the
copy and the compute timed apart; the compute runs over the first --host-samples samples of the window and is scaled to the whole
window (it is linear in the samples), and the largest relative difference of the mean exposures over those samples' own device call
is reported.  The host is the yardstick, not the code under test.  Not a test."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_project(e, X, S, H, steps):
    """the window copied to the host and the KL refit in numpy float64 over its first H samples; returns (seconds: copy, compute;
    the mean exposures N x J)"""
    import numpy as np
    t0 = time.perf_counter()
    P, A = e.window("P", S), e.window("A", S)
    t1 = time.perf_counter()
    t = X.sum(axis=0)
    mu = None
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(H):
            cs = P[s].sum(axis=0)
            part = (A[s].ravel() != 0) & (cs > 0)
            x = P[s][:, part] / cs[part][None, :]
            ex = np.tile(t[None, :] / max(int(part.sum()), 1), (x.shape[1], 1))
            for _ in range(steps):
                c = x @ ex
                ex = ex * (x.T @ np.where(c > 0.0, X / c, 0.0))
            a = np.zeros((P[s].shape[1], X.shape[1]))
            a[part] = ex
            mu = a if mu is None else mu + (a - mu) * (1.0 / (s + 1))
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, mu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=96)
    ap.add_argument("--G", type=int, default=10000)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--J", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--forms", action="store_true")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-samples", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import numpy as np
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    K, G, N, S, J = a.K, a.G, a.N, a.window, a.J
    M, _, _ = synth_counts(K, G, min(5, N), 20251016)
    X = np.asfortranarray(synth_counts(K, J, min(5, N), 20251017)[0], dtype=np.float64)
    e = Engine(M, N, likelihood="poisson", prior="gamma", seed=3, window=S, device=a.device)
    apply_hyperprior_params(e, "gamma", M, N)
    e.init()
    t0 = time.perf_counter()
    e.run(S, metrics=False)
    fill_s = time.perf_counter() - t0
    flops = 4.0 * S * J * a.steps * K * N
    out = dict(K=K, G=G, N=N, window=S, J=J, steps=a.steps, calls=a.calls, fill_s=fill_s, spec_flops=flops)
    first = None
    for tag, env in (("staged", "1"), ("uniform", "0")) if a.forms else (("default", None),):
        if env is not None:
            os.environ["BNMF_PROJ_STAGE"] = env
        warm = e.project(S, X, n_steps=a.steps)                  # untimed: grows the scratch, loads the kernel
        times = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            w = e.project(S, X, n_steps=a.steps)
            times.append(time.perf_counter() - t0)
        os.environ.pop("BNMF_PROJ_STAGE", None)
        first = first or warm
        assert w["total"] == first["total"] and np.array_equal(w["load"], first["load"]) and np.array_equal(w["fit"], first["fit"], equal_nan=True)
        med = statistics.median(times)
        out.update({f"{tag}_ms_median": 1e3 * med, f"{tag}_ms_min": 1e3 * min(times), f"{tag}_ms_max": 1e3 * max(times),
                    f"{tag}_spec_TFLOPs": flops / med / 1e12})
    out.update(total=w["total"], sum_of_X=float(X.sum()), max_rel_change=w["max_rel_change"], min_cosine=w["min_cosine"])
    if a.host:
        H = max(2, min(a.host_samples, S))
        tc, tn, mu = host_project(e, X, S, H, a.steps)
        dev = e.project(H, X, end_iter=e.iter - S + H, n_steps=a.steps)["load_mean"]
        out.update(host_copy_s=tc, host_samples=H, host_numpy_s_measured=tn, host_numpy_s_scaled_to_window=tn * S / H,
                   host_threads=os.environ.get("OMP_NUM_THREADS"), host_max_rel_diff=float(np.max(np.abs(mu - dev) / np.maximum(np.abs(dev), 1.0))))
    e.close()
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
