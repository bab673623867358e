"""Time of bnmf_decompose (recorded signatures as mixtures of a reference catalogue on the device, csrc/decompose.h) at a given shape.

    python tools/decompose_time.py --K 96 --G 10000 --N 20 --window 1000 --steps 200 [--min-share 0.05] [--calls 9] [--forms] [--host] [--host-samples 3]

Creates a Poisson-Gamma chain, runs it until the window is full, and times Engine.decompose(window, catalogue) over all samples of
the window against the 79 COSMIC v3.3.1 columns of tests/golden/cosmic_v3.3.1_sbs.npz (K = 96; for another K a catalogue of --R columns
is drawn): wall time around the call, which returns after its own stream synchronisation with the results on the host; one untimed
call first, then the median, minimum and maximum of --calls calls.  Prints one JSON line: the times, the floating-point operations
of the spec (S N 2 steps 4 K R: both stages over all R references, the division per row not counted) and the rate that is.
--forms times the call with BNMF_DEC_STAGE=1 (the catalogue staged in the LDS) and with BNMF_DEC_STAGE=0 (read through the caches at
wave-uniform addresses) instead of the default form, and checks that the bits are the same.  --host also evaluates the two-stage
refit with numpy on the host (window copied out with bnmf_window, then per sample C = z w, Q = y / C, w = w * (z' Q) as matrix
products; sums in BLAS's own order), the copy and the compute timed apart; the compute runs over the first --host-samples samples of
the window and is scaled to the whole window (it is linear in the samples), and the largest difference of the mean weights over
those samples' own device call is reported.  The host is the yardstick, not the code under test.  Not a test."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_decompose(e, cat, S, H, steps, min_share):
    """the window copied to the host and the two-stage KL refit in numpy float64 over its first H samples; returns (seconds: copy,
    compute; the mean weights R x N)"""
    import numpy as np
    t0 = time.perf_counter()
    P, A = e.window("P", S), e.window("A", S)
    t1 = time.perf_counter()
    z = cat / cat.sum(axis=0)[None, :]
    R = z.shape[1]
    mu = None
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(H):
            cs = P[s].sum(axis=0)
            part = (A[s].ravel() != 0) & (cs > 0)
            y = P[s][:, part] / cs[part][None, :]
            t = y.sum(axis=0)
            w = np.tile(t[None, :] / R, (R, 1))
            active = np.ones_like(w, dtype=bool)
            for stage in range(2 if min_share != 0.0 else 1):
                if stage == 1:
                    active = w >= min_share * t[None, :]
                    none = ~active.any(axis=0)
                    active[w.argmax(axis=0)[none], np.where(none)[0]] = True
                    w = np.where(active, w, 0.0)
                for _ in range(steps):
                    c = z @ w
                    w = np.where(active, w * (z.T @ np.where(c > 0.0, y / c, 0.0)), 0.0)
            a = np.zeros((R, P[s].shape[1]))
            a[:, part] = w
            mu = a if mu is None else mu + (a - mu) * (1.0 / (s + 1))
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, mu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=96)
    ap.add_argument("--G", type=int, default=10000)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--R", type=int, default=79)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--min-share", type=float, default=0.05)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--forms", action="store_true")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-samples", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import numpy as np
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    K, G, N, S = a.K, a.G, a.N, a.window
    if K == 96 and a.R == 79:
        cat = np.asfortranarray(np.load(os.path.join(ROOT, "tests", "golden", "cosmic_v3.3.1_sbs.npz"))["P"], dtype=np.float64)
    else:
        cat = np.asfortranarray(np.random.default_rng(20251019).gamma(0.4, 1.0, size=(K, a.R)))
    R = cat.shape[1]
    M, _, _ = synth_counts(K, G, min(5, N), 20251016)
    e = Engine(M, N, likelihood="poisson", prior="gamma", seed=3, window=S, device=a.device)
    apply_hyperprior_params(e, "gamma", M, N)
    e.init()
    t0 = time.perf_counter()
    e.run(S, metrics=False)
    fill_s = time.perf_counter() - t0
    n_stages = 2 if a.min_share != 0.0 else 1
    flops = 4.0 * S * N * n_stages * a.steps * K * R
    out = dict(K=K, G=G, N=N, window=S, R=R, steps=a.steps, min_share=a.min_share, calls=a.calls, fill_s=fill_s, spec_flops=flops)
    kw = dict(n_steps=a.steps, min_share=a.min_share)
    first = None
    for tag, env in (("staged", "1"), ("uniform", "0")) if a.forms else (("default", None),):
        if env is not None:
            os.environ["BNMF_DEC_STAGE"] = env
        warm = e.decompose(S, cat, **kw)                         # untimed: grows the scratch, loads the kernel
        times = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            w = e.decompose(S, cat, **kw)
            times.append(time.perf_counter() - t0)
        os.environ.pop("BNMF_DEC_STAGE", None)
        first = first or warm
        assert np.array_equal(w["weight"], first["weight"]) and np.array_equal(w["fit"], first["fit"], equal_nan=True) and np.array_equal(w["nactive"], first["nactive"])
        med = statistics.median(times)
        out.update({f"{tag}_ms_median": 1e3 * med, f"{tag}_ms_min": 1e3 * min(times), f"{tag}_ms_max": 1e3 * max(times),
                    f"{tag}_spec_TFLOPs": flops / med / 1e12})
    out.update(n_present=w["n_present"], max_rel_change=w["max_rel_change"], min_cosine=w["min_cosine"],
               nactive_mean=float(w["nactive"][w["nactive"] > 0].mean()) if (w["nactive"] > 0).any() else 0.0)
    if a.host:
        H = max(2, min(a.host_samples, S))
        tc, tn, mu = host_decompose(e, cat, S, H, a.steps, a.min_share)
        dev = e.decompose(H, cat, end_iter=e.iter - S + H, **kw)["weight_mean"]
        out.update(host_copy_s=tc, host_samples=H, host_numpy_s_measured=tn, host_numpy_s_scaled_to_window=tn * S / H,
                   host_threads=os.environ.get("OMP_NUM_THREADS"), host_max_abs_diff=float(np.max(np.abs(mu - dev))))
    e.close()
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
