"""bayesNMF(M, rank = 1:6, likelihood = "normal") on real-valued data M = P E + N(0, sd^2), E ~ Gamma(4, e_scale) (the data of
tests/test_gpu_real_data.py::test_bayesNMF_on_real_data): for each engine seed the learned rank, the cosines of the MAP signatures
assigned to the three true ones (Hungarian assignment) and the wall time.  One JSON line per seed.  Where the test's cosine
threshold and what it asserts about the rank come from.

    python tools/normal_real_e2e.py [--e-scale 40 --sd 1.5] [--seeds 1 2 3 4 5] [--out results/normal_real_e2e.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    from scipy.optimize import linear_sum_assignment
    from bayesnmf_amd.sampler import bayesNMF
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3, 4, 5])
    ap.add_argument("--e-scale", type=float, default=4.0, help="E ~ Gamma(4, e_scale): mean of P E = 3 * 4 * e_scale / 96")
    ap.add_argument("--sd", type=float, default=0.3, help="noise standard deviation")
    ap.add_argument("--prior", default="truncnormal")
    ap.add_argument("--data-seed", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = np.random.default_rng(a.data_seed)               # = tests/test_gpu_real_data.py _real_data(96, 200, 3, seed, sd, e_scale)
    K, G, R = 96, 200, 3
    Pt = rng.dirichlet(0.5 * np.ones(K), size=R).T
    E = rng.gamma(4.0, a.e_scale, size=(R, G))
    M = np.asfortranarray(Pt @ E + rng.normal(0.0, a.sd, size=(K, G)))
    data = dict(e_scale=a.e_scale, sd=a.sd, prior=a.prior, data_seed=a.data_seed, p99=float(np.percentile(M, 99)), neg=float((M < 0).mean()),
                floor0=float((np.floor(M) == 0).mean()))
    out = []
    for seed in a.seeds:
        with tempfile.TemporaryDirectory() as d:
            t0 = time.perf_counter()
            s = bayesNMF(M, rank=np.arange(1, 7), likelihood="normal", prior=a.prior, output_dir=os.path.join(d, "n"), periodic_save=False,
                         seed=seed)
            dt = time.perf_counter() - t0
            P = np.asarray(s.MAP["P"])
            cos = (P / np.linalg.norm(P, axis=0)).T @ (Pt / np.linalg.norm(Pt, axis=0))
            r, c = linear_sum_assignment(-cos)
            sm = s.state["sample_metrics"]
            rec = dict(data, seed=seed, learned_rank=int(P.shape[1]), assigned_cosines=[float(x) for x in cos[r, c]], iters=int(s.state["iter"]),
                       finite=bool(np.isfinite(sm[["RMSE", "KL", "loglikelihood", "logposterior"]].to_numpy()).all()), seconds=dt)
            s.close()
        print(json.dumps(rec), flush=True)
        out.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
