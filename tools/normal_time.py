"""Iteration time of the Normal model: integer data through two builds of the library (the int32 handle of a build without
bnmf_create_f64, the fp64 handle of this one) and real-valued data through this build.

    python tools/normal_time.py all --old tools/bin/libbnmf_parent.so [--rounds 3] [--out results/normal_time.json]
    python tools/normal_time.py one --lib PATH --cfg tn-fixed|exp-rank --data int|real [--iters 1000]

`all` runs every measurement in a fresh child process of its own under `timeout -k 10` (old and new alternate, `--rounds`
times), stops at the first child that fails, and prints one JSON line per measurement and a summary (median µs per
iteration; new / old on integer data).  Configurations:
    tn-fixed   Normal-TruncNormal, fixed N = 20, K = 96, G = 5,000
    exp-rank   Normal-Exponential, rank 1:20 (N = 20, learned), K = 96, G = 1,000
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = {"tn-fixed": dict(prior="truncnormal", N=20, K=96, G=5000, learning_rank=False),
        "exp-rank": dict(prior="exponential", N=20, K=96, G=1000, learning_rank=True)}


def data(cfg, kind):
    import numpy as np
    from bayesnmf_amd.setup import synth_counts
    c = CFGS[cfg]
    if kind == "int":
        M, _, _ = synth_counts(c["K"], c["G"], 5, 20251016)
        return M
    rng = np.random.default_rng(20251016)
    P = rng.dirichlet(0.5 * np.ones(c["K"]), size=5).T
    return np.asfortranarray(P @ rng.gamma(4.0, 4.0, size=(5, c["G"])) + rng.normal(0.0, 0.3, size=(c["K"], c["G"])))


def one(lib_path, cfg, kind, iters, warmup):
    """one measurement through the C ABI alone (ctypes, no binding module: the old build lacks bnmf_create_f64)"""
    sys.path.insert(0, ROOT)
    import numpy as np
    from bayesnmf_amd.engine import BnmfConfig, LIKELIHOOD, PRIOR, IDS, NMETRIC
    from bayesnmf_amd.setup import default_hyperprior_params
    L = C.CDLL(os.path.abspath(lib_path))
    dp = C.POINTER(C.c_double)
    c = CFGS[cfg]
    M = data(cfg, kind)
    K, G, N = M.shape[0], M.shape[1], c["N"]
    conf = BnmfConfig(K, G, N, LIKELIHOOD["normal"], PRIOR[c["prior"]], 0, int(c["learning_rank"]), 0, 0, 0, 3, 0, 0, None, 0)
    h = C.c_void_p()
    if hasattr(L, "bnmf_create_f64"):
        Mx, entry = np.asfortranarray(M, dtype=np.float64), "bnmf_create_f64"
        rc = L.bnmf_create_f64(C.byref(conf), Mx.ctypes.data_as(dp), C.byref(h))
    else:                                                   # a build without it: the int32 entry point Normal data took then
        Mx, entry = np.asfortranarray(M, dtype=np.int32), "bnmf_create"
        rc = L.bnmf_create(C.byref(conf), Mx.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(h))
    L.bnmf_last_error.restype = C.c_char_p
    assert rc == 0, L.bnmf_last_error()
    for k, v in default_hyperprior_params(c["prior"], M, N).items():
        x = (C.c_double * 1)(float(v))
        assert L.bnmf_set_array(h, IDS[k[0].upper() + k[1:]], x, C.c_size_t(1)) == 0
    row = np.empty(NMETRIC)
    assert L.bnmf_init(h, row.ctypes.data_as(dp)) == 0
    rows = np.empty((max(iters, warmup), NMETRIC))
    assert L.bnmf_run(h, warmup, 0, rows.ctypes.data_as(dp)) == 0
    t0 = time.perf_counter()
    assert L.bnmf_run(h, iters, 0, rows.ctypes.data_as(dp)) == 0   # returns with the metric rows written: the device work is done
    dt = time.perf_counter() - t0
    L.bnmf_destroy(h)
    return dict(lib=os.path.basename(lib_path), entry=entry, cfg=cfg, data=kind, iters=iters, us_per_iter=1e6 * dt / iters,
                finite=bool(np.isfinite(rows[:iters, 1:5]).all()), rank_last=float(rows[iters - 1, 7]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["one", "all"])
    ap.add_argument("--lib", default=os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so"))
    ap.add_argument("--old")
    ap.add_argument("--cfg", choices=list(CFGS))
    ap.add_argument("--data", choices=["int", "real"])
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.mode == "one":
        print(json.dumps(one(a.lib, a.cfg, a.data, a.iters, a.warmup)), flush=True)
        return 0
    new = os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")
    runs = []
    for r in range(a.rounds):
        for cfg in CFGS:
            for lib, kind in ((a.old, "int"), (new, "int"), (new, "real")):
                cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "one", "--lib", lib, "--cfg", cfg,
                       "--data", kind, "--iters", str(a.iters), "--warmup", str(a.warmup)]
                p = subprocess.run(cmd, capture_output=True, text=True)
                if p.returncode != 0:                       # a failure, a fault or the time limit: nothing more is started
                    print(f"FAILED rc={p.returncode}: {' '.join(cmd)}\n{p.stdout}\n{p.stderr}", file=sys.stderr)
                    return 128 - p.returncode if p.returncode < 0 else p.returncode   # (the caller sees the abort / time-out as such)
                rec = json.loads(p.stdout.strip().splitlines()[-1])
                rec["round"] = r
                print(json.dumps(rec), flush=True)
                runs.append(rec)
    summary = {}
    for cfg in CFGS:
        med = {key: statistics.median(x["us_per_iter"] for x in runs if x["cfg"] == cfg and (x["lib"], x["data"]) == key)
               for key in ((os.path.basename(a.old), "int"), ("libbnmf.so", "int"), ("libbnmf.so", "real"))}
        summary[cfg] = dict(old_int_us=med[(os.path.basename(a.old), "int")], new_int_us=med[("libbnmf.so", "int")],
                            new_real_us=med[("libbnmf.so", "real")],
                            new_over_old_int=med[("libbnmf.so", "int")] / med[(os.path.basename(a.old), "int")])
    print(json.dumps(dict(summary=summary)), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(runs=runs, summary=summary), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
