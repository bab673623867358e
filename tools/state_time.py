"""Cost of saving and loading a chain's state (bnmf_save_state / bnmf_load_state) at the headline shape: Poisson-Gamma, K = 96,
G = 10,000, N = 20, window (MAP_over) 1,000.

    python tools/state_time.py [--dir /tmp/bnmf_state] [--iters 1100]

Runs `--iters` iterations (more than the window: every ring slot is a kept sample), then reports as one JSON line: bytes and time of a
full save and of a load into a fresh handle (with a check that it continues bit for bit), and bytes and time of one periodic delta of
MAP_every = 100 iterations against those 100 iterations' own time.  The bench.py headline is measured by bench.py itself, before and
after.  Times are wall-clock, the file on local disk (page cache warm for the load).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/tmp/bnmf_state")
    ap.add_argument("--iters", type=int, default=1100)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    K, G, N, W = 96, 10000, 20, 1000
    M, _, _ = synth_counts(K, G, 5, 20251016)
    os.makedirs(a.dir, exist_ok=True)
    path = os.path.join(a.dir, "engine_state.bin")

    def engine():
        e = Engine(M, N, prior="gamma", seed=1, window=W, device=a.device)
        apply_hyperprior_params(e, "gamma", M, N)
        return e
    e = engine()
    e.init()
    e.run(a.iters - 1, metrics=False)
    t = time.perf_counter(); full = e.save_state(path); t_full = time.perf_counter() - t
    t = time.perf_counter(); e.run(100, metrics=False); t_run = time.perf_counter() - t
    t = time.perf_counter(); delta = e.save_state(path, since_iter=a.iters); t_delta = time.perf_counter() - t
    b = Engine(M, N, prior="gamma", seed=1, window=W, device=a.device)
    t = time.perf_counter(); it = b.load_state(path); t_load = time.perf_counter() - t
    same = it == e.iter and np.array_equal(b.run(20).view(np.uint64), e.run(20).view(np.uint64))
    out = dict(shape=dict(K=K, G=G, N=N, window=W), iters=int(it), full_bytes=full, full_s=round(t_full, 4),
               full_GBs=round(full / t_full / 1e9, 3), file_bytes=os.path.getsize(path), load_s=round(t_load, 4),
               load_GBs=round(os.path.getsize(path) / t_load / 1e9, 3), delta_bytes=delta, delta_s=round(t_delta, 4),
               run100_s=round(t_run, 4), delta_over_run100=round(t_delta / t_run, 3), continues_bit_identical=bool(same))
    print(json.dumps(out))
    e.close(); b.close()
    os.remove(path)


if __name__ == "__main__":
    main()
