"""What holding columns of P fixed (bnmf_set_fixed) does to the iteration rate: iterations/s at the headline shape (K = 96, G = 10,000,
N = 20) and at G = 2,000, with none, half and all of the columns fixed.  One process per measurement (its rate: the median of three timed blocks of 1,500 iterations), the three variants taken in turn and the
whole round repeated (alternation: a drift of the box hits every variant alike); the median and the spread over the processes are printed.
Usage: python tools/refit_time.py [rounds (default 3)] [G ...]"""
import os, sys, subprocess
code = '''
import sys, time
import numpy as np
sys.path.insert(0, ".")
from bayesnmf_amd import Engine
from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
G, F, N = int(sys.argv[1]), int(sys.argv[2]), 20
M, P, _ = synth_counts(96, G, 8, 20250218)
e = Engine(M, N, prior="gamma", seed=1, window=1000); apply_hyperprior_params(e, "gamma", M, N)
if F:
    P0 = np.full((96, N), np.nan); P0[:, :F] = np.random.default_rng(1).dirichlet(0.1 * np.ones(96), size=F).T
    e.set("P", P0); e.set_fixed("P", (np.arange(N) < F).astype(np.int32))
e.init(); e.run(300, metrics=False)
ts = []
for _ in range(3):
    t0 = time.perf_counter(); e.run(1500, metrics=True); ts.append(1500 / (time.perf_counter() - t0))
print(sorted(ts)[1])
'''
args = sys.argv[1:]
rounds = int(args[0]) if args else 3
res = {}
for G in [int(g) for g in args[1:]] or [10000, 2000]:
    for _ in range(rounds):
        for F in (0, 10, 20):
            out = subprocess.run([sys.executable, "-c", code, str(G), str(F)], check=True, capture_output=True, text=True, timeout=300).stdout
            res.setdefault((G, F), []).append(float(out.strip().splitlines()[-1]))
    for F in (0, 10, 20):
        v = sorted(res[(G, F)])
        print("G=%6d fixed %2d of 20: median %8.0f it/s  (min %.0f, max %.0f; %d runs)" % (G, F, v[len(v) // 2], v[0], v[-1], len(v)), flush=True)
