"""The chains of tests/test_map_host.py (on the CPU oracle), tests/test_gpu_map_bits.py and tests/test_gpu_assign_bits.py (on the
device): the same data, seeds and calls on both, so that what the oracle rehearsal shows holds for the device's rings, which are the
oracle's bits.  Test infrastructure only."""
import numpy as np

from test_gpu_attribution import CASES as _ATTR, USED, _temps as temps   # noqa: F401  (the rehearsed chains of the newer posterior tests)

W, T_END, N_RANGE = 16, 40, 12

# name: K, G, N, likelihood, prior, MH, learning_rank, seed
CASES = dict(_ATTR)
CASES.update({
    "n1": (5, 3, 1, "poisson", "gamma", False, False, 4),                  # one factor
    "k7": (7, 3, 3, "poisson", "gamma", False, False, 4),                  # K N = 21, N G = 9: neither a multiple of 8
    "n70": (5, 3, 70, "poisson", "gamma", False, False, 4),                # the assignment: more columns than lanes
    "rank_n3": (12, 8, 3, "poisson", "gamma", False, True, 3),            # rank learning: A patterns that repeat inside the range
    "fix1": (8, 7, 3, "poisson", "gamma", False, False, 4),                # ties (a): column 1 of P fixed
    "fixall_mh": (8, 7, 3, "poisson", "truncnormal", True, False, 4),      # ties (b): every column fixed, converged = True
})
FIXED = {"fix1": [0, 1, 0], "fixall_mh": [1, 1, 1]}
MAP_CASES = [c for c in CASES if c != "n70"]
ROUTE = (5, 3, 2, "poisson", "gamma", False, False, 4)                     # the route chain: window 2,100, run to iteration 2,150
ROUTE_W, ROUTE_END = 2100, 2150


def data(case):
    from bayesnmf_amd.setup import synth_counts
    K, G, N, lk, *_ = ROUTE if case == "route" else CASES[case]
    if lk == "normal":
        rng = np.random.default_rng(11)
        return np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, 3)) @ rng.gamma(0.5, 1.0, size=(3, G)) + rng.normal(0.0, 0.5, size=(K, G)))   # small means: some cells below 0
    return synth_counts(K, G, min(3, N), 21, mean_total=1500)[0]


def initial_P(case, M):
    """the P both chains of a case with fixed columns start from"""
    K, G, N, *_ = CASES[case]
    return np.asfortranarray(np.random.default_rng(17).dirichlet(np.ones(K), size=N).T * (0.1 * np.sqrt(np.mean(M) * K / N)))


def create(cls, case, **kw):
    """the case's chain on cls (Engine, or oracle.Oracle: the same bits), before init"""
    from bayesnmf_amd.setup import apply_hyperprior_params
    K, G, N, lk, prior, MH, lr, seed = ROUTE if case == "route" else CASES[case]
    M = data(case)
    c = cls(M, N, likelihood=lk, prior=prior, MH=MH, learning_rank=lr, seed=seed, temperature=temps() if lr else None, **kw)
    apply_hyperprior_params(c, prior, M, N)
    if case in FIXED:
        c.set("P", initial_P(case, M))
        if hasattr(c, "set_fixed"):
            c.set_fixed("P", FIXED[case])
    return c, M


def oracle_samples(case, t_end=T_END):
    """P [t_end][K][N], E [t_end][N][G], A [t_end][N] of iterations 1 .. t_end on the CPU oracle, one run(1) at a time; a case with fixed
    columns is composed from the oracle's conditionals as tests/test_gpu_fixed.py composes it (no P step, or the fixed columns restored
    after it)"""
    import oracle as O
    K, G, N, lk, prior, MH, lr, seed = ROUTE if case == "route" else CASES[case]
    o, M = create(O.Oracle, case)
    o.init()
    P, E, A = [o.get("P").copy()], [o.get("E").copy()], [o.get("A").ravel().copy()]
    mask = np.asarray(FIXED.get(case, []), dtype=bool)
    P0 = initial_P(case, M) if case in FIXED else None
    for t in range(2, t_end + 1):
        if case not in FIXED:
            o.run(1, converged=MH)
        else:
            for what in ["hyper"] + ([] if mask.all() else ["P"]) + ["E"] + ([] if MH else ["Z"]):
                o.step(what, t, converged=MH)
                if what == "P":
                    Pt = o.get("P"); Pt[:, mask] = P0[:, mask]; o.set("P", Pt)
        P.append(o.get("P").copy()); E.append(o.get("E").copy()); A.append(o.get("A").ravel().copy())
    o.close()
    return np.stack(P), np.stack(E), np.stack(A), M


def catalogue(K, R, seed=3):
    """a reference catalogue of R columns"""
    return np.asfortranarray(np.random.default_rng(seed).dirichlet(np.full(K, 0.5), size=R).T)


def tied_catalogue(P):
    """From a sample's P (K x 3): its columns 0 and 1, column 1 again, twice column 0 (its cosines are column 0's bits: the scaling by
    2 is exact), column 2.  Every factor has its own best reference, so each row of the solver augments in one step, the potentials of
    the columns stay 0 and the reduced costs of the tied columns are equal: the tie rule decides, and columns 2 and 3 must get no vote"""
    P = np.asarray(P, dtype=np.float64)
    return np.asfortranarray(np.stack([P[:, 0], P[:, 1], P[:, 1], 2.0 * P[:, 0], P[:, 2]], axis=1))


def keep_mask(N):
    """a keep mask with a gap"""
    k = np.ones(N, dtype=np.int32)
    k[1::4] = 0
    return k if N > 1 else np.ones(1, dtype=np.int32)


def repeated_values(e_series):
    """e_series [S][L]: per element the largest number of samples that hold one value -> (share of elements with a repeat, the maximum)"""
    S, L = e_series.shape
    mult = np.array([np.unique(e_series[:, i], return_counts=True)[1].max() for i in range(L)])
    return float((mult >= 2).mean()), int(mult.max())
