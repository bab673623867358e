"""Label-switching correction of a recorded range, the parts that need no GPU: the numpy restatement of the spec (tests/relabel_ref.py)
on planted permutations, its assignment step against scipy's, an unmatched sample, the stopping rule, bayesNMF_sampler.get_relabelling
over a stub engine, and the two new symbols."""
import os
import re
import subprocess

import numpy as np
import pytest

import relabel_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _stable(S=9, K=12, G=5, N=4, seed=3):
    """a series whose factors are far apart and keep their labels: fixed signatures and exposures, jittered per sample"""
    rng = np.random.default_rng(seed)
    P0 = rng.dirichlet(np.full(K, 0.3), size=N).T
    E0 = rng.gamma(4.0, 50.0, size=(N, G))
    return P0[None] * rng.uniform(0.9, 1.1, size=(S, K, N)), E0[None] * rng.uniform(0.9, 1.1, size=(S, N, G))


def _planted(seed=5):
    Pw, Ew = _stable()
    S, K, N = Pw.shape
    rng = np.random.default_rng(seed)
    perms = np.stack([np.arange(N)] + [rng.permutation(N) for _ in range(S - 1)])          # perms[s][j]: where label j of sample s went
    Pp, Ep = np.empty_like(Pw), np.empty_like(Ew)
    for s in range(S):
        Pp[s][:, perms[s]] = Pw[s]
        Ep[s][perms[s], :] = Ew[s]
    return Pw, Ew, Pp, Ep, perms


def test_planted_permutations_are_recovered_and_the_moments_are_the_unpermuted_series():
    Pw, Ew, Pp, Ep, perms = _planted()
    S, K, N = Pw.shape
    assert (perms != np.arange(N)).any(axis=1).sum() >= 6
    r = R.relabel_reference(Pp, Ep, pivot=Pw[0])
    inv = np.argsort(perms, axis=1)                            # factor n of the permuted sample s carries label inv[s][n]
    assert np.array_equal(r["perm"], inv)
    assert r["n_aligned"] == S and r["n_unmatched"] == 0 and r["converged"] == 1 and r["n_switched"] == int((inv != np.arange(N)).any(axis=1).sum())
    straight = R.relabel_reference(Pw, Ew, pivot=Pw[0])
    assert straight["n_switched"] == 0 and straight["rounds"] == 1
    for k in ("P_mean", "P_var", "E_mean", "E_var", "aligned_P", "aligned_E"):
        assert np.array_equal(_bits(r[k]), _bits(straight[k])), k
    # ... which are mixing's moments of the renormalised series
    import mixing_ref
    xP, xE = mixing_ref.renormalised_series(Pw, Ew)
    mP, mE = mixing_ref.mixing_reference(xP), mixing_ref.mixing_reference(xE)
    assert np.array_equal(_bits(r["P_mean"].ravel(order="F")), _bits(mP["mean"])) and np.array_equal(_bits(r["P_var"].ravel(order="F")), _bits(mP["var"]))
    assert np.array_equal(_bits(r["E_mean"].ravel(order="F")), _bits(mE["mean"])) and np.array_equal(_bits(r["E_var"].ravel(order="F")), _bits(mE["var"]))
    assert (r["confusion"].sum(axis=0) == S).all() and (r["confusion"].sum(axis=1) == S).all()
    assert r["min_cosine"] == np.min(r["cosine"]) and r["cosine"].ravel()[r["min_cosine_at"]] == r["min_cosine"]
    assert abs(r["mean_cosine"] - r["cosine"].mean()) < 1e-14
    # the NULL pivot is the newest sample: the labels are then that sample's
    last = R.relabel_reference(Pp, Ep)
    assert np.array_equal(last["perm"], perms[-1][inv])


def test_the_assignment_is_optimal_and_the_two_forms_agree():
    from scipy.optimize import linear_sum_assignment
    Pw, Ew, Pp, Ep, perms = _planted()
    rng = np.random.default_rng(1)
    mats = [R.cosine_matrix(Pp[s], Pw[0]) for s in range(Pp.shape[0])]
    mats += [rng.uniform(0, 1, size=(n, n)) for n in (2, 5, 17, 70)]
    mats += [np.round(rng.uniform(0, 1, size=(9, 9)), 1), np.ones((6, 6)), np.eye(5)]       # ties
    for C in mats:
        pm, ps = R.hungarian(C), R.hungarian_scalar(C)
        assert np.array_equal(pm, ps)                          # the same algorithm, the same tie rule
        n = C.shape[0]
        assert sorted(pm) == list(range(n))
        rows, cols = linear_sum_assignment(-C)
        best, got = C[rows, cols].sum(), C[np.arange(n), pm].sum()
        assert abs(got - best) <= 1e-12 * abs(best), (got, best)
    assert np.array_equal(R.hungarian(np.ones((6, 6))), np.arange(6))     # all equal: the lowest column for every row in turn
    # the wave form's first cosine: explicit loops
    C = R.cosine_matrix(Pp[3], Pw[0])
    p, q = Pp[3][:, 1], Pw[0][:, 2]
    dot = nn = rn = 0.0
    for k in range(len(p)):
        dot = dot + p[k] * q[k]; nn = nn + p[k] * p[k]; rn = rn + q[k] * q[k]
    assert C[1, 2] == dot / np.sqrt(nn * rn)


def test_an_unmatched_sample_leaves_the_sums():
    Pw, Ew, Pp, Ep, perms = _planted()
    S, K, N = Pw.shape
    Pz = Pp.copy()
    Pz[4][:, 2] = 0.0                                          # a zero column: its cosines are 0 / 0
    assert R.hungarian(R.cosine_matrix(Pz[4], Pw[0])) is None and R.hungarian_scalar(R.cosine_matrix(Pz[4], Pw[0])) is None
    r = R.relabel_reference(Pz, Ep, pivot=Pw[0])
    keep = [s for s in range(S) if s != 4]
    w = R.relabel_reference(Pp[keep], Ep[keep], pivot=Pw[0])
    assert r["n_unmatched"] == 1 and r["n_aligned"] == S - 1 and r["n_used"] == S
    assert (r["perm"][4] == -1).all() and np.isnan(r["cosine"][4]).all() and np.isnan(r["aligned_P"][4]).all() and np.isnan(r["aligned_E"][4]).all()
    for k in ("P_mean", "P_var", "E_mean", "E_var", "mean_cosine", "min_cosine"):
        assert np.array_equal(_bits(r[k]), _bits(w[k])), k
    assert np.array_equal(r["perm"][keep], w["perm"]) and np.array_equal(r["confusion"], w["confusion"])
    assert (r["confusion"].sum(axis=0) == S - 1).all() and (r["confusion"].sum(axis=1) == S - 1).all()
    s_w, n_w = divmod(w["min_cosine_at"], N)
    assert r["min_cosine_at"] == keep[s_w] * N + n_w           # the index counts used samples, aligned or not
    with pytest.raises(ValueError, match="aligned samples"):
        Pz[:-1, :, 0] = 0.0
        R.relabel_reference(Pz, Ep, pivot=Pw[0])


def test_the_stopping_rule():
    Pw, Ew, Pp, Ep, perms = _planted()
    one = R.relabel_reference(Pp, Ep, pivot=Pw[0], max_rounds=1)
    assert one["rounds"] == 1 and one["converged"] == 0 and one["n_changed_last"] == one["n_switched"] > 0
    full = R.relabel_reference(Pp, Ep, pivot=Pw[0], max_rounds=10)
    assert full["rounds"] == 2 and full["converged"] == 1 and full["n_changed_last"] == 0 and np.array_equal(full["history"][0], one["perm"])
    same = R.relabel_reference(Pw, Ew, pivot=Pw[0], max_rounds=1)       # nothing to move: round 1 already converges
    assert same["rounds"] == 1 and same["converged"] == 1 and same["n_changed_last"] == 0
    # a pivot far from every sample needs a second round that moves labels: two near-copies of one signature, told apart only by the mean
    rng = np.random.default_rng(0)
    S, K, N, G = 11, 10, 3, 4
    base = rng.dirichlet(np.full(K, 0.3), size=N).T
    base[:, 1] = base[:, 0] * rng.uniform(0.8, 1.25, size=K)
    Pq = base[None] * rng.uniform(0.7, 1.4, size=(S, K, N))
    Eq = rng.gamma(2.0, 10.0, size=(S, N, G))
    piv = base.copy()
    piv[:, [0, 1]] = rng.dirichlet(np.full(K, 0.3), size=2).T * 0.2 + base[:, [1, 0]] * 0.01
    r = R.relabel_reference(Pq, Eq, pivot=piv, max_rounds=10)
    print("samples changed per round", [int((b != a).any(axis=1).sum()) for a, b in zip([np.tile(np.arange(N), (S, 1))] + r["history"], r["history"])])
    assert r["rounds"] == 3 and r["converged"] == 1 and len(r["history"]) == 3 and (r["history"][1] != r["history"][0]).any()
    capped = R.relabel_reference(Pq, Eq, pivot=piv, max_rounds=2)
    assert capped["converged"] == 0 and capped["rounds"] == 2 and capped["n_changed_last"] == 1 and np.array_equal(capped["perm"], r["history"][1])


def test_get_relabelling_ranges_pivots_and_result(tmp_path):
    """bayesNMF_sampler.get_relabelling over a stub engine: the range and idx rules of get_WAIC (_recorded_range), the pivots, the result"""
    from test_waic_host import _NoWaicEngine
    from bayesnmf_amd.sampler import bayesNMF_sampler
    from bayesnmf_amd.convergence import new_convergence_control
    from bayesnmf_amd.setup import synth_counts

    class _RelEngine(_NoWaicEngine):
        calls = []

        def get(self, name):
            return super().get(name) * 7.0

        def relabel(self, last_n, used=None, end_iter=None, pivot_P=None, max_rounds=10, aligned=False):
            type(self).calls.append(dict(last_n=last_n, used=None if used is None else np.array(used), end_iter=end_iter,
                                         pivot_P=None if pivot_P is None else np.array(pivot_P), max_rounds=max_rounds, aligned=aligned))
            S = last_n if used is None else int(np.sum(used))
            K, G, N = self.K, self.G, self.N
            out = dict(n_used=S, n_aligned=S, n_unmatched=0, rounds=2, converged=1, n_switched=1, n_changed_last=0, mean_cosine=0.9, min_cosine=0.5,
                       min_cosine_at=3, perm=np.tile(np.arange(N, dtype=np.int32), (S, 1)), cosine=np.ones((S, N)), confusion=np.eye(N, dtype=np.int64) * S,
                       P_mean=np.arange(K * N, dtype=float).reshape(K, N), P_var=np.ones((K, N)), E_mean=np.arange(N * G, dtype=float).reshape(N, G),
                       E_var=np.ones((N, G)))
            if aligned:
                out.update(aligned_P=np.ones((S, K, N)), aligned_E=np.ones((S, N, G)))
            return out

    M, _, _ = synth_counts(12, 9, 2, 3, mean_total=200)
    cc = new_convergence_control()
    cc.update(MAP_over=4, MAP_every=2, maxiters=10, miniters=2)
    s = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "r"), engine_factory=_RelEngine,
                         convergence_control=cc, save_all_samples=True, periodic_save=False)
    s.run_gibbs_sampler()
    logs = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path / "r")) for f in fs if f.endswith((".log", ".txt"))]
    assert logs and any("Relabelling over 4 samples: 2 rounds | 1 samples switched | 0 unmatched | smallest cosine 0.5000" in open(f).read() for f in logs)
    c = _RelEngine.calls[-1]                                   # the call behind the log line of the run: the defaults
    assert c["last_n"] == 4 and c["end_iter"] is None and c["max_rounds"] == 10 and not c["aligned"] and np.array_equal(c["used"], [1, 1, 1, 1])
    assert c["pivot_P"].shape == (12, 3) and np.array_equal(c["pivot_P"], np.asarray(s.MAP["P"]))      # pivot = "MAP": every factor kept
    r = s.get_relabelling()
    assert r["rounds"] == 2 and r["n_switched"] == 1 and r["P"].shape == (12, 3) and r["E"].shape == (3, 9) and list(r["keep_sigs"]) == [0, 1, 2]
    # a MAP that dropped factor 1: its column of the pivot comes from the last sample, P / E keep the others
    s.MAP.update(P=np.asarray(s.MAP["P"])[:, [0, 2]] * 3.0, keep_sigs=np.array([0, 2]))
    r = s.get_relabelling(end_iter=8, n_samples=5, idx=[4, 6, 8], max_rounds=3, aligned=True)
    c = _RelEngine.calls[-1]
    assert c["end_iter"] == 8 and c["last_n"] == 5 and np.array_equal(c["used"], [1, 0, 1, 0, 1]) and c["aligned"] and c["max_rounds"] == 3
    assert (c["pivot_P"][:, 1] == 7.0).all() and (c["pivot_P"][:, [0, 2]] == 3.0).all()
    assert np.array_equal(r["P"], r["P_mean"][:, [0, 2]]) and np.array_equal(r["E"], r["E_mean"][[0, 2], :]) and r["aligned_P"].shape == (3, 12, 3)
    s.get_relabelling(end_iter=8, n_samples=5, idx=None, pivot="last")
    assert _RelEngine.calls[-1]["used"] is None and _RelEngine.calls[-1]["pivot_P"] is None
    given = np.full((12, 3), 2.0)
    s.get_relabelling(pivot=given)
    assert np.array_equal(_RelEngine.calls[-1]["pivot_P"], given)
    with pytest.raises(ValueError, match="pivot is"):
        s.get_relabelling(pivot=np.ones((12, 4)))
    with pytest.raises(ValueError, match="must be 'MAP', 'last'"):
        s.get_relabelling(pivot="first")
    with pytest.raises(ValueError, match="not all recorded"):
        s.get_relabelling(end_iter=12, n_samples=3)
    with pytest.raises(ValueError, match="idx must lie in"):
        s.get_relabelling(end_iter=8, n_samples=3, idx=[2])
    s.close()
    t = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "one"), engine_factory=_NoWaicEngine)
    with pytest.raises(ValueError, match="get_relabelling needs an engine"):
        t.get_relabelling()
    t.close()


def test_new_symbols_declared_exported_and_bound():
    import ctypes as C
    from bayesnmf_amd import engine
    hdr = open(os.path.join(ROOT, "include", "bnmf.h")).read()
    assert re.search(r"#define BNMF_NREL 2\b", hdr) and "} bnmf_relabel_info;" in hdr
    for sym in ("bnmf_relabel", "bnmf_relabel_at"):
        assert re.search(r"\bint\s+%s\s*\(\s*bnmf_handle\s*\*" % sym, hdr), f"{sym} not declared in include/bnmf.h"
        assert sym in engine.ABI_SYMBOLS
    so = os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    L = engine.lib()
    for sym, nargs in (("bnmf_relabel", 13), ("bnmf_relabel_at", 14)):
        assert re.search(r"\bT %s$" % sym, exported, re.M), f"{sym} not exported by libbnmf.so"
        assert len(getattr(L, sym).argtypes) == nargs
    assert C.sizeof(engine.BnmfRelabelInfo) == 56
    assert hasattr(engine.Engine, "relabel")
