"""Exposures of new tumours under recorded signatures, the parts that need no GPU: the numpy restatement of the spec
(tests/project_ref.py) against the laws of the KL multiplicative update, bayesNMF_sampler.get_projection over a stub
engine, and the two new symbols."""
import os
import re
import subprocess

import numpy as np
import pytest

import project_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps           # 2^-52: twice the unit roundoff u


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _problem(S, K, N, J, seed):
    rng = np.random.default_rng(seed)
    P = rng.gamma(0.7, 1.0, size=(S, K, N))
    A = np.ones((S, N))
    X = rng.poisson(rng.gamma(2.0, 20.0, size=(K, J))).astype(np.float64)
    return P, A, X


def test_disjoint_supports_are_solved_in_one_step():
    """Signatures of disjoint support and X = x e_true: one step returns e_true.  For k in the support of n the sum c has one term,
    c = fl(x e0), X = fl(x e_true) and q = fl(X / c): 3 roundings; g_n adds at most K products (1 rounding each) in at most K
    additions, and sum_k x[k,n] is 1 within the K + 1 roundings of the column sum and the division; e0 * g is one more.  That is at
    most 2 K + 8 relative errors of u = 2^-53 each; the bound allows twice that for the second-order terms."""
    S, K, N, J = 3, 30, 4, 5
    rng = np.random.default_rng(1)
    P = np.zeros((S, K, N))
    for n in range(N):
        rows = np.arange(n, K, N)                                # rows n, n + N, ...: disjoint
        P[:, rows, n] = rng.gamma(2.0, 1.0, size=(S, len(rows)))
    x, part = R.renormalise(P, np.ones((S, N)))
    assert part.all()
    e_true = rng.gamma(2.0, 50.0, size=(N, J))
    worst = 0.0
    for s in range(S):
        e, _ = R.refit(x[s:s + 1], part[s:s + 1], x[s] @ e_true, 1)
        worst = max(worst, float(np.max(np.abs(e[0] - e_true) / e_true)))
    bound = (2 * K + 8) * EPS
    print(f"largest relative error after one step {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound


def test_the_exposures_keep_the_total_of_the_tumour():
    """sum_n e_n g_n = sum_k (X_k / c_k) sum_n x[k,n] e_n = sum_k X_k in exact arithmetic, whatever e was.  Per step the relative error
    of the sum is at most N + 1 roundings in c, 1 in q, 1 in x q, K in g and 1 in e g: K + N + 4; over the steps, and with the N
    additions of the check itself, (steps (K + N + 4) + N) u.  The bound allows twice that."""
    S, K, N, J, steps = 4, 40, 6, 9, 30
    P, A, X = _problem(S, K, N, J, 3)
    X[:, 2] = 0.0                                                # an all-zero tumour: e = 0 throughout
    x, part = R.renormalise(P, A)
    tr = []
    R.refit(x, part, X, steps, trace=tr)
    t = X.sum(axis=0)
    for i, e in enumerate(tr):
        tot = np.zeros((S, J))
        for n in range(N):
            tot = tot + e[:, n, :]
        bound = ((i + 1) * (K + N + 4) + N) * EPS * t
        assert (np.abs(tot - t[None, :]) <= bound[None, :]).all(), i
    assert (tr[-1][:, :, 2] == 0).all()


def test_the_poisson_loglikelihood_never_decreases():
    """EM: L(e) = sum_k X_k log c_k - c_k does not decrease.  In float64 L carries the roundings of c (N + 1), of the logarithm and the
    product (2) and of the K additions, relative to the sum of the magnitudes of its terms: a decrease of up to
    2 (K + N + 3) u sum_k (|X_k log c_k| + c_k) per evaluated pair is rounding."""
    S, K, N, J, steps = 3, 25, 5, 8, 40
    P, A, X = _problem(S, K, N, J, 5)
    x, part = R.renormalise(P, A)
    tr = []
    R.refit(x, part, X, steps, trace=tr)

    def loglik(e):
        c = R.fitted(x, part, e)
        with np.errstate(all="ignore"):
            term = np.where(X[None] > 0, X[None] * np.log(c), 0.0)
        return (term - c).sum(axis=1), (np.abs(term) + c).sum(axis=1)
    prev, _ = loglik(tr[0])
    rose = 0
    for e in tr[1:]:
        cur, mag = loglik(e)
        tol = 2 * (K + N + 3) * EPS * mag
        assert (cur >= prev - tol).all()
        rose += int((cur > prev).sum())
        prev = cur
    assert rose > 0


def test_an_excluded_factor_has_exposure_zero_and_is_as_if_deleted():
    S, K, N, J, steps = 4, 20, 5, 6, 12
    P, A, X = _problem(S, K, N, J, 7)
    A[:, 1] = 0.0                                                # excluded by A in every sample
    P[:, :, 3] = 0.0                                             # a zero column: colsum 0, x = 0 / 0
    P[2, 4, 1] = np.inf                                          # a value in an excluded column that must not reach c
    x, part = R.renormalise(P, A)
    assert not part[:, 1].any() and not part[:, 3].any() and part[:, [0, 2, 4]].all()
    e, ch = R.refit(x, part, X, steps)
    for n in (1, 3):
        assert np.array_equal(_bits(e[:, n, :]), _bits(np.zeros((S, J)))), n          # +0.0, not -0.0
    assert np.isfinite(e).all() and np.isfinite(ch).all()
    keep = [0, 2, 4]
    x2, part2 = R.renormalise(P[:, :, keep], A[:, keep])
    e2, ch2 = R.refit(x2, part2, X, steps)
    assert np.array_equal(_bits(e[:, keep, :]), _bits(e2)) and np.array_equal(_bits(ch), _bits(ch2))
    # a sample without factors: every exposure 0, the change 0
    A[1, :] = 0.0
    x, part = R.renormalise(P, A)
    e, ch = R.refit(x, part, X, steps)
    assert (e[1] == 0).all() and (ch[1] == 0).all()


def test_the_whole_restatement_on_a_planted_case(oracle_lib):
    rng = np.random.default_rng(9)
    K, N, S, J = 24, 3, 8, 7
    P0 = rng.dirichlet(np.full(K, 0.3), size=N).T
    E0 = rng.gamma(4.0, 200.0, size=(N, J))
    E0[2, 0] = 0.0
    X = rng.poisson(P0 @ E0).astype(np.float64)
    X[:, 5] = 0.0                                                # an all-zero tumour: cosine NaN
    X[:, 6] = X[:, 1]                                            # a repeated tumour
    Ps = P0[None] * rng.uniform(0.97, 1.03, size=(S, K, N)) * rng.uniform(0.5, 2.0, size=(S, 1, N))   # scaled columns: renormalised away
    r = R.project_reference(Ps, np.ones((S, N)), X, 300, min_load=1.0)
    print("exposure_mean\n", r["load_mean"].round(1), "\nE0\n", E0.round(1), "\nfit\n", r["fit"])
    ok = [0, 1, 2, 3, 4, 6]
    E0[:, 6] = E0[:, 1]
    assert np.allclose(r["load_mean"][:, ok], E0[:, ok], rtol=0.25, atol=60.0)
    assert np.isnan(r["cosine"][5]) and (r["cosine"][ok] > 0.97).all() and r["rel_l1"][5] == 0.0 and r["rel_change"][5] == 0.0
    assert (r["load"][:, :, 5] == 0).all()
    assert np.array_equal(_bits(r["load"][:, :, 6]), _bits(r["load"][:, :, 1])) and np.array_equal(_bits(r["fit"][:, 6]), _bits(r["fit"][:, 1]))
    assert r["min_cosine_at"] == int(np.nanargmin(r["cosine"])) and r["min_cosine"] == np.nanmin(r["cosine"])
    assert r["max_rel_change"] == r["rel_change"].max() and r["max_rel_change"] < 1e-3
    assert np.allclose(r["load_mean"], r["exposures"].mean(axis=0), rtol=1e-13, atol=1e-300)
    assert np.allclose(r["load_var"], r["exposures"].var(axis=0, ddof=1), rtol=1e-9, atol=1e-300)
    assert abs(r["total"] - X.sum()) <= 1e-9 * X.sum()
    assert r["n_used"] == S and r["n_steps"] == 300 and r["series"].shape == (S, N)


def test_get_projection_ranges_idx_and_result(tmp_path):
    """bayesNMF_sampler.get_projection over a stub engine: the range and idx rules of get_WAIC (_recorded_range), the shape of the result"""
    from test_waic_host import _NoWaicEngine
    from bayesnmf_amd.sampler import bayesNMF_sampler
    from bayesnmf_amd.convergence import new_convergence_control
    from bayesnmf_amd.setup import synth_counts

    class _ProjEngine(_NoWaicEngine):
        calls = []

        def project(self, last_n, X, used=None, end_iter=None, n_steps=200, min_load=1.0, exposures=False):
            type(self).calls.append(dict(last_n=last_n, X=np.array(X), used=None if used is None else np.array(used), end_iter=end_iter,
                                         n_steps=n_steps, min_load=min_load, exposures=exposures))
            S = last_n if used is None else int(np.sum(used))
            N, J = self.N, np.shape(X)[1]
            ex = np.arange(S, dtype=float)[:, None, None] + np.zeros((S, N, J))
            return dict(n_used=S, n_steps=n_steps, n_present=5, min_load=min_load, total=123.0, max_rel_change=1e-4, min_cosine=0.9,
                        min_cosine_at=2, series=np.zeros((S, N)), load_mean=np.full((N, J), 2.0), load_var=np.full((N, J), 9.0),
                        share=np.full((N, J), 1.0 / N), p_present=np.full((N, J), 0.75), cosine=np.full(J, 0.95), rel_l1=np.full(J, 0.1),
                        rel_change=np.full(J, 1e-4), exposures=ex)

    M, _, _ = synth_counts(12, 9, 2, 3, mean_total=200)
    new = M[:, :4] + 1
    cc = new_convergence_control()
    cc.update(MAP_over=4, MAP_every=2, maxiters=10, miniters=2)
    s = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "r"), engine_factory=_ProjEngine,
                         convergence_control=cc, save_all_samples=True, periodic_save=False)
    s.run_gibbs_sampler()
    r = s.get_projection(new)
    c = _ProjEngine.calls[-1]
    assert c["last_n"] == 4 and c["end_iter"] is None and c["min_load"] == 1.0 and c["n_steps"] == 200 and c["exposures"]
    assert np.array_equal(c["used"], [1, 1, 1, 1]) and np.array_equal(c["X"], new) and c["X"].dtype == np.float64
    assert r["n_used"] == 4 and r["n_present"] == 5 and r["total"] == 123.0 and r["max_rel_change"] == 1e-4 and r["min_cosine_at"] == 2
    for k in ("exposure_mean", "exposure_sd", "share", "p_present", "lower", "upper"):
        assert r[k].shape == (3, 4), k
    assert (r["exposure_sd"] == 3.0).all()
    # quantile type 7 of the 4 values 0, 1, 2, 3 at 0.025 and 0.975
    assert np.allclose(r["lower"], 0.075, rtol=1e-13) and np.allclose(r["upper"], 3.0 - 0.075, rtol=1e-13)
    assert list(r["fit"].columns) == ["cosine", "rel_l1", "max_rel_change"] and len(r["fit"]) == 4
    r = s.get_projection(new, end_iter=8, n_samples=5, idx=[4, 6, 8], n_steps=50, min_load=2.5, credible_interval=0.5)
    c = _ProjEngine.calls[-1]
    assert c["end_iter"] == 8 and c["last_n"] == 5 and np.array_equal(c["used"], [1, 0, 1, 0, 1]) and c["n_steps"] == 50 and c["min_load"] == 2.5
    assert r["n_used"] == 3 and r["n_steps"] == 50 and np.allclose(r["lower"], 0.5) and np.allclose(r["upper"], 1.5)
    s.get_projection(new, end_iter=8, n_samples=5, idx=None)
    assert _ProjEngine.calls[-1]["used"] is None
    with pytest.raises(ValueError, match="not all recorded"):
        s.get_projection(new, end_iter=12, n_samples=3)
    with pytest.raises(ValueError, match="idx must lie in"):
        s.get_projection(new, end_iter=8, n_samples=3, idx=[2])
    s.close()
    t = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "one"), engine_factory=_NoWaicEngine)
    with pytest.raises(ValueError, match="get_projection needs an engine"):
        t.get_projection(new)
    t.close()


def test_new_symbols_declared_exported_and_bound():
    import ctypes as C
    from bayesnmf_amd import engine
    hdr = open(os.path.join(ROOT, "include", "bnmf.h")).read()
    assert re.search(r"typedef struct \{ int32_t n_used, n_steps; int64_t n_present; double min_load, total, max_rel_change, min_cosine;\s*"
                     r"int64_t min_cosine_at [^}]*; \} bnmf_project_info;", hdr)
    assert re.search(r"#define BNMF_PROJ_NLOAD 4\b", hdr) and re.search(r"#define BNMF_PROJ_NFIT\s+3\b", hdr) and re.search(r"#define BNMF_PROJ_MAX_N 128\b", hdr)
    assert re.search(r"#define BNMF_VERSION 100\b", hdr)
    for sym in ("bnmf_project", "bnmf_project_at"):
        assert re.search(r"\bint\s+%s\s*\(\s*bnmf_handle\s*\*" % sym, hdr), f"{sym} not declared in include/bnmf.h"
        assert sym in engine.ABI_SYMBOLS
    so = os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    L = engine.lib()
    for sym, nargs in (("bnmf_project", 12), ("bnmf_project_at", 13)):
        assert re.search(r"\bT %s$" % sym, exported, re.M), f"{sym} not exported by libbnmf.so"
        assert len(getattr(L, sym).argtypes) == nargs
    assert C.sizeof(engine.BnmfProjectInfo) == 56
    assert hasattr(engine.Engine, "project")
