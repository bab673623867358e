"""Signature attribution of a recorded range, the parts that need no GPU: the numpy restatement of the spec
(tests/attribution_ref.py) against its laws and on a planted case, bayesNMF_sampler.get_attribution over a stub engine, and the two
new symbols."""
import os
import re
import subprocess

import numpy as np
import pytest

import attribution_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


def _samples(S, K, G, N, seed):
    rng = np.random.default_rng(seed)
    P = rng.gamma(2.0, 1.0, size=(S, K, N))
    E = rng.gamma(2.0, 1.0, size=(S, N, G))
    A = np.ones((S, N))
    M = rng.poisson(30.0, size=(K, G))
    return P, E, A, M


def test_the_allocation_sums_to_the_data_and_the_shares_to_one(oracle_lib):
    S, K, G, N = 7, 150, 5, 6                                   # two row chunks
    P, E, A, M = _samples(S, K, G, N, 2)
    A[2:4, 1] = 0.0                                             # samples of another rank
    E[:, :, 3] = 0.0                                            # a tumour no factor reaches: c = 0 in every cell, t = 0
    A[5, :] = 0.0                                               # a sample that excludes every factor
    r = R.attribution_reference(P, E, A, M, "poisson", min_load=1.0)
    for k in ("load", "prob", "series", "x", "a", "shares"):
        assert np.isfinite(r[k]).all(), k
    assert np.isfinite(r["total"])
    c, x, m = r["c"], r["x"], np.asarray(M, dtype=np.float64)
    pos = c > 0
    assert pos.any() and (~pos).any()
    sx = np.zeros_like(c)
    for n in range(N):                                          # sum_n x_n, n ascending
        sx = sx + x[:, :, n, :]
    bound = 4 * N * EPS * m[None]
    assert (np.abs(sx - m[None])[pos] <= np.broadcast_to(bound, c.shape)[pos]).all()
    assert (x[~pos[:, :, None, :].repeat(N, 2)] == 0).all()     # c = 0: r = 0 for every factor, no NaN
    # the share of a (tumour, sample): 1 within 4 N eps, or exactly 0 where the tumour's load is 0
    t = r["a"].sum(axis=1)
    ssum = np.zeros_like(t)
    for n in range(N):
        ssum = ssum + r["shares"][:, n, :]
    assert (np.abs(ssum - 1.0)[t > 0] <= 4 * N * EPS).all() and (ssum[t == 0] == 0).all() and (t == 0).any()
    # total against the data, where every cell is reached in every sample: the same bound, summed over the cells
    Mz = M.copy()
    Mz[:, 3] = 0
    keep = [s for s in range(S) if s != 5]
    rz = R.attribution_reference(P[keep], E[keep], np.ones((S - 1, N)), Mz, "poisson")
    print(f"total {rz['total']!r} sum of the data {Mz.sum()} bound {4 * N * EPS * Mz.sum():.3e}")
    assert abs(rz["total"] - Mz.sum()) <= 4 * N * EPS * Mz.sum()
    # prob is a distribution over the factors wherever some sample reaches the cell
    pr = r["prob"].sum(axis=1)
    reached = pos.sum(axis=0) / S
    assert np.allclose(pr, reached, rtol=0, atol=8 * N * EPS)
    assert r["n_used"] == S and r["load"].shape == (4, N, G) and r["series"].shape == (S, N)
    assert (r["p_present"][:, 3] == 0).all() and r["n_present"] == int((r["p_present"] >= 0.5).sum())


def test_welford_rows_are_the_moments_of_the_loads(oracle_lib):
    S, K, G, N = 9, 70, 4, 3
    P, E, A, M = _samples(S, K, G, N, 5)
    r = R.attribution_reference(P, E, A, M, "poisson", min_load=500.0)
    a = r["a"]
    assert np.allclose(r["load_mean"], a.mean(axis=0), rtol=1e-13)
    assert np.allclose(r["load_var"], a.var(axis=0, ddof=1), rtol=1e-10)
    assert np.allclose(r["share"], r["shares"].mean(axis=0), rtol=1e-13)
    assert np.array_equal(r["p_present"], (a >= 500.0).mean(axis=0))
    assert np.allclose(r["series"], a.sum(axis=2), rtol=1e-13)
    assert r["total"] == pytest.approx(a.sum() / S, rel=1e-13)
    # Normal: the components of the fit, whatever the data
    rn = R.attribution_reference(P, E, A, M - 40.5, "normal")
    assert np.allclose(rn["a"], np.einsum("skn,sn,sng->sng", P, A, E), rtol=1e-13)
    assert np.array_equal(rn["prob"], r["prob"])                # the shares do not look at the data


def test_planted_signatures_are_found_where_they_are(oracle_lib):
    rng = np.random.default_rng(7)
    K, G, N, S = 24, 6, 3, 20
    P0 = rng.dirichlet(np.full(K, 0.5), size=N).T               # K x N signatures
    E0 = rng.gamma(4.0, 100.0, size=(N, G))
    E0[2, 0] = 0.0                                              # tumour 0 has no exposure to signature 2
    M = rng.poisson(P0 @ E0).astype(np.int32)
    Ps = P0[None] * rng.uniform(0.95, 1.05, size=(S, K, N))     # samples jittered around the truth
    Es = E0[None] * rng.uniform(0.95, 1.05, size=(S, N, G))
    r = R.attribution_reference(Ps, Es, np.ones((S, N)), M, "poisson", min_load=1.0)
    print("p_present\n", r["p_present"], "\nload_mean\n", r["load_mean"].round(1), "\nE0\n", E0.round(1))
    assert r["p_present"][2, 0] == 0.0 and r["load_mean"][2, 0] == 0.0 and r["share"][2, 0] == 0.0
    assert (r["p_present"][2, 1:] >= 0.5).all()
    assert (r["prob"][:, 2, 0] == 0).all()
    assert np.allclose(r["load_mean"], E0, rtol=0.25, atol=30.0)             # the loads recover the exposures
    assert abs(r["total"] - M.sum()) <= 4 * N * EPS * M.sum()
    assert r["n_present"] == N * G - 1


def test_get_attribution_ranges_idx_and_result(tmp_path):
    """bayesNMF_sampler.get_attribution over a stub engine: the range and idx rules of get_WAIC (_recorded_range), the shape of the result"""
    from test_waic_host import _NoWaicEngine
    from bayesnmf_amd.sampler import bayesNMF_sampler
    from bayesnmf_amd.convergence import new_convergence_control
    from bayesnmf_amd.setup import synth_counts

    class _AttrEngine(_NoWaicEngine):
        calls = []

        def attribution(self, last_n, used=None, end_iter=None, min_load=1.0, prob=False):
            type(self).calls.append(dict(last_n=last_n, used=None if used is None else np.array(used), end_iter=end_iter, min_load=min_load, prob=prob))
            S = last_n if used is None else int(np.sum(used))
            K, G, N = self.K, self.G, self.N
            series = np.arange(S * N, dtype=float).reshape(S, N)
            out = dict(n_used=S, n_present=5, min_load=min_load, total=123.0, series=series, load_mean=np.full((N, G), 2.0),
                       load_var=np.full((N, G), 9.0), share=np.full((N, G), 1.0 / N), p_present=np.full((N, G), 0.75))
            if prob:
                out["prob"] = np.full((K, N, G), 1.0 / N)
            return out

    M, _, _ = synth_counts(12, 9, 2, 3, mean_total=200)
    cc = new_convergence_control()
    cc.update(MAP_over=4, MAP_every=2, maxiters=10, miniters=2)
    s = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "r"), engine_factory=_AttrEngine,
                         convergence_control=cc, save_all_samples=True, periodic_save=False)
    s.run_gibbs_sampler()
    r = s.get_attribution()
    c = _AttrEngine.calls[-1]
    assert c["last_n"] == 4 and c["end_iter"] is None and c["min_load"] == 1.0 and not c["prob"] and np.array_equal(c["used"], [1, 1, 1, 1])
    assert r["n_used"] == 4 and r["n_present"] == 5 and r["total"] == 123.0 and "prob" not in r
    for k in ("load_mean", "load_sd", "share", "p_present"):
        assert r[k].shape == (3, 9), k
    assert (r["load_sd"] == 3.0).all()
    co = r["cohort"]
    assert list(co.columns) == ["signature", "mean", "lower", "upper"] and list(co["signature"]) == [1, 2, 3]
    ser = np.arange(12, dtype=float).reshape(4, 3)
    assert np.array_equal(co["mean"], ser.mean(axis=0))
    # quantile type 7 of 4 values at 0.025: x_(1) + 0.075 (x_(2) - x_(1))
    assert np.allclose(co["lower"], ser[0] + 0.075 * 3.0, rtol=1e-14) and np.allclose(co["upper"], ser[3] - 0.075 * 3.0, rtol=1e-14)
    r = s.get_attribution(end_iter=8, n_samples=5, idx=[4, 6, 8], min_load=2.5, credible_interval=0.5, prob=True)
    c = _AttrEngine.calls[-1]
    assert c["end_iter"] == 8 and c["last_n"] == 5 and np.array_equal(c["used"], [1, 0, 1, 0, 1]) and c["prob"] and c["min_load"] == 2.5
    assert r["prob"].shape == (12, 3, 9) and r["n_used"] == 3
    assert np.allclose(r["cohort"]["lower"], np.arange(3) + 0.5 * 3.0)       # the lower quartile of 3 values: halfway to the median
    s.get_attribution(end_iter=8, n_samples=5, idx=None)
    assert _AttrEngine.calls[-1]["used"] is None
    with pytest.raises(ValueError, match="not all recorded"):
        s.get_attribution(end_iter=12, n_samples=3)
    with pytest.raises(ValueError, match="idx must lie in"):
        s.get_attribution(end_iter=8, n_samples=3, idx=[2])
    s.close()
    t = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "one"), engine_factory=_NoWaicEngine)
    with pytest.raises(ValueError, match="get_attribution needs an engine"):
        t.get_attribution()
    t.close()


def test_new_symbols_declared_exported_and_bound():
    import ctypes as C
    from bayesnmf_amd import engine
    hdr = open(os.path.join(ROOT, "include", "bnmf.h")).read()
    assert re.search(r"typedef struct \{ int32_t n_used, _pad; int64_t n_present; double min_load, total; \} bnmf_attr_info;", hdr)
    assert re.search(r"#define BNMF_ATTR_NLOAD 4\b", hdr) and re.search(r"#define BNMF_VERSION 100\b", hdr)
    for sym in ("bnmf_attribution", "bnmf_attribution_at"):
        assert re.search(r"\bint\s+%s\s*\(\s*bnmf_handle\s*\*" % sym, hdr), f"{sym} not declared in include/bnmf.h"
        assert sym in engine.ABI_SYMBOLS
    so = os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    L = engine.lib()
    for sym, nargs in (("bnmf_attribution", 8), ("bnmf_attribution_at", 9)):
        assert re.search(r"\bT %s$" % sym, exported, re.M), f"{sym} not exported by libbnmf.so"
        assert len(getattr(L, sym).argtypes) == nargs
    assert C.sizeof(engine.BnmfAttrInfo) == 32
    assert hasattr(engine.Engine, "attribution")
