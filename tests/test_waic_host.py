"""WAIC of a recorded range, the parts that need no GPU: the numpy restatement of the spec (tests/waic_ref.py) against closed forms,
bayesNMF(rank_method = "WAIC") over a stub engine whose waic returns scripted values, and the two new symbols."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from waic_ref import waic_reference, canon64_colsum, seq_sum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------------- the reference function
def _samples(S, K, G, N, seed):
    rng = np.random.default_rng(seed)
    P = rng.gamma(2.0, 1.0, size=(S, K, N))
    E = rng.gamma(2.0, 1.0, size=(S, N, G))
    A = np.ones((S, N))
    M = rng.poisson(3.0, size=(K, G))
    return P, E, A, M


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_identical_samples_have_no_variance(dtype):
    P, E, A, M = _samples(1, 7, 5, 3, 1)
    S = 6
    r = waic_reference(np.repeat(P, S, 0), np.repeat(E, S, 0), np.repeat(A, S, 0), None, M, "poisson", dtype)
    one = waic_reference(np.repeat(P, 2, 0), np.repeat(E, 2, 0), np.repeat(A, 2, 0), None, M, "poisson", dtype)
    assert (r["p_cell"] == 0).all() and r["p_waic"] == 0 and r["n_high_var"] == 0
    assert np.array_equal(r["lppd_cell"], r["mean_cell"])                      # lppd = l, exactly: exp(0) = 1, log(S / S) = 0
    assert np.array_equal(r["lppd_cell"], one["lppd_cell"])
    c = (P[0] * A[0][None, :]) @ E[0]
    l = M * np.log(c) - c - np.vectorize(math.lgamma)(M + 1.0)
    assert np.allclose(np.asarray(r["lppd_cell"], dtype=float), l, rtol=1e-13, atol=1e-13)
    assert r["elpd_waic"] == r["lppd"] and r["waic"] == -2 * r["elpd_waic"]


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
@pytest.mark.parametrize("likelihood", ["poisson", "normal"])
def test_two_samples_closed_form(dtype, likelihood):
    # one cell, one factor: c_1 = 2 * 3, c_2 = 0.5 * 3
    P = np.array([[[2.0]], [[0.5]]]); E = np.array([[[3.0]], [[3.0]]]); A = np.ones((2, 1))
    if likelihood == "poisson":
        M, sig = np.array([[4]]), None
        l1, l2 = (4 * math.log(c) - c - math.lgamma(5.0) for c in (6.0, 1.5))
    else:
        M, sig = np.array([[-1.25]]), np.array([[2.0], [0.7]])
        l1, l2 = (-0.5 * math.log(2 * math.pi * v) - (-1.25 - c) ** 2 / (2 * v) for c, v in ((6.0, 2.0), (1.5, 0.7)))
    r = waic_reference(P, E, A, sig, M, likelihood, dtype)
    assert float(r["lppd"]) == pytest.approx(math.log((math.exp(l1) + math.exp(l2)) / 2), rel=1e-13)
    assert float(r["p_waic"]) == pytest.approx((l1 - l2) ** 2 / 2, rel=1e-13)
    assert float(r["mean_loglik"]) == pytest.approx((l1 + l2) / 2, rel=1e-13)
    assert float(r["elpd_waic"]) == pytest.approx(float(r["lppd"]) - float(r["p_waic"]), rel=1e-13)
    assert r["n_used"] == 2 and r["n_high_var"] == int((l1 - l2) ** 2 / 2 > 0.4)


def test_reference_streams_agree_with_the_batch_formulas_and_clip():
    S, K, G, N = 9, 70, 4, 3
    P, E, A, M = _samples(S, K, G, N, 5)
    A[2:5, 1] = 0.0                                             # samples of another rank
    E[:, :, 3] = 0.0; M[:, 3] = 0                               # a column of zeros: Mhat clipped at 1e-6
    r = waic_reference(P, E, A, None, M, "poisson", np.longdouble)
    c = np.maximum(np.einsum("skn,sn,sng->skg", P, A, E), 1e-6)
    l = M[None] * np.log(c) - c - np.vectorize(math.lgamma)(M + 1.0)[None]
    assert np.allclose(np.asarray(r["lppd_cell"], float), np.log(np.exp(l).mean(0)), rtol=1e-12)
    assert np.allclose(np.asarray(r["p_cell"], float), l.var(0, ddof=1), rtol=1e-10, atol=1e-13)
    assert np.allclose(np.asarray(r["lppd_cell"], float)[:, 3], -1e-6, rtol=1e-12) and (np.asarray(r["p_cell"])[:, 3] == 0).all()
    e = np.asarray(r["elpd_cell"], float)
    assert float(r["se_elpd"]) == pytest.approx(math.sqrt(K * G * e.var(ddof=1)), rel=1e-12)
    # the canonical column reduction and the sequential total are sums: they agree with numpy's to rounding
    assert np.allclose(canon64_colsum(e), e.sum(0), rtol=1e-13) and seq_sum(e.sum(0)) == pytest.approx(e.sum(), rel=1e-13)


# ----------------------------------------------------------------------------------------------- bayesNMF(rank_method = "WAIC")
class _NoWaicEngine:
    """what bayesNMF_sampler needs of an engine to run a fixed-rank chain to its final MAP; nothing is sampled.  No waic."""
    made = []

    def __init__(self, M, N, **kw):
        self.K, self.G = M.shape
        self.N, self.it, self.fixed = N, 0, None
        type(self).made.append(self)

    def set(self, name, value):
        pass

    def set_fixed(self, name, mask):
        self.fixed = np.array(mask)

    def get(self, name):
        shp = dict(P=(self.K, self.N), E=(self.N, self.G), A=(1, self.N), R=(1,)).get(name, (self.K, self.N) if name.endswith("_p") else (self.N, self.G))
        return np.ones(shp)

    def _rows(self, n):
        rows = np.zeros((n, 11))
        rows[:, 0] = np.arange(self.it + 1, self.it + n + 1)
        rows[:, 3] = -100.0 * self.N                             # loglikelihood: BIC = 200 N + n_params log G grows with the rank
        rows[:, 5] = self.N * (self.K + self.G)
        self.it += n
        return rows

    def init(self):
        return self._rows(1)[0]

    def run(self, n, converged=False, metrics=True):
        return self._rows(n)

    def map(self, last_n, credible_interval=0.95, end_iter=None):
        K, G, N = self.K, self.G, self.N
        return dict(P=np.ones((K, N)), E=np.ones((N, G)), A=np.ones((1, N)), used=np.ones(last_n, dtype=bool), P_lower=None, P_upper=None,
                    E_lower=None, E_upper=None, top_A=np.ones((1, N)), top_counts=[last_n], n_used=last_n, n_patterns=1, rmse=1.0, kl=1.0)

    def close(self):
        pass


SCRIPT = {2: -510.0, 3: -480.5, 4: -470.25, 5: -475.0}        # elpd_waic by rank: 4 is best, while BIC prefers the smallest rank


class _WaicEngine(_NoWaicEngine):
    calls = []

    def waic(self, last_n, used=None, end_iter=None, pointwise=False):
        type(self).calls.append(dict(N=self.N, last_n=last_n, used=None if used is None else np.array(used), end_iter=end_iter, it=self.it))
        e = SCRIPT[self.N]
        return dict(n_used=int(np.sum(used)) if used is not None else last_n, n_high_var=self.N, lppd=e + 10.0, p_waic=10.0, elpd_waic=e,
                    waic=-2 * e, se_elpd=0.5 * self.N, mean_loglik=e - 1.0)


def _run(tmp_path, factory, ranks, **kw):
    from bayesnmf_amd import sampler as S
    from bayesnmf_amd.convergence import new_convergence_control
    from bayesnmf_amd.setup import synth_counts
    M, _, _ = synth_counts(12, 9, 2, 3, mean_total=200)
    cc = new_convergence_control()
    cc.update(MAP_over=4, MAP_every=2, maxiters=6, miniters=2)
    return S.bayesNMF(M, ranks, likelihood="poisson", prior="gamma", rank_method="WAIC", convergence_control=cc, devices=[0],
                      engine_factory=factory, output_dir=str(tmp_path / "waic"), periodic_save=False, save_all_samples=False, **kw)


def test_waic_sweep_picks_the_largest_elpd(tmp_path):
    _WaicEngine.calls = []
    out = _run(tmp_path, _WaicEngine, range(2, 6))
    assert out["best_rank"] == 4 and out["sampler"].dims["N"] == 4
    t = out["results"]
    assert {"rank", "BIC", "elpd_waic", "se_elpd", "p_waic", "n_high_var"} <= set(t.columns)
    assert list(t["rank"]) == [4, 5, 3, 2]                                   # sorted by elpd_waic, largest first
    assert list(t["elpd_waic"]) == [SCRIPT[k] for k in (4, 5, 3, 2)]
    assert t.set_index("rank")["BIC"].idxmin() == 2                          # BIC, carried for comparison, would have chosen otherwise
    assert list(t.set_index("rank").loc[[2, 3, 4, 5], "n_high_var"]) == [2, 3, 4, 5]
    # one call per rank, over the final MAP window (the last MAP_over samples), restricted to MAP$idx
    assert sorted(c["N"] for c in _WaicEngine.calls) == [2, 3, 4, 5]
    for c in _WaicEngine.calls:
        assert c["last_n"] == 4 and c["end_iter"] is None and c["it"] == 6 and np.array_equal(c["used"], [1, 1, 1, 1])
    for r in out["results"]["dir"]:
        assert os.path.isdir(r)


def test_waic_sweep_drops_the_ranks_below_F(tmp_path, capsys):
    _WaicEngine.calls = []
    fp = np.random.default_rng(1).dirichlet(np.ones(12), size=3).T
    out = _run(tmp_path, _WaicEngine, range(1, 6), fixed_P=fp)
    assert sorted(c["N"] for c in _WaicEngine.calls) == [3, 4, 5] and out["best_rank"] == 4
    assert "dropping ranks [1, 2]" in capsys.readouterr().out
    with pytest.raises(ValueError, match="top of the rank range is below 3"):
        _run(tmp_path, _WaicEngine, range(1, 3), fixed_P=fp)


def test_engine_without_waic_is_refused(tmp_path):
    with pytest.raises(ValueError, match="waic"):
        _run(tmp_path, _NoWaicEngine, range(2, 4))
    from bayesnmf_amd.sampler import bayesNMF_sampler
    from bayesnmf_amd.setup import synth_counts
    M, _, _ = synth_counts(12, 9, 2, 3, mean_total=200)
    s = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "one"), engine_factory=_NoWaicEngine)
    with pytest.raises(ValueError, match="get_WAIC needs an engine"):
        s.get_WAIC()
    s.close()


def test_other_rank_methods_are_untouched(tmp_path):
    from bayesnmf_amd import sampler as S
    from bayesnmf_amd.setup import synth_counts
    M, _, _ = synth_counts(12, 9, 2, 3, mean_total=200)
    with pytest.raises(ValueError, match="Rank method must be SBFI, BFI, BIC, or WAIC"):
        S.bayesNMF(M, range(1, 4), likelihood="poisson", prior="gamma", rank_method="AIC", engine_factory=_WaicEngine,
                   output_dir=str(tmp_path / "x"))


def test_get_WAIC_ranges_and_idx(tmp_path):
    from bayesnmf_amd.sampler import bayesNMF_sampler
    from bayesnmf_amd.convergence import new_convergence_control
    from bayesnmf_amd.setup import synth_counts
    M, _, _ = synth_counts(12, 9, 2, 3, mean_total=200)
    cc = new_convergence_control()
    cc.update(MAP_over=4, MAP_every=2, maxiters=10, miniters=2)
    s = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "r"), engine_factory=_WaicEngine,
                         convergence_control=cc, save_all_samples=True, periodic_save=False)
    s.run_gibbs_sampler()
    _WaicEngine.calls = []
    w = s.get_WAIC()
    assert w["elpd_waic"] == SCRIPT[3] and _WaicEngine.calls[-1]["last_n"] == 4
    s.get_WAIC(end_iter=8, n_samples=5, idx=None)
    c = _WaicEngine.calls[-1]
    assert c["end_iter"] == 8 and c["last_n"] == 5 and c["used"] is None
    s.get_WAIC(end_iter=8, n_samples=5, idx=[4, 6, 8])
    assert np.array_equal(_WaicEngine.calls[-1]["used"], [1, 0, 1, 0, 1])
    s.get_WAIC(end_iter=8, n_samples=5)                       # "MAP_idx" of another range: the mode of that range (Engine.map)
    assert np.array_equal(_WaicEngine.calls[-1]["used"], [1, 1, 1, 1, 1])
    with pytest.raises(ValueError, match="not all recorded"):
        s.get_WAIC(end_iter=12, n_samples=3)
    with pytest.raises(ValueError, match="idx must lie in"):
        s.get_WAIC(end_iter=8, n_samples=3, idx=[2])
    s.close()


# ----------------------------------------------------------------------------------------------- symbols
def test_new_symbols_declared_exported_and_bound():
    from bayesnmf_amd import engine
    hdr = open(os.path.join(ROOT, "include", "bnmf.h")).read()
    assert re.search(r"typedef struct \{ int32_t n_used, n_high_var;\s*double lppd, p_waic, elpd_waic, waic[^;]*, se_elpd, mean_loglik; \} bnmf_waic_info;", hdr)
    assert re.search(r"#define BNMF_VERSION 100\b", hdr)
    for sym in ("bnmf_waic", "bnmf_waic_at"):
        assert re.search(r"\bint\s+%s\s*\(\s*bnmf_handle\s*\*" % sym, hdr), f"{sym} not declared in include/bnmf.h"
        assert sym in engine.ABI_SYMBOLS
    so = os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    L = engine.lib()
    for sym, nargs in (("bnmf_waic", 6), ("bnmf_waic_at", 7)):
        assert re.search(r"\bT %s$" % sym, exported, re.M), f"{sym} not exported by libbnmf.so"
        assert len(getattr(L, sym).argtypes) == nargs
    import ctypes as C
    assert C.sizeof(engine.BnmfWaicInfo) == 8 + 6 * 8
    assert hasattr(engine.Engine, "waic")
