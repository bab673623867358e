"""Mixing diagnostics of a recorded range, the parts that need no GPU: the numpy restatement of the spec (tests/mixing_ref.py) against
closed forms, against an independent implementation (FFT autocovariances, np.mean / np.var) and against the law of AR(1) series;
multichain.combine_rhat against a direct computation; get_mixing's defaults over a stub engine; the two new symbols."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from mixing_ref import mixing_reference, mixing_independent, mixing_summary, ar1, ROWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------------- closed forms
def test_a_constant_series_is_degenerate():
    x = np.column_stack([np.full(50, 3.25), np.r_[np.full(49, 1.0), np.nan], np.arange(50.0)])
    r = mixing_reference(x)
    for j in (0, 1):
        assert all(np.isnan(r[k][j]) for k in ("ess", "mcse", "rhat")) and r["pairs"][j] == 0 and r["exit"][j] == 0
    assert r["mean"][0] == 3.25 and r["var"][0] == 0.0 and r["mean_a"][0] == 3.25 and r["var_b"][0] == 0.0
    assert np.isfinite(r["ess"][2]) and r["pairs"][2] >= 1
    info = mixing_summary(r["rows"][:, :2], r["rows"][:, 2:], 2, 1, 50)
    assert info["n_const"] == 2 and info["min_ess_P_at"] == -1 and math.isnan(info["min_ess_P"]) and info["min_ess_E_at"] == 0


def test_a_constant_series_whose_mean_does_not_round_back_is_degenerate():
    """nine samples of 0.7: canon(x) / 9 is not 0.7, so d_s and gamma0 are rounding noise, not zero: the series is still constant"""
    x = np.full((9, 2), 0.7)
    x[4, 1] = np.nextafter(0.7, 1.0)                                          # one sample an ulp away: not constant
    r = mixing_reference(x)
    assert r["mean"][0] != 0.7 and 0.0 < r["var"][0] < 1e-30
    assert np.isnan(r["ess"][0]) and np.isnan(r["mcse"][0]) and np.isnan(r["rhat"][0]) and r["pairs"][0] == 0 and r["exit"][0] == 0
    assert r["pairs"][1] >= 1 and np.isfinite(r["ess"][1])


@pytest.mark.parametrize("S", [10, 100, 1000])
def test_the_alternating_series_is_floored_at_S_log10_S(S):
    r = mixing_reference(((-1.0) ** np.arange(S))[:, None])
    assert r["ess"][0] == S / (1.0 / math.log10(S)) and r["ess"][0] == pytest.approx(S * math.log10(S), rel=1e-15)
    assert r["exit"][0] == 1 and r["pairs"][0] == (S - 3) // 2 + 1           # every Gamma is 1 / S > 0: the lags run out
    assert r["mean"][0] == 0.0
    if (S // 2) % 2 == 0:                                                     # halves of mean 0: B = 0
        assert r["rhat"][0] == pytest.approx(math.sqrt((S // 2 - 1) / (S // 2)), rel=1e-14)


@pytest.mark.parametrize("S", [4, 10, 64, 130, 1000])
def test_a_ramp_has_rhat_in_closed_form(S):
    r = mixing_reference(np.arange(float(S))[:, None])
    h = S // 2
    assert r["mean_a"][0] == (h - 1) / 2 and r["mean_b"][0] == (h - 1) / 2 + h
    assert r["var_a"][0] == pytest.approx(h * (h + 1) / 12, rel=1e-13) and r["var_b"][0] == pytest.approx(h * (h + 1) / 12, rel=1e-13)
    W = h * (h + 1) / 12
    assert r["rhat"][0] == pytest.approx(math.sqrt((W * (h - 1) / h + h * h / 2) / W), rel=1e-12)
    assert r["mean"][0] == (S - 1) / 2 and r["var"][0] == pytest.approx(S * (S + 1) / 12, rel=1e-13)


def test_four_samples_are_the_minimum():
    x = np.random.default_rng(5).normal(size=(4, 9))
    r = mixing_reference(x)
    assert (r["pairs"] == 1).all() and (r["exit"] == 1).all()                 # Gamma_0 alone: 2 m + 1 <= S - 2 admits no m
    assert np.isfinite(r["rows"]).all()
    assert np.allclose(r["var_a"], x[:2].var(axis=0, ddof=1), rtol=1e-13) and np.allclose(r["var_b"], x[2:].var(axis=0, ddof=1), rtol=1e-13)
    with pytest.raises(AssertionError):
        mixing_reference(x[:3])


def test_an_odd_middle_sample_is_dropped():
    x = np.random.default_rng(6).normal(size=(9, 3))
    r = mixing_reference(x)
    assert np.allclose(r["mean_a"], x[:4].mean(0), rtol=1e-13) and np.allclose(r["mean_b"], x[5:].mean(0), rtol=1e-13)


# ----------------------------------------------------------------------------------------------- restatement vs independent implementation
AR_CASES = [(0.0, 130, 11), (0.5, 130, 12), (0.9, 130, 13), (0.0, 1000, 14), (0.5, 1000, 15), (0.9, 1000, 16), (-0.5, 257, 17), (0.99, 1000, 18)]


@pytest.mark.parametrize("phi,S,seed", AR_CASES)
def test_restatement_agrees_with_fft_autocovariances(phi, S, seed):
    x = ar1(phi, S, 40, seed)
    r, q = mixing_reference(x), mixing_independent(x)
    assert not q["fragile"].any(), "choose another seed: a Gamma of the independent implementation lies within 1e-9 of a decision"
    assert np.array_equal(r["pairs"], q["pairs"]) and np.array_equal(r["exit"], q["exit"])
    assert np.allclose(r["tau"], q["tau"], rtol=1e-9, atol=0) and np.allclose(r["ess"], q["ess"], rtol=1e-9, atol=0)
    assert np.allclose(r["rhat"], q["rhat"], rtol=1e-12, atol=0)
    assert np.allclose(r["mean"], q["mean"], rtol=1e-12, atol=1e-15) and np.allclose(r["var"], q["var"], rtol=1e-12, atol=0)
    assert np.allclose(r["mcse"], np.sqrt(q["var"] / q["ess"]), rtol=1e-9, atol=0)


# ----------------------------------------------------------------------------------------------- the law of AR(1)
LAW_S, LAW_L = 1000, 200


def _independent_spread(phi):
    """the ratio median(ess / S) / ((1 - phi) / (1 + phi)) the INDEPENDENT implementation shows over 8 batches of other seeds"""
    want = (1.0 - phi) / (1.0 + phi)
    return [float(np.median(mixing_independent(ar1(phi, LAW_S, LAW_L, 1000 + 10 * b + int(10 * phi)))["ess"] / LAW_S)) / want for b in range(8)]


@pytest.mark.parametrize("phi", [0.0, 0.5, 0.9])
def test_ess_follows_the_law_of_an_ar1_series(phi):
    """Bracket: the minimum and maximum of the independent implementation's batch ratios, widened on each side by their range (the
    batches are 8 draws of the statistic; the 9th, from the code under test on seeds of its own, may fall outside their hull, rarely
    by more than its width).  Geyer's truncated sum is biased, so the ratios do not centre on 1: what is checked is that the
    restatement shows the independent implementation's behaviour.  Measured: DESIGN.md 13."""
    ratios = _independent_spread(phi)
    lo, hi = min(ratios), max(ratios)
    lo, hi = lo - (hi - lo), hi + (hi - lo)
    r = mixing_reference(ar1(phi, LAW_S, LAW_L, 77 + int(10 * phi)))
    got = float(np.median(r["ess"] / LAW_S)) / ((1.0 - phi) / (1.0 + phi))
    print(f"law[phi = {phi}]: independent batch ratios {min(ratios):.4f} .. {max(ratios):.4f}, bracket {lo:.4f} .. {hi:.4f}, restatement {got:.4f}")
    assert 0.5 < lo and hi < 1.5, "the independent implementation itself is off the law"
    assert lo <= got <= hi


# ----------------------------------------------------------------------------------------------- combine_rhat
def _chains(C, S, K, N, G, seed, shift=0.0):
    rng = np.random.default_rng(seed)
    return [(rng.normal(size=(S, K, N)) + shift * c, rng.normal(size=(S, N, G)) * (1.0 + c)) for c in range(C)]


def _halves(P, E):
    h = P.shape[0] // 2
    S = P.shape[0]
    d = dict(n_half=h)
    for side, w in (("P", P), ("E", E)):
        for half, part in (("a", w[:h]), ("b", w[S - h:])):
            d[f"mean_{half}_{side}"], d[f"var_{half}_{side}"] = part.mean(axis=0), part.var(axis=0, ddof=1)
    return d


def _direct_rhat(ws):
    """ws: the chains' sample arrays [S][...]; R-hat over their 2 C halves, straight from the definition"""
    S = ws[0].shape[0]
    h = S // 2
    halves = np.stack([part for w in ws for part in (w[:h], w[S - h:])])        # [2C][h][...]
    W = halves.var(axis=1, ddof=1).mean(axis=0)
    B = h * halves.mean(axis=1).var(axis=0, ddof=1)
    return np.sqrt(((h - 1) / h * W + B / h) / W)


def test_combine_rhat_is_the_definition():
    from bayesnmf_amd.multichain import combine_rhat
    ch = _chains(3, 41, 4, 3, 5, 2, shift=0.3)
    out = combine_rhat([_halves(P, E) for P, E in ch])
    assert out["n_half"] == 20 and out["n_chains"] == 3
    assert np.allclose(out["rhat_P"], _direct_rhat([P for P, _ in ch]), rtol=1e-12) and out["rhat_P"].shape == (4, 3)
    assert np.allclose(out["rhat_E"], _direct_rhat([E for _, E in ch]), rtol=1e-12) and out["rhat_E"].shape == (3, 5)
    assert (out["rhat_P"] > 1.0).any()
    one = combine_rhat([_halves(*ch[0])])                                     # one chain: its own split R-hat
    assert np.allclose(one["rhat_P"], mixing_reference(ch[0][0].reshape(41, -1))["rhat"].reshape(4, 3), rtol=1e-12)


def test_combine_rhat_aligns_labels_with_perm():
    from bayesnmf_amd.multichain import combine_rhat
    ch = _chains(3, 40, 4, 3, 5, 3, shift=0.0)
    perms = [np.array([0, 1, 2]), np.array([2, 0, 1]), np.array([1, 0, 2])]
    # chain c relabelled: its factor perms[c][j] is the common factor j
    mixed = []
    for (P, E), p in zip(ch, perms):
        inv = np.argsort(p)
        mixed.append((P[:, :, inv], E[:, inv, :]))
    aligned = combine_rhat([_halves(P, E) for P, E in mixed], perm=perms)
    plain = combine_rhat([_halves(P, E) for P, E in ch])
    assert np.array_equal(aligned["rhat_P"], plain["rhat_P"]) and np.array_equal(aligned["rhat_E"], plain["rhat_E"])
    unaligned = combine_rhat([_halves(P, E) for P, E in mixed])
    assert not np.allclose(unaligned["rhat_E"], plain["rhat_E"])
    with pytest.raises(ValueError, match="not a permutation"):
        combine_rhat([_halves(P, E) for P, E in mixed], perm=[[0, 0, 1]] * 3)
    with pytest.raises(ValueError, match="perm has 2 entries"):
        combine_rhat([_halves(P, E) for P, E in mixed], perm=perms[:2])


def test_combine_rhat_refuses_unequal_halves():
    from bayesnmf_amd.multichain import combine_rhat
    a, b = _chains(2, 40, 4, 3, 5, 4)
    with pytest.raises(ValueError, match="n_half"):
        combine_rhat([_halves(*a), _halves(b[0][:30], b[1][:30])])


# ----------------------------------------------------------------------------------------------- get_mixing over a stub engine
def _stub_engines():
    from test_waic_host import _NoWaicEngine

    class _MixEngine(_NoWaicEngine):
        calls = []

        def mixing(self, last_n, used=None, end_iter=None, keep=None, arrays=True):
            type(self).calls.append(dict(last_n=last_n, used=None if used is None else np.array(used), end_iter=end_iter,
                                         keep=None if keep is None else np.array(keep), arrays=arrays, it=self.it))
            return dict(n_used=last_n if used is None else int(np.sum(used)), n_half=last_n // 2, n_const=1, n_ran_out=2, n_low_ess=3, n_high_rhat=4,
                        min_ess_P=12.5, min_ess_E=7.25, max_rhat_P=1.5, max_rhat_E=1.25, min_ess_P_at=0, min_ess_E_at=1, max_rhat_P_at=2, max_rhat_E_at=3)
    return _NoWaicEngine, _MixEngine


def _sampler(tmp_path, factory, name):
    from bayesnmf_amd.sampler import bayesNMF_sampler
    from bayesnmf_amd.convergence import new_convergence_control
    from bayesnmf_amd.setup import synth_counts
    M, _, _ = synth_counts(12, 9, 2, 3, mean_total=200)
    cc = new_convergence_control()
    cc.update(MAP_over=4, MAP_every=2, maxiters=10, miniters=2)
    return bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / name), engine_factory=factory,
                            convergence_control=cc, save_all_samples=True, periodic_save=False)


def test_get_mixing_defaults_ranges_and_the_log_line(tmp_path):
    plain, mix = _stub_engines()
    s = _sampler(tmp_path, mix, "m")
    s.run_gibbs_sampler()
    log = open(tmp_path / "m" / "log.txt").read()
    line = [ln for ln in log.splitlines() if "Mixing over" in ln]
    assert len(line) == 1 and "min ESS P 12.5 E 7.2" in line[0] and "max split R-hat P 1.5000 E 1.2500" in line[0]
    assert "3 ESS < 100 | 4 R-hat > 1.01 | 1 constant | 2 ran out of lags" in line[0]
    assert log.index("Final MAP computed") < log.index("Mixing over") < log.index("Sampler done")
    c = mix.calls[-1]                                                         # the run's own call: the final MAP window, no arrays
    assert c["last_n"] == 4 and c["end_iter"] is None and c["arrays"] is False and np.array_equal(c["used"], [1, 1, 1, 1])
    assert np.array_equal(c["keep"], [1, 1, 1])
    m = s.get_mixing()
    c = mix.calls[-1]
    assert m["min_ess_E"] == 7.25 and c["last_n"] == 4 and c["arrays"] is True and np.array_equal(c["keep"], [1, 1, 1])
    s.get_mixing(end_iter=8, n_samples=5, idx=None)
    c = mix.calls[-1]
    assert c["end_iter"] == 8 and c["last_n"] == 5 and c["used"] is None and np.array_equal(c["keep"], [1, 1, 1])
    s.get_mixing(end_iter=8, n_samples=5, idx=[4, 6, 8])
    assert np.array_equal(mix.calls[-1]["used"], [1, 0, 1, 0, 1])
    s.get_mixing(end_iter=8, n_samples=5)
    assert np.array_equal(mix.calls[-1]["used"], [1, 1, 1, 1, 1])
    with pytest.raises(ValueError, match="not all recorded"):
        s.get_mixing(end_iter=12, n_samples=3)
    assert "gap" in type(s).get_mixing.__doc__ and "contiguous" in type(s).get_mixing.__doc__
    s.close()
    t = _sampler(tmp_path, plain, "p")                                        # an engine without mixing: no line, and a clear refusal
    t.run_gibbs_sampler()
    assert "Mixing" not in open(tmp_path / "p" / "log.txt").read()
    with pytest.raises(ValueError, match="get_mixing needs an engine"):
        t.get_mixing()
    t.close()


# ----------------------------------------------------------------------------------------------- symbols
def test_new_symbols_declared_exported_and_bound():
    import ctypes as C
    from bayesnmf_amd import engine
    hdr = open(os.path.join(ROOT, "include", "bnmf.h")).read()
    assert re.search(r"#define BNMF_NMIX 11\b", hdr) and engine.NMIX == 11 and tuple(engine.MIX_ROWS) == ROWS
    assert re.search(r"#define BNMF_MIXING_LOW_ESS 100\.0\b", hdr) and re.search(r"#define BNMF_MIXING_HIGH_RHAT 1\.01\b", hdr)
    assert "} bnmf_mixing_info;" in hdr
    for sym in ("bnmf_mixing", "bnmf_mixing_at"):
        assert re.search(r"\bint\s+%s\s*\(\s*bnmf_handle\s*\*" % sym, hdr), f"{sym} not declared in include/bnmf.h"
        assert sym in engine.ABI_SYMBOLS
    so = os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    L = engine.lib()
    for sym, nargs in (("bnmf_mixing", 7), ("bnmf_mixing_at", 8)):
        assert re.search(r"\bT %s$" % sym, exported, re.M), f"{sym} not exported by libbnmf.so"
        assert len(getattr(L, sym).argtypes) == nargs
    assert C.sizeof(engine.BnmfMixingInfo) == 2 * 4 + 8 * 8 + 4 * 8
