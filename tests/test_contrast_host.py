"""Group contrasts of exposures over a recorded range, the parts that need no GPU: the numpy restatement of the spec
(tests/contrast_ref.py) against its laws, bayesNMF_sampler.get_contrast over a stub engine, and the two new symbols."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import contrast_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53                           # the unit roundoff of float64


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _gamma(k):
    return k * U / (1.0 - k * U)


def _samples(S, K, N, G, seed, exclude=()):
    """non-negative P, E and 0 / 1 A: the samples in `exclude` include no factor at all"""
    rng = np.random.default_rng(seed)
    P = rng.gamma(0.5, 1.0, size=(S, K, N))
    E = rng.gamma(0.7, 30.0, size=(S, N, G))
    A = (rng.uniform(size=(S, N)) < 0.8).astype(np.float64)
    A[:, 0] = 1.0                                             # every other sample has a factor, so t > 0 (gamma draws are positive)
    for s in exclude:
        A[s] = 0.0
    return P, E, A


def test_shares_sum_to_one_and_vanish_without_factors():
    """sum_n v1[n, c] = 1 wherever every member has t > 0.  Per tumour: t^ = sum_n x_n (1 + th_n) with |th_n| <= gamma(N - 1) (N - 1
    additions of non-negative terms), u = fl(1 / t^), r_n = fl(x_n u): sum_n r_n = 1 within gamma(N - 1) + 2 U to first order.  The
    canonical sum over the m members adds at most ceil(m / 64) - 1 additions per accumulator and 6 levels of the tree to every
    non-negative term, the division by m one rounding more; math.fsum over n is exact.  All of it inside gamma(N + ceil(m / 64) + 8).
    A sample that includes no factor has x = +0.0 everywhere: t = 0, u = 0 and every share exactly +0.0."""
    S, K, N, G = 6, 10, 5, 200
    P, E, A = _samples(S, K, N, G, 1, exclude=(3,))
    groups = np.array(([0] * 1 + [1] * 70 + [2] * 129), dtype=np.int32)
    groups = np.random.default_rng(5).permutation(groups)
    ref = R.contrast_reference(P, E, A, groups)
    assert (ref["t"][3] == 0).all() and (np.delete(ref["t"], 3, axis=0) > 0).all()
    for c, m in enumerate(ref["sizes"]):
        bound = _gamma(N + math.ceil(m / 64) + 8)
        for s in range(S):
            tot = math.fsum(ref["series"][1, s, :, c])
            if s == 3:
                assert tot == 0.0 and not np.signbit(ref["series"][1, s, :, c]).any()
                assert (ref["series"][0, s, :, c] == 0).all()
            else:
                assert abs(tot - 1.0) <= bound, (c, s, tot - 1.0, bound)
    assert not np.isnan(ref["series"]).any() and not np.isnan(ref["group"]).any()


def test_prevalence_is_a_count_over_the_group_size():
    S, K, N, G = 5, 10, 4, 150
    P, E, A = _samples(S, K, N, G, 2)
    groups = (np.arange(G) % 3).astype(np.int32)
    groups[::11] = -1
    ref = R.contrast_reference(P, E, A, groups, min_load=20.0)
    assert ref["n_left_out"] == int((groups < 0).sum()) and ref["sizes"].sum() + ref["n_left_out"] == G
    seen = set()
    for c, m in enumerate(ref["sizes"]):
        allowed = np.arange(m + 1) / float(m)
        v2 = ref["series"][2, :, :, c]
        assert np.isin(v2, allowed).all()
        seen |= set(np.unique(v2 * m).round().astype(int).tolist())
    assert len(seen) > 3                                      # (neither all present nor all absent)
    # min_load 0: every load counts, an excluded factor's +0.0 too; a min_load above every load: none does
    assert (R.contrast_reference(P, E, A, groups, min_load=0.0)["series"][2] == 1.0).all()
    assert (R.contrast_reference(P, E, A, groups, min_load=1e300)["series"][2] == 0.0).all()


def test_a_group_of_one_is_its_tumour():
    S, K, N, G = 4, 10, 3, 9
    P, E, A = _samples(S, K, N, G, 3)
    groups = np.array([1, 1, 1, 1, 0, 1, 1, -1, 1], dtype=np.int32)
    ref = R.contrast_reference(P, E, A, groups, min_load=15.0)
    assert ref["sizes"].tolist() == [1, 7]
    assert np.array_equal(ref["series"][0, :, :, 0], ref["x"][:, :, 4])
    assert np.array_equal(ref["series"][1, :, :, 0], ref["r"][:, :, 4])
    assert np.array_equal(ref["series"][2, :, :, 0], ref["b"][:, :, 4].astype(np.float64))


def test_exchanging_two_labels_permutes_the_groups_and_negates_the_pair():
    """Labels 0 and 1 of three exchanged: the group rows and series change places bit for bit; d of the pair (0, 1) changes sign, an exact
    operation, so its mean is negated and its variance kept bit for bit and p_greater / p_less change places; the pairs (0, 2) and
    (1, 2) change places.  lower' = -upper and upper' = -lower hold up to the rounding of the quantile's position: h = (S - 1) p carries
    one rounding, g = h - j is then off by at most U h <= U S, the two products and the sum add 3 roundings: (S + 4) eps max|d|."""
    S, K, N, G = 13, 10, 4, 90
    P, E, A = _samples(S, K, N, G, 4)
    g1 = (np.arange(G) * 7 % 3).astype(np.int32)
    g2 = np.where(g1 == 0, 1, np.where(g1 == 1, 0, g1)).astype(np.int32)
    a, b = R.contrast_reference(P, E, A, g1, 10.0, 0.9), R.contrast_reference(P, E, A, g2, 10.0, 0.9)
    assert a["pairs"] == [(0, 1), (0, 2), (1, 2)]
    perm = [1, 0, 2]
    assert np.array_equal(_bits(b["group"]), _bits(a["group"][:, :, :, perm])) and np.array_equal(_bits(b["series"]), _bits(a["series"][:, :, :, perm]))
    assert np.array_equal(b["sizes"], a["sizes"][perm])
    assert np.array_equal(_bits(b["pair"][:, :, :, 1]), _bits(a["pair"][:, :, :, 2])) and np.array_equal(_bits(b["pair"][:, :, :, 2]), _bits(a["pair"][:, :, :, 1]))
    pa, pb = a["pair"][:, :, :, 0], b["pair"][:, :, :, 0]
    assert np.array_equal(_bits(pb[:, 0]), _bits(-pa[:, 0])) and np.array_equal(_bits(pb[:, 1]), _bits(pa[:, 1]))
    assert np.array_equal(pb[:, 4], pa[:, 5]) and np.array_equal(pb[:, 5], pa[:, 4])
    for q in range(3):
        d = a["series"][q, :, :, 0] - a["series"][q, :, :, 1]
        tol = (S + 4) * 2 * U * np.abs(d).max(axis=0)
        assert (np.abs(pb[q, 2] + pa[q, 3]) <= tol).all() and (np.abs(pb[q, 3] + pa[q, 2]) <= tol).all()
    assert b["n_credible"] == a["n_credible"]


def test_a_planted_difference_is_found_and_an_equal_signature_is_not():
    """Signature 0 at 50 mutations per tumour in group "a" and 10 in group "b", signatures 1 and 2 at 20 and 5 in both; every sample
    jitters the truth by 5 %.  The pair's interval of signature 0 excludes 0 with p_greater 1; the other two are not counted."""
    rng = np.random.default_rng(8)
    S, K, N, G = 40, 6, 3, 60
    groups = (np.arange(G) % 2).astype(np.int32)
    truth = np.stack([np.where(groups == 0, 50.0, 10.0), np.full(G, 20.0), np.full(G, 5.0)])
    Pn = rng.dirichlet(np.ones(K), size=N).T                  # unit column sums: the renormalised exposure is E itself (up to rounding)
    P = np.repeat(Pn[None], S, axis=0)
    E = truth[None] * (1.0 + 0.05 * rng.standard_normal((S, N, G)))
    ref = R.contrast_reference(P, E, np.ones((S, N)), groups, min_load=30.0, credible_interval=0.95)
    load = ref["pair"][0, :, :, 0]
    assert load[2, 0] > 0 and load[4, 0] == 1.0 and load[5, 0] == 0.0 and abs(load[0, 0] - 40.0) < 1.0
    for n in (1, 2):
        assert load[2, n] < 0 < load[3, n] and 0 < load[4, n] < 1
    assert ref["n_credible"][0] == 1
    # prevalence: signature 0 reaches 30 mutations in every tumour of a and in none of b
    assert (ref["series"][2, :, 0, 0] == 1.0).all() and (ref["series"][2, :, 0, 1] == 0.0).all() and ref["pair"][2, 2, 0, 0] == 1.0
    assert ref["n_credible"][2] == 1
    # no interval: NaN bounds, nothing counted
    none = R.contrast_reference(P, E, np.ones((S, N)), groups, min_load=30.0, credible_interval=0.0)
    assert np.isnan(none["group"][:, 2:]).all() and np.isnan(none["pair"][:, 2:4]).all() and none["n_credible"] == [0, 0, 0]
    assert np.array_equal(_bits(none["pair"][:, [0, 1, 4, 5]]), _bits(ref["pair"][:, [0, 1, 4, 5]]))


def test_contrast_labels():
    from bayesnmf_amd.sampler import contrast_labels
    lab, names = contrast_labels(["smoker", None, "never", "smoker", float("nan"), "ex", "never"], 7)
    assert lab.tolist() == [0, -1, 1, 0, -1, 2, 1] and lab.dtype == np.int32 and names == ["smoker", "never", "ex"]
    lab, names = contrast_labels(np.array([3, 3, 1, 3]), 4)
    assert lab.tolist() == [0, 0, 1, 0] and names == [3, 1]
    import pandas as pd
    lab, names = contrast_labels(pd.Series(["x", None, "y"]), 3)
    assert lab.tolist() == [0, -1, 1] and names == ["x", "y"]
    with pytest.raises(ValueError, match="groups has 2 labels for 3 tumours"):
        contrast_labels(["a", "b"], 3)


def test_get_contrast_ranges_idx_and_result(tmp_path):
    """bayesNMF_sampler.get_contrast over a stub engine: the label mapping, the range and idx rules of get_WAIC, the shape of the result"""
    from test_waic_host import _NoWaicEngine
    from bayesnmf_amd.sampler import bayesNMF_sampler
    from bayesnmf_amd.convergence import new_convergence_control
    from bayesnmf_amd.setup import synth_counts

    class _ConEngine(_NoWaicEngine):
        calls = []

        def contrast(self, last_n, groups, used=None, end_iter=None, min_load=1.0, credible_interval=0.95, series=False):
            type(self).calls.append(dict(last_n=last_n, groups=np.array(groups), used=None if used is None else np.array(used), end_iter=end_iter,
                                         min_load=min_load, ci=credible_interval, series=series))
            S = last_n if used is None else int(np.sum(used))
            N, Cn = self.N, int(np.max(groups)) + 1
            pairs = [(a, b) for a in range(Cn) for b in range(a + 1, Cn)]
            out = dict(n_used=S, n_groups=Cn, n_pairs=len(pairs), n_left_out=int((np.asarray(groups) < 0).sum()), n_credible=[2, 1, 0], min_load=min_load,
                       credible_interval=credible_interval, sizes=np.bincount(np.asarray(groups)[np.asarray(groups) >= 0]).astype(np.int32),
                       group=np.arange(3 * 4 * N * Cn, dtype=float).reshape(3, 4, N, Cn), pair=np.arange(3 * 6 * N * len(pairs), dtype=float).reshape(3, 6, N, len(pairs)),
                       pairs=pairs)
            if series:
                out["series"] = np.zeros((3, S, N, Cn))
            return out

    M, _, _ = synth_counts(12, 9, 2, 3, mean_total=200)
    cc = new_convergence_control()
    cc.update(MAP_over=4, MAP_every=2, maxiters=10, miniters=2)
    s = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "r"), engine_factory=_ConEngine,
                         convergence_control=cc, save_all_samples=True, periodic_save=False)
    s.run_gibbs_sampler()
    labels = ["msi", "mss", None, "mss", "msi", "pole", float("nan"), "mss", "msi"]
    msgs, log = [], s.log
    s.log = lambda m, **kw: (msgs.append(m), log(m, **kw))[1]
    r = s.get_contrast(labels)
    c = _ConEngine.calls[-1]
    assert c["last_n"] == 4 and c["end_iter"] is None and c["min_load"] == 1.0 and c["ci"] == 0.95 and not c["series"]
    assert c["groups"].tolist() == [0, 1, -1, 1, 0, 2, -1, 1, 0] and np.array_equal(c["used"], [1, 1, 1, 1])
    assert r["names"] == ["msi", "mss", "pole"] and r["pair_names"] == [("msi", "mss"), ("msi", "pole"), ("mss", "pole")]
    assert r["sizes"].tolist() == [3, 3, 1] and r["n_left_out"] == 2 and r["n_groups"] == 3 and r["n_pairs"] == 3 and r["n_credible"] == [2, 1, 0]
    assert r["n_used"] == 4 and "series" not in r
    g, p = np.arange(3 * 4 * 3 * 3, dtype=float).reshape(3, 4, 3, 3), np.arange(3 * 6 * 3 * 3, dtype=float).reshape(3, 6, 3, 3)
    for q, stat in enumerate(("load", "share", "prevalence")):
        for i, row in enumerate(("mean", "var", "lower", "upper")):
            assert np.array_equal(r[stat][row], g[q, i]), (stat, row)
        for i, row in enumerate(("diff_mean", "diff_var", "diff_lower", "diff_upper", "p_greater", "p_less")):
            assert np.array_equal(r[stat][row], p[q, i]), (stat, row)
    assert msgs == ["Contrast: groups msi (3), mss (3), pole (1); 3 pairs msi - mss, msi - pole, mss - pole; n_credible load 2, share 1, prevalence 0"]
    r = s.get_contrast(np.array([5, 5, 7, 7, 5, 7, 5, 7, 7]), end_iter=8, n_samples=5, idx=[4, 6, 8], min_load=3.0, credible_interval=0.5, series=True)
    c = _ConEngine.calls[-1]
    assert c["end_iter"] == 8 and c["last_n"] == 5 and np.array_equal(c["used"], [1, 0, 1, 0, 1]) and c["min_load"] == 3.0 and c["ci"] == 0.5 and c["series"]
    assert r["names"] == [5, 7] and r["pair_names"] == [(5, 7)] and r["n_used"] == 3 and r["series"].shape == (3, 3, 3, 2) and r["n_left_out"] == 0
    r = s.get_contrast(["a"] * 9, end_iter=8, n_samples=5, idx=None)                        # one group: no pair
    assert _ConEngine.calls[-1]["used"] is None and r["pair_names"] == [] and r["load"]["diff_mean"].shape == (3, 0)
    with pytest.raises(ValueError, match="groups has 3 labels for 9 tumours"):
        s.get_contrast(["a", "b", "a"])
    with pytest.raises(ValueError, match="not all recorded"):
        s.get_contrast(labels, end_iter=12, n_samples=3)
    with pytest.raises(ValueError, match="idx must lie in"):
        s.get_contrast(labels, end_iter=8, n_samples=3, idx=[2])
    s.close()
    t = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "one"), engine_factory=_NoWaicEngine)
    with pytest.raises(ValueError, match="get_contrast needs an engine"):
        t.get_contrast(labels)
    t.close()


def test_new_symbols_declared_exported_and_bound():
    import ctypes as C
    from bayesnmf_amd import engine
    hdr = open(os.path.join(ROOT, "include", "bnmf.h")).read()
    assert re.search(r"typedef struct \{ int32_t n_used, n_groups, n_pairs, n_left_out; int64_t n_credible\[BNMF_CON_NSTAT\];\s*"
                     r"double min_load, credible_interval; \} bnmf_contrast_info;", hdr)
    for name, v in (("MAX_GROUPS", 64), ("NSTAT", 3), ("NGROW", 4), ("NPROW", 6)):
        assert re.search(r"#define BNMF_CON_%s %d\b" % (name, v), hdr), name
    assert re.search(r"#define BNMF_VERSION 100\b", hdr)
    for sym in ("bnmf_contrast", "bnmf_contrast_at"):
        assert re.search(r"\bint\s+%s\s*\(\s*bnmf_handle\s*\*" % sym, hdr), f"{sym} not declared in include/bnmf.h"
        assert sym in engine.ABI_SYMBOLS
    so = os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    L = engine.lib()
    for sym, nargs in (("bnmf_contrast", 11), ("bnmf_contrast_at", 12)):
        assert re.search(r"\bT %s$" % sym, exported, re.M), f"{sym} not exported by libbnmf.so"
        assert len(getattr(L, sym).argtypes) == nargs
    assert C.sizeof(engine.BnmfContrastInfo) == 56 and engine.CON_MAX_GROUPS == 64
    assert hasattr(engine.Engine, "contrast")
    src = open(os.path.join(ROOT, "bayesnmf_amd", "csrc", "contrast.h")).read()
    assert "asm" not in src and "atomic" not in src.lower()
