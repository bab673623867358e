"""Decomposition of recorded signatures into a reference catalogue, the parts that need no GPU: the numpy restatement of the spec
(tests/decompose_ref.py) against the laws of the two-stage KL multiplicative update, bayesNMF_sampler.get_decomposition
over a stub engine, and the two new symbols."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import decompose_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps           # 2^-52: twice the unit roundoff u


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _cosmic():
    c = np.load(os.path.join(ROOT, "tests", "golden", "cosmic_v3.3.1_sbs.npz"))
    return np.asarray(c["P"], dtype=np.float64), [str(s) for s in c["signatures"]]


def _problem(S, K, N, R, seed):
    rng = np.random.default_rng(seed)
    ref = rng.gamma(0.5, 1.0, size=(K, R)) + 1e-6              # every cell positive: c > 0 whatever the active set
    mix = rng.dirichlet(np.full(R, 0.3), size=(S, N))          # [S][N][R]
    P = np.einsum("kr,snr->skn", ref / ref.sum(axis=0), mix) * rng.uniform(0.9, 1.1, size=(S, K, N)) * rng.uniform(0.5, 2.0, size=(S, 1, N))
    return P, np.ones((S, N)), ref


def test_disjoint_supports_are_solved_in_one_update():
    """Catalogue columns of pairwise disjoint support and y = a z_i + b z_j: one update from equal weights returns, for every r, the
    part of y on the support of r, T_r = sum_{k in supp r} y[k] (0 for every reference but i and j).  For k in the support of r the
    sum c has one term that is not +0.0, c = fl(z w0): 1 rounding; q = fl(y / c): 1; fl(z q): 1; g_r adds at most K such products in
    at most K additions: K; w0 * g_r: 1.  That is at most K + 4 relative errors of u = 2^-53 each on a sum of positive terms; the bound
    allows twice that for the second-order terms.  T_r is taken from y itself (math.fsum, correctly rounded), so the construction of y
    is not part of the bound.  With min_share = 0.05 below min(a, b) the active set is exactly {i, j}."""
    K, R, S = 30, 5, 3
    rng = np.random.default_rng(1)
    ref = np.zeros((K, R))
    supp = [np.arange(r, K, R) for r in range(R)]              # rows r, r + R, ...: disjoint
    for r in range(R):
        ref[supp[r], r] = rng.gamma(2.0, 1.0, size=len(supp[r]))
    z = D.normalise_catalogue(ref)
    pairs = [(0, 3, 0.6, 0.4), (4, 1, 0.25, 0.75), (2, 0, 0.9, 0.1)]
    P = np.stack([np.stack([a * z[:, i] + b * z[:, j] for i, j, a, b in pairs], axis=1) * sc for sc in (1.0, 3.7, 0.01)])   # [S][K][N]
    y, part = D.columns(P, np.ones((S, len(pairs))))
    assert part.all()
    w, _, _ = D.refit(z, y, 1, 0.0)
    worst = 0.0
    for s in range(S):
        for n, (i, j, a, b) in enumerate(pairs):
            for r in range(R):
                T = math.fsum(y[supp[r], s, n])
                if r in (i, j):
                    worst = max(worst, abs(w[r, s, n] - T) / T)
                    assert abs(T - (a if r == i else b)) < 1e-12
                else:
                    assert T == 0.0 and _bits(w[r, s, n]) == _bits(0.0)
    bound = (K + 4) * EPS
    print(f"largest relative error after one update {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound
    r = D.decompose_reference(P, np.ones((S, len(pairs))), ref, 1, min_share=0.05)
    for n, (i, j, a, b) in enumerate(pairs):
        assert (r["nactive"][:, n] == 2).all()
        assert ((r["weights"][:, :, n] > 0) == np.isin(np.arange(R), (i, j))[None, :]).all()


def test_the_weights_keep_the_total_of_the_column():
    """sum_r w_r g_r = sum_k (y_k / c_k) sum_r z[k,r] w_r = sum_k y_k in exact arithmetic, whatever w was and whichever references are
    active (c holds the active terms only, and every cell of z is positive here, so c > 0).  Every update returns the total, so the
    error is that of the one update: R + 1 roundings in c, 1 in q, 1 in z q, K in g and 1 in w g, K + R + 4; the R additions of the
    check itself and the K of t: (2 K + 2 R + 4) u relative to t.  The bound allows twice that."""
    S, K, N, R, steps = 3, 40, 4, 9, 30
    P, A, ref = _problem(S, K, N, R, 3)
    z = D.normalise_catalogue(ref)
    y, part = D.columns(P, A)
    t = D.total(y)
    tr = []
    _, _, active = D.refit(z, y, steps, 0.1, trace=tr)
    assert len(tr) == 2 * steps and (active.sum(axis=0) < R).any()
    bound = (2 * K + 2 * R + 4) * EPS * t
    worst = 0.0
    for _, w in tr:
        tot = np.zeros((S, N))
        for r in range(R):
            tot = tot + w[r]
        worst = max(worst, float(np.max(np.abs(tot - t) / t)))
        assert (np.abs(tot - t) <= bound).all()
    print(f"largest relative error of the total {worst:.3e}, bound {(2 * K + 2 * R + 4) * EPS:.3e}")


def test_the_kl_divergence_never_increases_in_either_stage():
    """EM: KL(y || z w) = sum_k y log(y / c) - y + c does not increase from one update to the next within a stage (the pruning
    between the stages may raise it: that pair is not compared).  In float64 an evaluation carries the roundings of c (R + 1), of the
    division, the logarithm and the product (3) and of the K + 2 additions, relative to the sum of the magnitudes of its terms: an
    increase of up to 2 (K + R + 5) u mag per evaluated pair is rounding; the bound allows twice that."""
    S, K, N, R, steps = 3, 25, 4, 8, 40
    P, A, ref = _problem(S, K, N, R, 5)
    z = D.normalise_catalogue(ref)
    y, _ = D.columns(P, A)
    tr = []
    D.refit(z, y, steps, 0.1, trace=tr)

    def kl(w):
        c = D.fitted(z, w)
        with np.errstate(all="ignore"):
            term = np.where(y > 0, y * np.log(y / c), 0.0)
        return (term - y + c).sum(axis=0), (np.abs(term) + y + c).sum(axis=0)
    fell = [0, 0]
    for stage in (0, 1):
        ws = [w for st, w in tr if st == stage]
        assert len(ws) == steps
        prev, _ = kl(ws[0])
        for w in ws[1:]:
            cur, mag = kl(w)
            assert (cur <= prev + 2 * (K + R + 5) * EPS * mag).all(), stage
            fell[stage] += int((cur < prev).sum())
            prev = cur
    assert fell[0] > 0 and fell[1] > 0


def test_pruning():
    S, K, N, R, steps = 2, 20, 3, 7, 15
    P, A, ref = _problem(S, K, N, R, 7)
    z = D.normalise_catalogue(ref)
    y, _ = D.columns(P, A)
    tr = []
    w, d, active = D.refit(z, y, steps, 0.1, trace=tr)
    # inactive weights are exactly +0.0 after stage 2, active ones positive; some reference was dropped somewhere
    assert (~active).any() and np.array_equal(_bits(w[~active]), _bits(np.zeros(int((~active).sum())))) and (w[active] > 0).all()
    t = D.total(y)
    w1 = tr[steps - 1][1]
    assert np.array_equal(active, w1 >= (0.1 * t)[None])                                       # (none needed the fallback here)
    # min_share = 0: no pruning, no second stage; the stage-1 weights bit for bit
    w0, d0, a0 = D.refit(z, y, steps, 0.0)
    assert np.array_equal(_bits(w0), _bits(w1)) and a0.all()
    r0 = D.decompose_reference(P, A, ref, steps, min_share=0.0)
    assert (r0["nactive"] == R).all() and np.array_equal(_bits(r0["weights"]), _bits(w0.transpose(1, 0, 2))) and (r0["p_present"] == 1.0).all()
    # none reaches the threshold: the first largest stays, alone
    wf = np.array([0.2, 0.3, 0.3, 0.2])[:, None, None] * np.ones((4, 1, 2))
    act = D.prune(wf, np.ones((1, 2)), 0.5)
    assert np.array_equal(act[:, 0, 0], [False, True, False, False]) and np.array_equal(act[:, 0, 1], [False, True, False, False])
    act = D.prune(np.full((4, 1, 1), 0.25), np.ones((1, 1)), 0.5)
    assert np.array_equal(act[:, 0, 0], [True, False, False, False])
    wl, _, al = D.refit(z, y, steps, 0.999)
    assert (al.sum(axis=0) == 1).all() and np.array_equal(al.argmax(axis=0), w1.argmax(axis=0))
    assert np.allclose(wl.sum(axis=0), t, rtol=(2 * K + 2 * R + 4) * EPS, atol=0)               # the one reference left takes the total


def test_a_planted_cosmic_mixture_is_found():
    """0.6 SBS2 + 0.4 SBS13 against the 79 COSMIC v3.3.1 columns, 200 + 200 steps at min_share = 0.05.  How close the weights and the
    cosine come is not derivable; measured with this restatement: weights 0.6000000000000001 and 0.4 (errors 1.1e-16
    and 0), cosine 1.0, max_rel_change 1.1e-16, 2 references active in both samples: the two signatures barely overlap, so the refit
    is all but exact.  The margins asserted are 1e-6 for the weights and the change and 1e-9 for the cosine: far above the measured
    values (another BLAS-free platform may round differently), far below any confusion with a third reference."""
    ref, names = _cosmic()
    i, j = names.index("SBS2"), names.index("SBS13")
    col = 0.6 * ref[:, i] + 0.4 * ref[:, j]
    P = np.stack([col[:, None] * 1.0, col[:, None] * 5.0])                              # S = 2, N = 1; the scale is renormalised away
    r = D.decompose_reference(P, np.ones((2, 1)), ref, 200, min_share=0.05)
    w = r["weight_mean"][:, 0]
    top = np.argsort(-w, kind="stable")[:2]
    print(f"planted 0.6 SBS2 + 0.4 SBS13: weights {w[i]!r} {w[j]!r}, errors {abs(w[i] - 0.6):.3e} {abs(w[j] - 0.4):.3e}, cosine {r['cosine'][0]!r} "
          f"(1 - {1.0 - r['cosine'][0]:.3e}), max_rel_change {r['max_rel_change']:.3e}, nactive {r['nactive'].ravel().tolist()}")
    assert top.tolist() == [i, j]
    assert abs(w[i] - 0.6) < 1e-6 and abs(w[j] - 0.4) < 1e-6 and r["cosine"][0] > 1.0 - 1e-9 and r["max_rel_change"] < 1e-6
    assert (r["nactive"] == 2).all() and r["n_present"] == 2 and r["p_present"][i, 0] == 1.0 and r["p_present"][j, 0] == 1.0
    assert r["min_cosine_at"] == 0 and r["min_cosine"] == r["cosine"][0] and r["R"] == 79 and r["included"].tolist() == [2]


def test_an_excluded_factor_has_weight_zero_and_is_as_if_deleted():
    S, K, N, R, steps = 4, 20, 6, 5, 12
    P, A, ref = _problem(S, K, N, R, 9)
    A[:, 1] = 0.0                                                # excluded by A in every sample
    P[:, :, 3] = 0.0                                             # a zero column: colsum 0
    A[2, 4] = 0.0; P[2, 4, 4] = np.inf                           # an Inf inside a column that sample 2 excludes
    keep = np.array([1, 1, 1, 1, 1, 0])                          # factor 5 not asked for
    r = D.decompose_reference(P, A, ref, steps, min_share=0.1, keep=keep)
    part = r["part"]
    assert not part[:, [1, 3, 5]].any() and part[:, [0, 2]].all() and part[:, 4].tolist() == [True, True, False, True]
    out = ~part
    assert np.array_equal(_bits(r["weights"].transpose(0, 2, 1)[out]), _bits(np.zeros((int(out.sum()), R))))     # +0.0, not -0.0
    assert np.isnan(r["cosines"][out]).all() and (r["rel_l1s"][out] == 0).all() and (r["changes"][out] == 0).all() and (r["nactive"][out] == 0).all()
    assert np.isfinite(r["weights"]).all() and np.isfinite(r["cosines"][part]).all() and (r["nactive"][part] >= 1).all()
    assert r["included"].tolist() == [4, 0, 4, 0, 3, 0]
    assert np.isnan(r["cosine"][[1, 3, 4, 5]]).all() and np.isfinite(r["cosine"][[0, 2]]).all() and r["min_cosine_at"] in (0, 2)
    # the factors that take part everywhere have the bits of the run without the others
    r2 = D.decompose_reference(P[:, :, [0, 2]], A[:, [0, 2]], ref, steps, min_share=0.1)
    assert np.array_equal(_bits(r["weights"][:, :, [0, 2]]), _bits(r2["weights"])) and np.array_equal(_bits(r["weight"][:, :, [0, 2]]), _bits(r2["weight"]))
    assert np.array_equal(_bits(r["fit"][:, [0, 2]]), _bits(r2["fit"])) and np.array_equal(r["nactive"][:, [0, 2]], r2["nactive"])
    # the moments are numpy's over the per-sample weights
    assert np.allclose(r["weight_mean"], r["weights"].mean(axis=0), rtol=1e-13, atol=1e-300)
    assert np.allclose(r["weight_var"], r["weights"].var(axis=0, ddof=1), rtol=1e-9, atol=1e-300)
    assert np.array_equal(r["p_present"], (r["weights"] >= 0.1).mean(axis=0))


def test_get_decomposition_ranges_idx_and_result(tmp_path):
    """bayesNMF_sampler.get_decomposition over a stub engine: the range and idx rules of get_WAIC (_recorded_range), the shape of the result"""
    from test_waic_host import _NoWaicEngine
    from bayesnmf_amd.sampler import bayesNMF_sampler
    from bayesnmf_amd.convergence import new_convergence_control
    from bayesnmf_amd.setup import synth_counts

    class _DecEngine(_NoWaicEngine):
        calls = []

        def decompose(self, last_n, reference_P, used=None, end_iter=None, keep=None, n_steps=200, min_share=0.05, weights=False):
            type(self).calls.append(dict(last_n=last_n, ref=np.array(reference_P), used=None if used is None else np.array(used), end_iter=end_iter,
                                         keep=keep, n_steps=n_steps, min_share=min_share, weights=weights))
            S = last_n if used is None else int(np.sum(used))
            N, R = self.N, np.shape(reference_P)[1]
            ws = np.arange(S, dtype=float)[:, None, None] + np.zeros((S, R, N))
            pp = np.zeros((R, N)); pp[1, :] = 1.0; pp[3, 0] = 0.5; pp[2, 0] = 0.25
            wm = np.zeros((R, N)); wm[1, :] = 0.3; wm[3, 0] = 0.7
            return dict(n_used=S, n_steps=n_steps, R=R, n_present=4, min_share=min_share, max_rel_change=1e-4, min_cosine=0.9, min_cosine_at=2,
                        weight_mean=wm, weight_var=np.full((R, N), 9.0), share=np.full((R, N), 1.0 / R), p_present=pp,
                        cosine=np.full(N, 0.95), rel_l1=np.full(N, 0.1), rel_change=np.full(N, 1e-4), nactive=np.full((S, N), 2, dtype=np.int32),
                        included=np.full(N, S, dtype=np.int32), weights=ws)

    M, _, _ = synth_counts(12, 9, 2, 3, mean_total=200)
    ref = np.random.default_rng(2).gamma(1.0, 1.0, size=(12, 5))
    cc = new_convergence_control()
    cc.update(MAP_over=4, MAP_every=2, maxiters=10, miniters=2)
    s = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "r"), engine_factory=_DecEngine,
                         convergence_control=cc, save_all_samples=True, periodic_save=False)
    s.run_gibbs_sampler()
    r = s.get_decomposition(ref)
    c = _DecEngine.calls[-1]
    assert c["last_n"] == 4 and c["end_iter"] is None and c["min_share"] == 0.05 and c["n_steps"] == 200 and c["weights"] and c["keep"] is None
    assert np.array_equal(c["used"], [1, 1, 1, 1]) and np.array_equal(c["ref"], ref) and c["ref"].dtype == np.float64
    assert r["n_used"] == 4 and r["n_present"] == 4 and r["R"] == 5 and r["max_rel_change"] == 1e-4 and r["min_cosine_at"] == 2 and r["min_share"] == 0.05
    for k in ("weight_mean", "weight_sd", "share", "p_present", "lower", "upper"):
        assert r[k].shape == (5, 3), k
    assert (r["weight_sd"] == 3.0).all() and r["nactive"].shape == (4, 3) and r["included"].tolist() == [4, 4, 4]
    # quantile type 7 of the 4 values 0, 1, 2, 3 at 0.025 and 0.975
    assert np.allclose(r["lower"], 0.075, rtol=1e-13) and np.allclose(r["upper"], 3.0 - 0.075, rtol=1e-13)
    assert list(r["fit"].columns) == ["cosine", "rel_l1", "max_rel_change"] and len(r["fit"]) == 3
    # per factor the references with p_present >= 0.5, the largest mean weight first; by column without names
    assert r["components"] == [[(3, 0.5, 0.7), (1, 1.0, 0.3)], [(1, 1.0, 0.3)], [(1, 1.0, 0.3)]]
    names = ["a", "b", "c", "d", "e"]
    r = s.get_decomposition(ref, end_iter=8, n_samples=5, idx=[4, 6, 8], n_steps=50, min_share=0.2, keep=[1, 0, 1], credible_interval=0.5, reference_names=names)
    c = _DecEngine.calls[-1]
    assert c["end_iter"] == 8 and c["last_n"] == 5 and np.array_equal(c["used"], [1, 0, 1, 0, 1]) and c["n_steps"] == 50 and c["min_share"] == 0.2
    assert c["keep"] == [1, 0, 1]
    assert r["n_used"] == 3 and r["n_steps"] == 50 and np.allclose(r["lower"], 0.5) and np.allclose(r["upper"], 1.5)
    assert r["components"][0] == [("d", 0.5, 0.7), ("b", 1.0, 0.3)]
    import pandas as pd
    r = s.get_decomposition(pd.DataFrame(ref, columns=["v", "w", "x", "y", "z"]), end_iter=8, n_samples=5, idx=None)
    assert _DecEngine.calls[-1]["used"] is None and r["components"][1] == [("w", 1.0, 0.3)]
    with pytest.raises(ValueError, match="reference_names has 2 entries"):
        s.get_decomposition(ref, reference_names=["a", "b"])
    with pytest.raises(ValueError, match="not all recorded"):
        s.get_decomposition(ref, end_iter=12, n_samples=3)
    with pytest.raises(ValueError, match="idx must lie in"):
        s.get_decomposition(ref, end_iter=8, n_samples=3, idx=[2])
    s.close()
    t = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "one"), engine_factory=_NoWaicEngine)
    with pytest.raises(ValueError, match="get_decomposition needs an engine"):
        t.get_decomposition(ref)
    t.close()


def test_new_symbols_declared_exported_and_bound():
    import ctypes as C
    from bayesnmf_amd import engine
    hdr = open(os.path.join(ROOT, "include", "bnmf.h")).read()
    assert re.search(r"typedef struct \{ int32_t n_used, n_steps, R, _pad; int64_t n_present [^;]*;\s*"
                     r"double min_share, max_rel_change, min_cosine; int64_t min_cosine_at [^}]*; \} bnmf_decompose_info;", hdr)
    assert re.search(r"#define BNMF_DEC_NW 4\b", hdr) and re.search(r"#define BNMF_DEC_NFIT 3\b", hdr) and re.search(r"#define BNMF_DEC_MAX_R 128\b", hdr)
    assert re.search(r"#define BNMF_VERSION 100\b", hdr)
    for sym in ("bnmf_decompose", "bnmf_decompose_at"):
        assert re.search(r"\bint\s+%s\s*\(\s*bnmf_handle\s*\*" % sym, hdr), f"{sym} not declared in include/bnmf.h"
        assert sym in engine.ABI_SYMBOLS
    so = os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    L = engine.lib()
    for sym, nargs in (("bnmf_decompose", 14), ("bnmf_decompose_at", 15)):
        assert re.search(r"\bT %s$" % sym, exported, re.M), f"{sym} not exported by libbnmf.so"
        assert len(getattr(L, sym).argtypes) == nargs
    assert C.sizeof(engine.BnmfDecomposeInfo) == 56
    assert hasattr(engine.Engine, "decompose")
