"""Posterior inference on any recorded range (bnmf_map_at, bnmf_assign_at: get_MAP_(end_iter, n_samples), R/utils.R:194-230) and
the label-switching trace (bnmf_label_switching: plot_label_switching, R/postprocessing_visualizations.R:598-669, whose per-sample
step is hungarian_assignment(keep_all_est = TRUE), R/helpers.R:287-398) against the existing entry points, numpy and scipy."""
import os
import time
from collections import Counter

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL = 1e-12      # fp64 sums in a different association order than numpy's


def _cosmic():
    c = np.load(os.path.join(GOLD, "cosmic_v3.3.1_sbs.npz"))
    return c["P"], [str(x) for x in c["signatures"]]


def _temps(n):
    return np.concatenate([np.zeros(3), 10.0 ** np.linspace(-6, 0, 60), np.ones(n)])


def _engine(model, window, K=96, G=48, N=6, seed=4, data_seed=21, n_temps=1000):
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    M, _, _ = synth_counts(K, G, 3, data_seed)
    prior, MH, lr = dict(gibbs=("gamma", False, False), mh=("truncnormal", True, False), rank=("gamma", False, True))[model]
    e = Engine(M, N, prior=prior, MH=MH, learning_rank=lr, seed=seed, window=window, temperature=_temps(n_temps) if lr else None)
    apply_hyperprior_params(e, prior, M, N)
    e.init()
    return e, M


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_map(a, b):
    for k in ("P", "E", "A", "P_lower", "P_upper", "E_lower", "E_upper", "top_A"):
        if a[k] is None:
            assert b[k] is None, k
            continue
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert np.array_equal(a["used"], b["used"])
    for k in ("top_counts", "n_used", "n_patterns"):
        assert a[k] == b[k], k
    assert _bits(a["rmse"]) == _bits(b["rmse"]) and _bits(a["kl"]) == _bits(b["kl"])


def _same_assign(a, b):
    for k in ("votes", "MAP_cosine", "lower_cosine", "upper_cosine"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert np.array_equal(a["assigned"], b["assigned"])


def _keep(m, model):
    keep = (m["A"].ravel() == 1).astype(np.int32) if model == "rank" else np.ones(m["A"].size, dtype=np.int32)
    if keep.sum() == 0:
        keep[:] = 1
    return keep


@pytest.mark.parametrize("model", ["gibbs", "mh", "rank"])
def test_at_the_current_iteration_is_the_existing_call(model):
    """bnmf_map_at(end_iter = iter, n) / bnmf_assign_at(end_iter = iter, n) are bnmf_map(n) / bnmf_assign(n), bit for bit."""
    ref, _ = _cosmic()
    e, _ = _engine(model, window=100)
    e.run(120, converged=True)
    for n, ci in ((60, 0.95), (100, 0.9), (7, None)):
        m1, m2 = e.map(n, ci), e.map(n, ci, end_iter=e.iter)
        _same_map(m1, m2)
        keep = _keep(m1, model)
        kw = dict(used=m1["used"].astype(np.int32), keep=keep, MAP_P=m1["P"], credible_interval=0.9)
        _same_assign(e.assign(n, ref, **kw), e.assign(n, ref, end_iter=e.iter, **kw))
    e.close()


@pytest.mark.parametrize("model", ["rank", "mh"])
def test_a_past_window_reproduces_what_was_computed_then(model):
    """map(n) and assign(n) saved at iteration t0; 300 iterations later map_at(t0, n) and assign_at(t0, n) give the same bits."""
    ref, _ = _cosmic()
    e, _ = _engine(model, window=400)
    e.run(100, converged=True)
    t0, n = e.iter, 50
    m0 = e.map(n, 0.95)
    kw = dict(used=m0["used"].astype(np.int32), keep=_keep(m0, model), MAP_P=m0["P"], credible_interval=0.9)
    a0 = e.assign(n, ref, **kw)
    e.run(300, converged=True)
    assert e.iter == t0 + 300
    _same_map(m0, e.map(n, 0.95, end_iter=t0))
    _same_assign(a0, e.assign(n, ref, end_iter=t0, **kw))
    e.close()


def _np_map_range(e, end_iter, n, ci, M):
    """get_MAP_(end_iter, n_samples) restated in numpy over slices of Engine.window"""
    back = e.iter - (end_iter - n + 1) + 1
    A, P, E = (e.window(x, back)[:n] for x in ("A", "P", "E"))
    keys = ["".join(str(int(v)) for v in a.ravel()) for a in A]
    tab = sorted(Counter(keys).items(), key=lambda kv: (-kv[1], kv[0]))
    mode = tab[0][0]
    idx = [i for i, k in enumerate(keys) if k == mode]
    Pn = np.stack([P[i] / P[i].sum(0)[None, :] for i in idx], axis=2)
    En = np.stack([E[i] * P[i].sum(0)[:, None] for i in idx], axis=2)
    Am = np.array([float(c) for c in mode])
    pr = [0.5 - ci / 2, 0.5 + ci / 2]
    out = dict(P=Pn.mean(2), E=En.mean(2), A=Am, idx=idx, tab=tab,
               P_lower=np.quantile(Pn, pr[0], axis=2), P_upper=np.quantile(Pn, pr[1], axis=2),
               E_lower=np.quantile(En, pr[0], axis=2), E_upper=np.quantile(En, pr[1], axis=2))
    Mh = (out["P"] * Am[None, :]) @ out["E"]
    out["rmse"] = np.sqrt(((Mh - M) ** 2).mean())
    Mt = np.maximum(M, 1e-6)
    out["kl"] = (Mt * np.log(Mt / np.maximum(Mh, 1e-6))).sum()
    return out


@pytest.mark.parametrize("model", ["rank", "mh"])
def test_a_window_in_the_middle_of_the_chain_matches_numpy(model):
    e, M = _engine(model, window=300)
    e.run(250, converged=True)
    for end_iter, n in ((150, 80), (80, 80), (e.iter - 1, 33)):
        want = _np_map_range(e, end_iter, n, 0.9, M)
        got = e.map(n, 0.9, end_iter=end_iter)
        assert np.array_equal(np.where(got["used"])[0], want["idx"])
        assert np.array_equal(got["A"].ravel(), want["A"])
        assert got["top_counts"] == [c for _, c in want["tab"][:5]]
        for k in ("P", "E", "P_lower", "P_upper", "E_lower", "E_upper"):
            assert np.allclose(got[k], want[k], rtol=RTOL, atol=0), k
        assert np.isclose(got["rmse"], want["rmse"], rtol=1e-10) and np.isclose(got["kl"], want["kl"], rtol=1e-10)
    e.close()


def test_ranges_outside_the_kept_samples_are_refused():
    from bayesnmf_amd.engine import BnmfError
    ref, _ = _cosmic()
    e, _ = _engine("gibbs", window=50)
    e.run(100)                                           # iter 101: iterations 52..101 are kept
    for end_iter, n in ((102, 10), (60, 20), (101, 51)):  # past iter; a start before iter - window + 1
        with pytest.raises(BnmfError, match="52..101") as ei:
            e.map(n, 0.9, end_iter=end_iter)
        assert ei.value.code == -2
        with pytest.raises(BnmfError) as ei:
            e.assign(n, ref, end_iter=end_iter)
        assert ei.value.code == -2
    for iters in ([51], [101, 102], [0]):
        with pytest.raises(BnmfError) as ei:
            e.label_switching(iters, ref)
        assert ei.value.code == -2
    e2, _ = _engine("gibbs", window=500)
    e2.run(20)
    with pytest.raises(BnmfError, match="1..21") as ei:  # a start before iteration 1
        e2.map(10, 0.9, end_iter=5)
    assert ei.value.code == -2
    # both handles keep running
    e.run(5); e2.run(5)
    assert e.map(10, 0.9, end_iter=e.iter - 3)["n_used"] >= 1 and e2.map(10, None)["n_used"] >= 1
    e.close(); e2.close()


def _np_label_switch(P, ref):
    """hungarian_assignment(P, ref, keep_all_est = TRUE) diagonal: (assigned column or -1, cosine or 0.0) per factor"""
    from scipy.optimize import linear_sum_assignment
    rn2 = (ref * ref).sum(0)
    cos = (P.T @ ref) / np.sqrt((P * P).sum(0)[:, None] * rn2[None, :])
    r, c = linear_sum_assignment(-cos)
    asg, cs = np.full(P.shape[1], -1), np.zeros(P.shape[1])
    asg[r], cs[r] = c, cos[r, c]
    return asg, cs


def _check_label_switch(e, iters, ref, got, sample=None):
    back = e.iter - int(np.min(iters)) + 1
    Ps, As = e.window("P", back), e.window("A", back)
    rows = range(len(iters)) if sample is None else sample
    for i in rows:
        P, A = Ps[iters[i] - (e.iter - back + 1)], As[iters[i] - (e.iter - back + 1)]
        asg, cs = _np_label_switch(P, ref)
        assert np.array_equal(got["assigned"][i], asg), (iters[i], got["assigned"][i], asg)
        assert np.allclose(got["cosine"][i], cs, rtol=RTOL, atol=0), iters[i]
        assert np.array_equal(got["included"][i], A.ravel() != 0), iters[i]


def test_label_switching_matches_scipy_on_cosmic():
    """COSMIC v3.3.1 (R = 79), a learned rank of N = 10, every sample of a 300-iteration chain"""
    ref, _ = _cosmic()
    e, _ = _engine("rank", window=400, N=10, G=40)
    e.run(300)
    iters = np.arange(1, e.iter + 1)
    got = e.label_switching(iters, ref)
    assert got["assigned"].shape == got["cosine"].shape == got["included"].shape == (len(iters), 10)
    _check_label_switch(e, iters, ref, got)
    assert got["included"].any() and not got["included"].all()           # the rank was learned: some factors are excluded somewhere
    assert (got["assigned"] >= 0).all()
    # any subset, in any order, gives the same rows
    sub = np.array([300, 7, 150, 7])
    g2 = e.label_switching(sub, ref)
    for k in ("assigned", "cosine", "included"):
        assert np.array_equal(g2[k], got[k][sub - 1]), k
    # more factors than references ("without a reference": reference_P = MAP$P of the kept factors): the rest are "None"
    m = e.map(100, None)
    kept = np.where(m["A"].ravel() == 1)[0]
    refP = m["P"][:, kept] if 0 < len(kept) < 10 else m["P"][:, :6]
    g3 = e.label_switching(iters, refP)
    _check_label_switch(e, iters, refP, g3)
    R = refP.shape[1]
    assert ((g3["assigned"] >= 0).sum(1) == R).all()
    assert (g3["cosine"][g3["assigned"] < 0] == 0.0).all()
    e.close()


def test_label_switching_past_the_lds_takes_the_chunked_path():
    """N R 8 bytes over 160 KiB: k_ref_cosine + k_hungarian in chunks of samples, the same answers.  N = 24, R = 900: 1,553 samples per
    chunk, so the 2,000 samples take two; N = 150 > R = 140: the references are the rows of the assignment, 10 factors get "None"."""
    rng = np.random.default_rng(5)
    ref = rng.dirichlet(np.full(96, 0.3), size=900).T
    assert 24 * 900 * 8 > 160 * 1024
    e, _ = _engine("gibbs", window=2000, N=24, G=32)
    e.run(2000)
    iters = np.arange(2, e.iter + 1)
    got = e.label_switching(iters, ref)
    sample = sorted(set(rng.choice(len(iters), 60, replace=False)) | {0, 1551, 1552, 1553, len(iters) - 1})
    _check_label_switch(e, iters, ref, got, sample)
    ref2 = ref[:, :140]
    assert 150 * 140 * 8 > 160 * 1024
    e2, _ = _engine("gibbs", window=100, N=150, G=16)
    e2.run(20)
    it2 = np.arange(1, e2.iter + 1)
    g2 = e2.label_switching(it2, ref2)
    _check_label_switch(e2, it2, ref2, g2)
    assert ((g2["assigned"] >= 0).sum(1) == 140).all() and (g2["cosine"][g2["assigned"] < 0] == 0.0).all()
    e.close(); e2.close()


@pytest.mark.parametrize("model", ["gibbs", "rank"])
def test_label_switching_cosines_are_the_votes_of_bnmf_assign(model):
    """All factors kept, N <= R: the chosen cosines summed over the used samples in sample order are bnmf_assign's votes, bit for bit"""
    ref, _ = _cosmic()
    e, _ = _engine(model, window=200, N=8)
    e.run(150)
    n = 120
    m = e.map(n, None)
    a = e.assign(n, ref, used=m["used"].astype(np.int32))
    iters = (e.iter - n + 1) + np.where(m["used"])[0]
    ls = e.label_switching(iters, ref)
    votes = np.zeros((8, ref.shape[1]))
    for s in range(len(iters)):
        for k in range(8):
            votes[k, ls["assigned"][s, k]] += ls["cosine"][s, k]
    assert np.array_equal(_bits(votes), _bits(a["votes"]))
    e.close()


def test_label_switching_over_seven_thousand_samples():
    """save_all_samples with the reference's defaults keeps 7,000 samples (maxiters 5,000 + post_warmup 2,000): one call"""
    ref, _ = _cosmic()
    e, _ = _engine("rank", window=7000, N=10, G=16, n_temps=8000)
    e.run(7000)
    iters = np.arange(e.iter - 6999, e.iter + 1)
    e.label_switching(iters[:10], ref)                                   # first call: scratch allocation, kernel attributes
    t = time.perf_counter()
    got = e.label_switching(iters, ref)
    dt = time.perf_counter() - t
    print(f"\nbnmf_label_switching: {len(iters)} samples x N = 10 x R = {ref.shape[1]}: {dt * 1e3:.2f} ms per call")
    rng = np.random.default_rng(1)
    _check_label_switch(e, iters, ref, got, sorted(rng.choice(len(iters), 150, replace=False)))
    e.close()


def test_sampler_get_MAP_on_a_past_range_then_assign_and_label_switching(tmp_path):
    """bayesNMF(save_all_samples = TRUE): get_MAP(end_iter, n_samples, final = TRUE), assign_signatures_ensemble() on that MAP,
    label_switching() — against numpy / scipy"""
    from scipy.optimize import linear_sum_assignment
    from bayesnmf_amd.sampler import bayesNMF
    from bayesnmf_amd.convergence import new_convergence_control
    from bayesnmf_amd.setup import synth_counts
    cosmic, names = _cosmic()
    M, _, _ = synth_counts(96, 40, 3, 8)
    cc = new_convergence_control(MAP_over=50, MAP_every=25, miniters=150, maxiters=200)
    s = bayesNMF(M, range(1, 6), prior="gamma", convergence_control=cc, output_dir=str(tmp_path / "o"), periodic_save=False,
                 save_all_samples=True, seed=2)
    it = s.state["iter"]
    assert it > 160
    e = s._chain
    end_iter, n = 150, 40
    want = _np_map_range(e, end_iter, n, 0.95, M)
    MAP = s.get_MAP(end_iter=end_iter, n_samples=n, final=True)
    keep = np.where(want["A"] == 1)[0]
    assert list(MAP["idx"]) == [end_iter - n + 1 + i for i in want["idx"]]
    assert list(MAP["keep_sigs"]) == list(keep)
    assert np.allclose(MAP["P"], want["P"][:, keep], rtol=RTOL, atol=0) and np.allclose(MAP["E"], want["E"][keep], rtol=RTOL, atol=0)
    assert np.allclose(s.credible_intervals["P"]["lower"], want["P_lower"][:, keep], rtol=RTOL, atol=0)

    res = s.assign_signatures_ensemble(cosmic, reference_names=names)
    Ps = e.window("P", it - (end_iter - n + 1) + 1)
    rn = cosmic / np.linalg.norm(cosmic, axis=0)
    votes, cos_all = np.zeros((s.dims["N"], cosmic.shape[1])), []
    for i in want["idx"]:
        Pk = Ps[i][:, keep]
        cos = (Pk / np.linalg.norm(Pk, axis=0)).T @ rn
        r, c = linear_sum_assignment(-cos)
        votes[keep[r], c] += cos[r, c]
        cos_all.append(cos)
    cos_all = np.stack(cos_all)
    a = res["assignments"]
    assert list(a["sig_est"]) == [int(i) + 1 for i in keep]
    for row, (i, n_) in zip(a.itertuples(), enumerate(keep)):
        j = int(np.argmax(votes[n_]))
        assert row.sig_ref == names[j]
        lo, hi = np.quantile(cos_all[:, i, j], [0.025, 0.975])
        assert np.isclose(row.lower_cosine, lo, rtol=RTOL) and np.isclose(row.upper_cosine, hi, rtol=RTOL)
        mp = MAP["P"][:, i]
        assert np.isclose(row.MAP_cosine, mp @ cosmic[:, j] / np.sqrt((mp @ mp) * (cosmic[:, j] @ cosmic[:, j])), rtol=RTOL)
    assert list(s.reference_comparison["idxs"]) == list(MAP["idx"])
    with pytest.raises(ValueError, match="kept"):
        s.assign_signatures_ensemble(cosmic, idxs=[it + 1])

    df = s.label_switching(cosmic, reference_names=names)
    N = s.dims["N"]
    assert list(df.columns) == ["iter", "estimated", "assigned", "cosine_sim", "k", "included"]
    assert len(df) == it * N and list(df["iter"][:2 * N]) == [1] * N + [2] * N
    assert list(df["estimated"][:N]) == [f"Est{k}" for k in range(1, N + 1)] and list(df["k"][:N]) == list(range(1, N + 1))
    assert s.reference_comparison["label_switching_df"] is df
    Pall, Aall = e.window("P", it), e.window("A", it)
    for t in (1, 77, end_iter, it):
        d = df[df["iter"] == t]
        asg, cs = _np_label_switch(Pall[t - 1], cosmic)
        assert list(d["assigned"]) == [names[j] for j in asg]
        assert np.allclose(d["cosine_sim"], cs, rtol=RTOL, atol=0)
        assert list(d["included"]) == ["Included" if v else "Excluded" for v in Aall[t - 1].ravel() != 0]
    sub = s.label_switching(cosmic, idx=[5, 3])                               # a subset: ordered by iter, not cached
    assert list(sub["iter"]) == [3] * N + [5] * N and s.reference_comparison["label_switching_df"] is df
    none = s.label_switching(MAP["P"])                                      # without a reference: the unmatched factors are "None"
    if len(keep) < N:
        assert (none["assigned"] == "None").any() and (none.loc[none["assigned"] == "None", "cosine_sim"] == 0.0).all()
    assert set(none["assigned"]) <= {f"Ref{j}" for j in range(1, len(keep) + 1)} | {"None"}
    s.close()
