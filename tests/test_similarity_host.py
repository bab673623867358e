"""Similarity of tumours over a recorded range, the parts that need no GPU: the numpy restatement of the spec (tests/similarity_ref.py)
against the matrix form in extended precision inside a derived bound, the cases whose answer can be derived, a planted cohort of two
subtypes, the library's own finish (csrc/reduce_host.h) as a stand-alone program under the sanitizers, bayesNMF_sampler.get_similarity
over a stub engine, the two new symbols and the refusals that need no device.

The bound.  With u = 2^-53 and gamma_n = n u / (1 - n u): the loads x are taken as given by both sides.  dot and nn are sums of N
products from +0.0, each within gamma_N of the exact sum relative to the sum of the absolute values of the terms: for nn that is nn
itself, for dot it is at most sqrt(nn_g nn_h) by Cauchy-Schwarz, so after the division the error of the numerator is at most gamma_N in
the cosine.  The product of the two norms carries 2 gamma_N + u, its square root half of that and u, the division one more u: the
denominator is within gamma_N + 2.5 u relatively, and |c| <= 1.  Together |c - c_exact| <= gamma_(2 N + 3).  Welford's mean: a step is
one subtraction, one product with 1 / s (itself rounded) and one addition on values of magnitude at most 1 + gamma, so it adds at most
4 u, and the step's map mu -> mu + (c - mu) / s is a contraction: the mean over S samples is within gamma_(2 N + 3 + 4 S).  The
variance M2 / (S - 1): moving every c_s by delta moves it by at most (2 |d| delta + delta^2) S / (S - 1) <= 4 delta + 2 delta^2 with
|d| <= 1 and S >= 2, and M2 itself is S sums of products of magnitude <= 1 with 4 roundings each and the final division: within
4 gamma_(2 N + 3 + 4 S) + 2 gamma_(4 S + 1)."""
import os
import re
import subprocess

import numpy as np
import pytest

import similarity_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def gamma(n):
    return n * U / (1.0 - n * U)


def bound_mean(N, S):
    return gamma(2 * N + 3 + 4 * S)


def bound_var(N, S):
    return 4.0 * gamma(2 * N + 3 + 4 * S) + 2.0 * gamma(4 * S + 1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(_bits(x)[~np.isnan(x)], _bits(y)[~np.isnan(y)])


def _samples(S, K, G, N, seed, excluded=True):
    rng = np.random.default_rng(seed)
    P = rng.gamma(0.7, 1.0, size=(S, K, N))
    E = rng.gamma(0.5, 20.0, size=(S, N, G))
    A = np.ones((S, N))
    if excluded and N > 2:
        A[1, N - 1] = 0.0                                    # a sample that excludes a factor
    return P, E, A


def _matrix_form(P, E, A):
    """mean and variance (S - 1 form) of U^T U per sample, U the profiles normalised in extended precision: (m x m) each, longdouble"""
    x = R.loads(P, E, A).astype(np.longdouble)
    S = x.shape[0]
    cs = []
    for s in range(S):
        nrm = np.sqrt((x[s] * x[s]).sum(axis=0))
        Un = x[s] / np.where(nrm > 0, nrm, 1)
        cs.append(Un.T @ Un)
    cs = np.stack(cs)
    mean = cs.sum(axis=0) / S
    return mean, ((cs - mean) ** 2).sum(axis=0) / (S - 1)


ALL = dict(top_k=5, min_cosine=0.9)


@pytest.mark.parametrize("S,G,N", [(6, 23, 5), (2, 9, 1), (12, 70, 20), (4, 5, 40)])
def test_restatement_against_the_extended_precision_matrix_form(S, G, N):
    P, E, A = _samples(S, 8, G, N, 11 + N)
    r = R.similarity_reference(P, E, A, query=np.arange(G), **ALL)
    mean, var = _matrix_form(P, E, A)
    off = ~np.eye(G, dtype=bool)
    em = float(np.abs(r["mean"].astype(np.longdouble) - mean)[off].max())
    ev = float(np.abs(r["var"].astype(np.longdouble) - var)[off].max())
    print(f"S {S} G {G} N {N}: mean off by {em:.3g} (bound {bound_mean(N, S):.3g}), variance by {ev:.3g} (bound {bound_var(N, S):.3g})")
    assert em <= bound_mean(N, S) and ev <= bound_var(N, S)
    # the outputs are those matrices: dense of every tumour is the whole matrix, NaN on the diagonal; symmetric bit for bit
    for t, tab in enumerate(("mean", "var", "p")):
        assert _same_bits(r["dense"][t], np.where(off, r[tab], np.nan)) and _same_bits(r[tab], r[tab].T)
    if N == 1:
        assert (np.abs(r["mean"][off] - 1.0) <= bound_mean(1, S)).all()                     # one factor: every profile is the same direction
        assert (r["p"][off] == 1.0).all() and r["n_similar_pairs"] == G * (G - 1) // 2 and r["n_isolated"] == 0


def test_label_switching_changes_nothing_beyond_the_bound():
    S, K, G, N = 7, 8, 19, 6
    P, E, A = _samples(S, K, G, N, 3)
    rng = np.random.default_rng(5)
    P2, E2, A2 = P.copy(), E.copy(), A.copy()
    for s in range(S):
        perm = rng.permutation(N)                                                            # another permutation for every sample
        P2[s], E2[s], A2[s] = P[s][:, perm], E[s][perm], A[s][perm]
    a, b = R.similarity_reference(P, E, A, **ALL), R.similarity_reference(P2, E2, A2, **ALL)
    off = ~np.eye(G, dtype=bool)
    assert np.abs(a["mean"] - b["mean"])[off].max() <= 2 * bound_mean(N, S)                  # (each side is within the bound of the exact value)
    assert np.abs(a["var"] - b["var"])[off].max() <= 2 * bound_var(N, S)
    assert not _same_bits(a["mean"], b["mean"])                                              # (the order of the sum did change)


def test_permuting_the_tumours_permutes_the_outputs():
    """a pair's values involve its two tumours only, so they move with the tumours bit for bit, and with them the neighbour lists (no
    two means are equal here), the first neighbour's mean and the degree; the typicality is a sum over the member list in its order, so
    it moves within the rounding of a sum of m - 1 terms of magnitude <= 1 + gamma: gamma_m"""
    S, K, G, N = 5, 8, 70, 4
    P, E, A = _samples(S, K, G, N, 8)
    perm = np.random.default_rng(1).permutation(G)
    a = R.similarity_reference(P, E, A, query=np.arange(G), top_k=6, min_cosine=0.8)
    b = R.similarity_reference(P, E[:, :, perm], A, query=np.arange(G), top_k=6, min_cosine=0.8)
    off = a["mean"][~np.eye(G, dtype=bool)]
    assert len(np.unique(off)) == G * (G - 1) // 2, "two pairs with the same mean"
    assert _same_bits(b["dense"], a["dense"][:, perm][:, :, perm])
    assert np.array_equal(perm[b["neighbour_at"]], a["neighbour_at"][perm]) and _same_bits(b["neighbour"], a["neighbour"][:, perm])
    assert _same_bits(b["tumour"][1:], a["tumour"][1:, perm])
    assert np.abs(b["tumour"][0] - a["tumour"][0, perm]).max() <= gamma(G)
    assert (b["n_similar_pairs"], b["n_isolated"]) == (a["n_similar_pairs"], a["n_isolated"])


def test_include_is_the_cohort_without_the_tumours():
    S, K, G, N = 5, 8, 40, 3
    P, E, A = _samples(S, K, G, N, 21)
    inc = np.ones(G, dtype=np.int32)
    inc[[0, 17, 39]] = 0
    keep = np.where(inc == 1)[0]
    a = R.similarity_reference(P, E, A, include=inc, query=[1, 38], top_k=4, min_cosine=0.8)
    b = R.similarity_reference(P, E[:, :, keep], A, query=[0, len(keep) - 1], top_k=4, min_cosine=0.8)
    assert _same_bits(a["tumour"][:, keep], b["tumour"]) and np.isnan(a["tumour"][:, inc == 0]).all()
    assert _same_bits(a["neighbour"][:, keep], b["neighbour"]) and np.isnan(a["neighbour"][:, inc == 0]).all()
    assert np.array_equal(a["neighbour_at"][keep], keep[b["neighbour_at"]]) and (a["neighbour_at"][inc == 0] == -1).all()
    assert _same_bits(a["dense"][:, :, keep], b["dense"]) and np.isnan(a["dense"][:, :, inc == 0]).all()
    for k in ("n_pairs", "n_similar_pairs", "n_isolated", "n_included"):
        assert a[k] == b[k], k
    assert _same_bits(a["mean_similarity"], b["mean_similarity"]) and _same_bits(a["least_typical"], b["least_typical"])
    assert a["least_typical_at"] == keep[b["least_typical_at"]] and a["n_left_out"] == 3 and b["n_left_out"] == 0


def test_conventions_zero_profile_nan_ties_and_unfilled_places():
    S, K, G, N = 4, 8, 12, 3
    P, E, A = _samples(S, K, G, N, 2, excluded=False)
    # a sample in which tumour 4 has no exposure enters as +0.0 against every tumour
    E0 = E.copy()
    E0[2, :, 4] = 0.0
    r = R.similarity_reference(P, E0, A, **ALL)
    assert (r["c"][2, 4, :] == 0.0).all() and not np.signbit(r["c"][2, 4, :]).any() and (r["c"][2, :, 4] == 0.0).all()
    assert not np.isnan(r["mean"]).any() and (r["p"][4, np.arange(G) != 4] <= 0.75).all()
    # a sample that excludes every factor: every cosine of it is +0.0
    A0 = A.copy()
    A0[1] = 0.0
    assert (R.similarity_reference(P, E, A0, **ALL)["c"][1] == 0.0).all()
    # a NaN load: the tumour's means are NaN, so it is listed by nobody and lists nobody; its row of dense is NaN
    En = E.copy()
    En[1, 0, 7] = np.nan
    r = R.similarity_reference(P, En, A, query=[7], top_k=G + 3)
    assert np.isnan(r["mean"][7]).all() and not (r["neighbour_at"] == 7).any() and (r["neighbour_at"][7] == -1).all()
    assert np.isnan(r["neighbour"][:, 7]).all() and np.isnan(r["dense"][:2, 0]).all() and np.isnan(r["tumour"][:2, 7]).all() and r["tumour"][2, 7] == 0
    assert (r["dense"][2, 0, others7 := np.arange(G) != 7] <= 0.75).all()                   # (NaN >= min_cosine is false: the sample is not counted)
    others = np.arange(G) != 7
    assert ((r["neighbour_at"][others] >= 0).sum(axis=1) == G - 2).all()                    # the others list everybody but it
    assert np.isnan(r["tumour"][0]).all() and r["least_typical_at"] == -1 and np.isnan(r["least_typical"])   # its NaN enters every typicality
    assert not np.isnan(r["tumour"][1][others]).any()
    # ties go to the lower tumour: two tumours with the same profile in every sample are equally far from everybody
    Et = E.copy()
    Et[:, :, 9] = Et[:, :, 5]
    r = R.similarity_reference(P, Et, A, top_k=G - 1)
    assert _same_bits(r["mean"][:, 5], r["mean"][:, 9])
    for g in range(G):
        if g not in (5, 9):
            lst = r["neighbour_at"][g].tolist()
            assert lst.index(9) == lst.index(5) + 1, (g, lst)
    # top_k > m - 1: the places behind the m - 1 candidates hold -1 / NaN
    r = R.similarity_reference(P, E, A, top_k=32)
    assert (r["neighbour_at"][:, :G - 1] >= 0).all() and (r["neighbour_at"][:, G - 1:] == -1).all()
    assert not np.isnan(r["neighbour"][:, :, :G - 1]).any() and np.isnan(r["neighbour"][:, :, G - 1:]).all()
    assert (np.diff(r["neighbour"][0, :, :G - 1], axis=1) <= 0).all()                        # the mean descending
    # the queries alone: the same rows, the fields of the pass over all pairs say that it did not run
    full = R.similarity_reference(P, E, A, query=[3, 0, 3], **ALL)
    alone = R.similarity_reference(P, E, A, query=[3, 0, 3], top_k=0, min_cosine=0.9, tumour=False)
    assert _same_bits(full["dense"], alone["dense"]) and "tumour" not in alone
    assert (alone["n_similar_pairs"], alone["n_isolated"], alone["least_typical_at"]) == (-1, -1, -1) and np.isnan(alone["mean_similarity"])


def _planted():
    """40 tumours, the first 20 with signatures 0 - 1 only, the rest with 2 - 3 only; 12 samples: the true exposures under lognormal jitter"""
    rng = np.random.default_rng(20261019)
    S, K, G, N = 12, 10, 40, 4
    E0 = np.zeros((N, G))
    E0[:2, :20] = rng.gamma(2.0, 50.0, size=(2, 20))
    E0[2:, 20:] = rng.gamma(2.0, 50.0, size=(2, 20))
    E = E0[None] * rng.lognormal(0.0, 0.2, size=(S, N, G))
    P = rng.gamma(0.7, 1.0, size=(S, K, N))
    return P, E, np.ones((S, N))


def test_planted_subtypes():
    P, E, A = _planted()
    r = R.similarity_reference(P, E, A, top_k=3, min_cosine=0.9)
    sub = np.arange(40) >= 20
    assert (sub[r["neighbour_at"]] == sub[:, None]).all()                                    # the 3 nearest are of the tumour's own subtype
    cross = r["mean"][:20, 20:]
    assert (cross == 0.0).all() and (r["p"][:20, 20:] == 0.0).all()                          # no shared signature: exactly 0 in every sample
    within = int((r["p"][:20, :20] >= 0.5).sum() - 20 + (r["p"][20:, 20:] >= 0.5).sum() - 20) // 2
    print("similar pairs", r["n_similar_pairs"], "within", within, "isolated", r["n_isolated"], "typicality", r["tumour"][0].round(3))
    assert r["n_similar_pairs"] == within and r["n_similar_pairs"] > 0
    assert (r["tumour"][0] < 20.0 / 39.0).all()                                              # at most the 19 of the own subtype resemble it


def _finish_input(r, G, k):
    """the rows in member order, as the device leaves them, from a restatement's outputs"""
    members = np.asarray(r["members"], dtype=np.int32)
    m = len(members)
    place = np.full(G, -1, dtype=np.int32)
    place[members] = np.arange(m)
    nat = r["neighbour_at"][members]
    nat = np.where(nat >= 0, place[np.where(nat >= 0, nat, 0)], -1).astype(np.int32)
    return members, nat, np.ascontiguousarray(r["neighbour"][:, members]), np.ascontiguousarray(r["tumour"][:, members])


def test_finish_under_the_sanitizers_is_the_restatement(tmp_path):
    """csrc/reduce_host.h's similarity_finish (the library's own code), built as a stand-alone program with -fsanitize=address,undefined:
    a clean run, and the outputs by tumour and the info fields the restatement's bit for bit; edge cases: tumours left out at both ends,
    m = 2, top_k = 0, top_k beyond m - 1, a NaN typicality, more than 64 members, the pass over all pairs not run"""
    exe = str(tmp_path / "similarity_reduce_check")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tools", "similarity_reduce_check.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", p.stderr
    P, E, A = _samples(4, 6, 70, 3, 9)
    inc = np.ones(70, dtype=np.int32)
    inc[[0, 33, 69]] = 0
    En = E.copy()
    En[0, 1, 5] = np.nan
    cases = [dict(P=P, E=E, A=A, include=inc, top_k=4), dict(P=P, E=E, A=A, top_k=0), dict(P=P, E=E[:, :, :2], A=A, top_k=32),
             dict(P=P, E=En[:, :, :9], A=A, top_k=3), dict(P=P, E=E, A=A, top_k=0, query=[2], tumour=False)]
    for kw in cases:
        G, k = kw["E"].shape[2], kw["top_k"]
        ref = R.similarity_reference(kw["P"], kw["E"], kw["A"], include=kw.get("include"), query=kw.get("query"), top_k=k, min_cosine=0.8,
                                     tumour=kw.get("tumour", True))
        ran = "tumour" in ref
        members = np.asarray(ref["members"], dtype=np.int32)
        blob = np.array([len(members), G, k, int(ran)], dtype=np.int64).tobytes() + members.tobytes()
        if ran:
            _, nat, nb, tum = _finish_input(ref, G, k)
            blob += np.ascontiguousarray(nat).tobytes() + nb.tobytes() + tum.tobytes()
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(blob)
        q = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert q.returncode == 0 and q.stderr == "", q.stderr
        out = np.fromfile(dst, dtype=np.float64)
        at, ne, tu, info = np.split(out, np.cumsum([G * k, 3 * G * k, 3 * G]))
        if ran:
            assert np.array_equal(at.reshape(G, k), ref["neighbour_at"]) and _same_bits(ne.reshape(3, G, k), ref["neighbour"])
            assert _same_bits(tu.reshape(3, G), ref["tumour"])
        else:
            assert (at == -1).all() and np.isnan(ne).all() and np.isnan(tu).all()
        assert [int(v) for v in info[[0, 1, 2, 3, 4, 7]]] == [ref[n] for n in ("n_included", "n_left_out", "n_pairs", "n_similar_pairs", "n_isolated", "least_typical_at")]
        assert _same_bits(info[5:7], np.array([ref["mean_similarity"], ref["least_typical"]]))


def test_get_similarity_ranges_idx_names_and_result(tmp_path):
    """bayesNMF_sampler.get_similarity over a stub engine: the range and idx rules of get_WAIC (_recorded_range), the defaults, include
    and query as the sampler passes them on, the tables with the data's column names"""
    pd = pytest.importorskip("pandas")
    from test_waic_host import _NoWaicEngine
    from bayesnmf_amd.sampler import bayesNMF_sampler
    from bayesnmf_amd.convergence import new_convergence_control
    from bayesnmf_amd.setup import synth_counts

    class _SimEngine(_NoWaicEngine):
        calls = []

        def similarity(self, last_n, include=None, query=None, top_k=10, min_cosine=0.9, used=None, end_iter=None, tumour=True):
            type(self).calls.append(dict(last_n=last_n, used=None if used is None else np.array(used), end_iter=end_iter, include=include, query=query,
                                         top_k=top_k, min_cosine=min_cosine))
            S, G = last_n if used is None else int(np.sum(used)), self.G
            nat = np.full((G, top_k), -1, dtype=np.int32)
            nat[:, :2] = [[(g + 1) % G, (g + 2) % G] for g in range(G)]
            out = dict(n_used=S, n_included=G, n_left_out=0, top_k=top_k, n_query=0 if query is None else len(query), n_pairs=G * (G - 1) // 2, n_similar_pairs=4,
                       n_isolated=1, least_typical_at=2, mean_similarity=0.5, least_typical=0.25, min_cosine=min_cosine, neighbour_at=nat,
                       neighbour=np.full((3, G, top_k), 0.25), tumour=np.arange(3.0 * G).reshape(3, G))
            if query is not None:
                out.update(dense=np.zeros((3, len(query), G)), query=np.asarray(query))
            return out

    M, _, _ = synth_counts(12, 9, 2, 3, mean_total=200)
    names = [f"PD{g:03d}" for g in range(9)]
    cc = new_convergence_control()
    cc.update(MAP_over=4, MAP_every=2, maxiters=10, miniters=2)
    s = bayesNMF_sampler(pd.DataFrame(M, columns=names), 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "r"), engine_factory=_SimEngine,
                         convergence_control=cc, save_all_samples=True, periodic_save=False)
    s.run_gibbs_sampler()
    r = s.get_similarity()
    c = _SimEngine.calls[-1]
    assert c["last_n"] == 4 and c["end_iter"] is None and c["top_k"] == 10 and c["min_cosine"] == 0.9 and c["include"] is None and c["query"] is None
    assert np.array_equal(c["used"], [1, 1, 1, 1])
    nb = r["neighbours"]
    assert list(nb.columns) == ["tumour", "rank", "neighbour", "mean", "sd", "p_similar"] and len(nb) == 18              # the -1 places are not listed
    assert nb.iloc[0].tolist() == ["PD000", 1, "PD001", 0.25, 0.5, 0.25] and nb.iloc[17]["neighbour"] == "PD001"
    assert list(r["tumours"].columns) == ["tumour", "typicality", "nearest_mean", "degree", "included"] and r["tumours"]["tumour"].tolist() == names
    assert np.array_equal(r["tumours"]["degree"], r["tumour"][2]) and r["tumours"]["included"].all() and "dense" not in r
    assert [r[k] for k in ("n_used", "n_included", "n_pairs", "n_similar_pairs", "n_isolated", "least_typical_at", "min_cosine")] == [4, 9, 36, 4, 1, 2, 0.9]
    inc = [1, 1, None, 1, 0, 1, float("nan"), 1, 1]
    r = s.get_similarity(include=inc, query=["PD003", "PD000"], top_k=2, min_cosine=0.8, end_iter=8, n_samples=5, idx=[4, 6, 8])
    c = _SimEngine.calls[-1]
    assert c["end_iter"] == 8 and c["last_n"] == 5 and np.array_equal(c["used"], [1, 0, 1, 0, 1]) and c["min_cosine"] == 0.8 and c["top_k"] == 2
    assert np.array_equal(c["include"], [1, 1, 0, 1, 0, 1, 0, 1, 1]) and np.array_equal(c["query"], [3, 0])
    assert r["dense"].shape == (3, 2, 9) and r["query"] == ["PD003", "PD000"] and r["tumours"]["included"].tolist() == [bool(v) for v in c["include"]]
    assert np.array_equal(s.get_similarity(query=[5])["query"], ["PD005"])
    s.get_similarity(end_iter=8, n_samples=5, idx=None)
    assert _SimEngine.calls[-1]["used"] is None
    with pytest.raises(ValueError, match="names no tumour"):
        s.get_similarity(query=["nobody"])
    with pytest.raises(ValueError, match="include has 3 values"):
        s.get_similarity(include=[1, 1, 1])
    with pytest.raises(ValueError, match="other than 0, 1"):
        s.get_similarity(include=[2] * 9)
    with pytest.raises(ValueError, match="not all recorded"):
        s.get_similarity(end_iter=12, n_samples=3)
    with pytest.raises(ValueError, match="Parameter `idx` must be"):
        s.get_similarity(idx="all")
    s.close()
    t = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "one"), engine_factory=_NoWaicEngine)
    assert t.tumour_names is None
    with pytest.raises(ValueError, match="get_similarity needs an engine"):
        t.get_similarity()
    t.close()


def test_new_symbols_declared_exported_bound_and_refused_without_a_device():
    import ctypes as C
    from bayesnmf_amd import engine
    hdr = open(os.path.join(ROOT, "include", "bnmf.h")).read()
    for name, val in (("BNMF_SIM_NNROW", 3), ("BNMF_SIM_NDROW", 3), ("BNMF_SIM_NTUM", 3), ("BNMF_SIM_MAX_K", 32)):
        assert re.search(r"#define %s\s+%d\b" % (name, val), hdr), name
    assert re.search(r"#define BNMF_VERSION 100\b", hdr) and "label switching" in hdr and "the bits of a cohort without them" in hdr
    for sym in ("bnmf_similarity", "bnmf_similarity_at"):
        assert re.search(r"\bint\s+%s\s*\(\s*bnmf_handle\s*\*" % sym, hdr), f"{sym} not declared in include/bnmf.h"
        assert sym in engine.ABI_SYMBOLS
    so = os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    L = engine.lib()
    for sym, nargs in (("bnmf_similarity", 13), ("bnmf_similarity_at", 14)):
        assert re.search(r"\bT %s$" % sym, exported, re.M), f"{sym} not exported by libbnmf.so"
        assert len(getattr(L, sym).argtypes) == nargs
    assert C.sizeof(engine.BnmfSimilarityInfo) == 80 and engine.SIM_MAX_K == 32 == R.MAX_K
    assert hasattr(engine.Engine, "similarity") and hasattr(engine.Engine, "similarity_at")
    # what is refused before the handle is looked at needs no device: a null handle, a null info
    info = engine.BnmfSimilarityInfo()
    assert L.bnmf_similarity(None, 4, None, None, None, 0, 3, 0.9, None, None, None, None, C.byref(info)) == -1 and b"null" in L.bnmf_last_error()
    assert L.bnmf_similarity_at(None, 9, 4, None, None, None, 0, 3, 0.9, None, None, None, None, None) == -1 and b"bnmf_similarity_at" in L.bnmf_last_error()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 24." in design and "bnmf_similarity" in design
