"""bnmf_summary's numerical spec on the host: the numpy restatement (tests/summary_ref.py) on hand-built rings whose
answers are known by hand and against numpy.quantile, its invariances, the library's host reduction (csrc/reduce_host.h's summary_reduce)
as a stand-alone program under the sanitizers against it bit for bit, bayesNMF_sampler.summary() and summarize_samplers() over a stub
engine, and the new symbols in the header, the library, the ctypes binding and the R shim.  No device."""
import os
import re
import subprocess

import numpy as np
import pytest

import summary_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(_bits(x)[~np.isnan(x)], _bits(y)[~np.isnan(y)])


def _ring(loads, S=2, A=None):
    """S equal samples whose renormalised loads are `loads` [N][G]: P has one row of ones (column sums 1), E the loads"""
    loads = np.asarray(loads, dtype=np.float64)
    N, G = loads.shape
    P = np.ones((S, 1, N))
    E = np.stack([loads] * S)
    return P, E, np.ones((S, N)) if A is None else np.asarray(A, dtype=np.float64)


def test_answers_known_by_hand():
    #            g:  0    1    2    3    4
    loads = [[0.0, 0.5, 0.25, 0.75, 0.125],                        # c = 0
             [0.5, 4.0, 0.25, 0.0, 0.75],                           # c = 1
             [1.0, 2.0, 3.0, 4.0, 10.0],                            # c = m
             [2.0, 2.0, 2.0, 2.0, 2.0]]                             # all tied
    probs = (0.0, 0.25, 0.5, 1.0)
    r = R.summary_reference(*_ring(loads), probs=probs, min_load=1.0)
    ser = dict(zip(r["names"], r["series"][:, 0, :]))
    assert r["n_used"] == 2 and r["n_aligned"] == 2 and r["n_included"] == 5 and r["n_levels"] == 4 and r["n_blocks"] == 1 and r["n_nonfinite"] == 0
    assert ser["prevalence"].tolist() == [0.0, 0.2, 1.0, 1.0]
    assert ser["total"].tolist() == [1.625, 5.5, 20.0, 10.0] and ser["fraction"].tolist() == [1.625 / 37.125, 5.5 / 37.125, 20.0 / 37.125, 10.0 / 37.125]
    assert np.isnan(ser["mean_present"][0]) and ser["mean_present"][1:].tolist() == [4.0, 4.0, 2.0]
    assert ser["load_all_0"].tolist() == [0.0, 0.0, 1.0, 2.0] and ser["load_all_1"].tolist() == [0.75, 4.0, 10.0, 2.0]      # p = 0 and p = 1: the ends
    assert ser["load_all_0.5"].tolist() == [0.25, 0.5, 3.0, 2.0] and ser["load_all_0.25"].tolist() == [0.125, 0.25, 2.0, 2.0]
    for p in ("0", "0.25", "0.5", "1"):
        v = ser["load_present_" + p]
        assert np.isnan(v[0]) and v[1] == 4.0 and v[3] == 2.0                       # c = 0: NaN; c = 1: the one load at every level; ties: the value
    assert [ser["load_present_" + p][2] for p in ("0", "0.25", "0.5", "1")] == [1.0, 2.0, 3.0, 10.0]
    # the shares: tumour 0 holds 0, 0.5, 1, 2 of a total 3.5
    assert ser["share_all_1"][3] == max(2.0 * (1.0 / t) for t in (3.5, 8.5, 5.5, 6.75, 12.875))
    # the rows over two equal samples: the mean is the value, the variance 0, both bounds the value, n_valid 2; c = 0: NaN rows, n_valid 0
    st = dict(zip(r["names"], r["stat"]))
    assert st["load_present_0.5"][:, 2].tolist() == [3.0, 0.0, 3.0, 3.0, 2.0]
    assert np.isnan(st["load_present_0.5"][:4, 0]).all() and st["load_present_0.5"][4, 0] == 0 and st["mean_present"][4, 0] == 0
    assert st["prevalence"][:, 1].tolist() == [0.2, 0.0, 0.2, 0.2, 2.0]


def test_an_excluded_factor_an_infinite_load_and_a_negative_zero():
    loads = np.array([[3.0, 1.0, 2.0], [5.0, 6.0, 7.0], [1.0, np.inf, 2.0]])
    A = np.array([[1.0, 0.0, 1.0], [1.0, 1.0, 1.0]])               # sample 0 excludes factor 1
    r = R.summary_reference(*_ring(loads, A=A), probs=(0.5,), min_load=1.0)
    ser = dict(zip(r["names"], r["series"]))
    assert ser["total"][:, 1].tolist() == [0.0, 18.0] and ser["prevalence"][:, 1].tolist() == [0.0, 1.0] and ser["load_all_0.5"][:, 1].tolist() == [0.0, 6.0]
    assert np.isnan(ser["load_present_0.5"][0, 1]) and ser["load_present_0.5"][1, 1] == 6.0 and ser["share_all_0.5"][0, 1] == 0.0
    assert not np.signbit(ser["load_all_0.5"][0, 1])
    # an infinite load: the factor's order statistics are NaN in every sample that holds it, counted once per (sample, factor); the tumour's
    # total is infinite, u = 1 / inf = 0, so the other factors' shares there are 0 and stay defined
    assert r["n_nonfinite"] == 2 and np.isnan(ser["load_all_0.5"][:, 2]).all() and np.isnan(ser["share_all_0.5"][:, 2]).all()
    assert np.isnan(ser["load_present_0.5"][:, 2]).all() and not np.isnan(ser["share_all_0.5"][:, 0]).any()
    assert ser["prevalence"][:, 2].tolist() == [1.0, 1.0] and np.isinf(ser["total"][:, 2]).all()
    assert (r["stat"][4:, 4, 2] == 0).all() and (r["stat"][:2, 4, 2] == 2).all()
    # -0.0 among the loads: ties carry one pattern, the median of (-0.0, +0.0, +0.0) is +0.0
    z = R.summary_reference(*_ring([[-0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]), probs=(0.0, 0.5), min_load=0.0)
    assert not np.signbit(z["series"][4:, :, 0]).any() and (z["series"][0] == 1.0).all()


def test_against_numpy_quantile_within_the_counted_roundings():
    """map_interp is (1 - g) a + g b, numpy's linear method a + (b - a) g (or its mirror): 1 - g and b - a are one rounding each, the two
    products one each, the sum one: no more than 4 roundings on either side, each at most eps / 2 relative to max(|a|, |b|), so the two
    differ by at most 8 eps max(|a|, |b|) with room to spare.  The bound is from this count, not tuned."""
    rng = np.random.default_rng(3)
    eps = np.finfo(np.float64).eps
    worst = 0.0
    for k in (1, 2, 3, 7, 64, 65, 1000):
        for scale in (1e-3, 1.0, 1e6):
            y = np.sort(rng.gamma(0.7, scale, size=k))
            for p in (0.0, 0.05, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.95, 0.999, 1.0):
                mine, theirs = R.quantile(y, p), float(np.quantile(y, p, method="linear"))
                j = int(np.floor((k - 1) * p))
                big = max(abs(y[j]), abs(y[min(j + 1, k - 1)]))
                worst = max(worst, abs(mine - theirs) / (eps * big))
                assert abs(mine - theirs) <= 8 * eps * big, (k, scale, p, mine, theirs)
    print(f"summary: largest |restatement - numpy.quantile| / (eps max(|a|, |b|)) = {worst:.3g} (bound 8)")


def _random(S=4, K=6, N=3, G=90, seed=1):
    rng = np.random.default_rng(seed)
    P = rng.gamma(0.5, 1.0, size=(S, K, N))
    E = rng.gamma(0.6, 3.0, size=(S, N, G))
    return P, E, np.ones((S, N))


def test_suffix_shuffle_and_perm():
    P, E, A = _random()
    probs = (0.05, 0.5, 0.95)
    r = R.summary_reference(P, E, A, probs=probs, min_load=1.0)
    L = len(probs)
    # the suffix property: load_present is the quantile of the filtered set
    for s in range(4):
        for n in range(3):
            x = r["x"][s, n]
            f = np.sort(x[x >= 1.0])
            assert 0 < f.size < x.size
            for l, p in enumerate(probs):
                assert _same_bits(r["series"][4 + L + l, s, n], R.quantile(f, p))
            assert r["series"][0, s, n] == f.size / x.size
    # order statistics and counts do not depend on the members' order: the same members' values shuffled (with include) give the same order
    # statistics bit for bit (the canonB sums may differ in the last place: they are held to their own order elsewhere)
    inc = np.zeros(90, dtype=np.int32)
    inc[np.random.default_rng(2).permutation(90)[:70]] = 1
    a = R.summary_reference(P, E, A, probs=probs, include=inc, min_load=1.0)
    sh = np.random.default_rng(4).permutation(90)
    b = R.summary_reference(P, E[:, :, sh], A, probs=probs, include=inc[sh], min_load=1.0)
    assert _same_bits(a["series"][4:], b["series"][4:]) and _same_bits(a["series"][0], b["series"][0]) and a["n_included"] == b["n_included"] == 70
    assert np.allclose(a["series"][1:4], b["series"][1:4], rtol=1e-13, atol=0)
    # perm permutes the outputs; a row of -1 leaves the sample out
    pm = np.tile(np.arange(3), (4, 1))
    pm[1] = [2, 0, 1]
    pm[2] = -1
    c = R.summary_reference(P, E, A, probs=probs, perm=pm, min_load=1.0)
    assert c["n_aligned"] == 3 and np.isnan(c["series"][:, 2]).all() and (c["stat"][:, 4] == 3).all()
    assert _same_bits(c["series"][:, 1][:, [2, 0, 1]], r["series"][:, 1]) and _same_bits(c["series"][:, [0, 3]], r["series"][:, [0, 3]])
    for bad in ([0, 0, 1], [0, 1, 3], [-1, 0, 1]):
        pm[1] = bad
        with pytest.raises(R.Refused):
            R.summary_reference(P, E, A, probs=probs, perm=pm)
    for kw in (dict(probs=()), dict(probs=tuple(np.linspace(0, 1, 9))), dict(probs=(0.5, 0.5)), dict(probs=(0.6, 0.5)), dict(probs=(-0.1,)),
               dict(probs=(1.1,)), dict(probs=(float("nan"),)), dict(min_load=-1.0), dict(min_load=float("inf")), dict(credible_interval=1.0),
               dict(include=np.zeros(90, dtype=int)), dict(include=np.full(90, 2))):
        with pytest.raises(R.Refused):
            R.summary_reference(P, E, A, **kw)
    with pytest.raises(R.Refused):
        R.summary_reference(P[:1], E[:1], A[:1])


def test_reduce_under_the_sanitizers_is_the_restatement(tmp_path):
    """csrc/reduce_host.h's summary_reduce (the library's own code), built as a stand-alone program with -fsanitize=address,undefined: a
    clean run, and stat the restatement's bit for bit: NaN runs of every length (0, 1, 2 valid samples), one sample, enough series for
    several threads, with and without an interval"""
    exe = str(tmp_path / "summary_reduce_check")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tools", "summary_reduce_check.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", p.stderr
    for S, N, Q, ci in ((9, 3, 7, 0.9), (1, 1, 7, 0.95), (2, 5, 19, 0.0), (70, 20, 28, 0.5)):
        rng = np.random.default_rng(S + N)
        ser = rng.gamma(1.0, 2.0, size=(Q, S, N))
        ser[rng.random(ser.shape) < 0.2] = np.nan
        ser[0, :, 0] = np.nan                                                         # no valid sample
        if S > 1:
            ser[1, 1:, 0] = np.nan                                                    # one valid sample
            ser[1, 0, 0] = 2.5
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(np.array([S, N, Q], dtype=np.int64).tobytes() + np.array([ci]).tobytes() + ser.tobytes())
        done = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert done.returncode == 0 and done.stderr == "", done.stderr
        out = np.fromfile(dst, dtype=np.float64).reshape(Q, 5, N)
        assert _same_bits(out, R.reduce(ser, ci)), (S, N, Q, ci)
        assert np.isnan(out[0, :4, 0]).all() and out[0, 4, 0] == 0
        if S > 1:
            assert out[1, 0, 0] == 2.5 and np.isnan(out[1, 1, 0]) and out[1, 4, 0] == 1


class _SumEngine:
    """what bayesNMF_sampler needs of an engine to run a fixed-rank chain to its final MAP, with assign and summary; nothing is sampled"""
    calls = []

    def __init__(self, M, N, **kw):
        self.K, self.G = M.shape
        self.N, self.it = N, 0

    def set(self, name, value):
        pass

    def get(self, name):
        shp = dict(P=(self.K, self.N), E=(self.N, self.G), A=(1, self.N), R=(1,)).get(name, (self.K, self.N) if name.endswith("_p") else (self.N, self.G))
        return np.ones(shp)

    def _rows(self, n):
        rows = np.zeros((n, 11))
        rows[:, 0] = np.arange(self.it + 1, self.it + n + 1)
        rows[:, 3] = -100.0 * self.N
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

    def assign(self, last_n, reference_P, used=None, keep=None, MAP_P=None, credible_interval=0.95, end_iter=None):
        N, Rn = self.N, np.asarray(reference_P).shape[1]
        votes = np.zeros((N, Rn))
        asg = np.array([(2 * n + 1) % Rn for n in range(N)], dtype=np.int32)       # factor n -> reference 1, 3, 0 (of 5)
        votes[np.arange(N), asg] = 1.0
        return dict(votes=votes, assigned=asg, MAP_cosine=np.array([0.9, 0.8, 0.7])[:N], lower_cosine=np.full(N, 0.5), upper_cosine=np.full(N, 0.95))

    def summary(self, last_n, probs=(0.5,), include=None, perm=None, min_load=1.0, credible_interval=0.95, used=None, end_iter=None, series=False):
        type(self).calls.append(dict(last_n=last_n, probs=tuple(probs), include=include, perm=perm, min_load=min_load, used=None if used is None else np.array(used),
                                     end_iter=end_iter, series=series, credible_interval=credible_interval))
        N, L = self.N, len(probs)
        st = np.arange((4 + 3 * L) * 5 * N, dtype=np.float64).reshape(4 + 3 * L, 5, N)
        S = last_n if used is None else int(np.sum(used))
        return dict(n_used=S, n_aligned=S, n_included=self.G, n_left_out=0, n_levels=L, n_blocks=1, n_nonfinite=0, min_load=min_load,
                    credible_interval=credible_interval, stat=st, probs=np.asarray(probs, dtype=np.float64), names=R.names(probs))

    def close(self):
        pass


def _sampler(tmp_path, name, K=12, G=9, N=3, seed=3):
    pd = pytest.importorskip("pandas")
    from bayesnmf_amd.sampler import bayesNMF_sampler
    from bayesnmf_amd.convergence import new_convergence_control
    from bayesnmf_amd.setup import synth_counts
    M, _, _ = synth_counts(K, G, 2, seed, mean_total=200)
    cc = new_convergence_control()
    cc.update(MAP_over=4, MAP_every=2, maxiters=10, miniters=2)
    return bayesNMF_sampler(pd.DataFrame(M), N, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / name), engine_factory=_SumEngine,
                            convergence_control=cc, save_all_samples=True, periodic_save=False)


def test_summary_frames_cache_reference_and_summarize_samplers(tmp_path):
    pd = pytest.importorskip("pandas")
    from bayesnmf_amd.sampler import summarize_samplers
    s = _sampler(tmp_path, "a")
    s.run_gibbs_sampler()
    assert s.state["converged"]
    # a MAP built by hand: 3 signatures over 9 tumours
    E = np.array([[0.5, 1.0, 2.0, 3.0, 10.0, 0.0, 0.9, 4.0, 5.0],                   # 6 of 9 carry it: median of 1, 2, 3, 4, 5, 10 = 3.5
                  [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5],                    # none: NaN, 0
                  [7.0, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0]])                   # all: 7, 1
    s.MAP["E"], s.MAP["P"] = E, np.ones((12, 3)) / 12.0
    s.MAP["A"], s.MAP["keep_sigs"] = np.ones((1, 3)), np.arange(3)
    df = s.summary()
    assert list(df.columns) == ["G", "N", "K", "Signature", "Med_Contribution", "Prop_atleast_1"]
    assert df["G"].tolist() == [9] * 3 and df["N"].tolist() == [3] * 3 and df["K"].tolist() == [12] * 3 and df["Signature"].tolist() == [1, 2, 3]
    assert df["Med_Contribution"][0] == 3.5 and np.isnan(df["Med_Contribution"][1]) and df["Med_Contribution"][2] == 7.0
    assert df["Prop_atleast_1"].tolist() == [6 / 9, 0.0, 1.0]
    assert s.summary() is df and s.reference_comparison["summary"] is df            # the cached return
    with pytest.raises(ValueError, match="no catalogue is bundled"):
        s.summary("cosmic")
    # with a catalogue: through assign_signatures_ensemble, the reference's two further columns; names as given
    ref = np.random.default_rng(1).dirichlet(np.ones(12), size=5).T
    names = ["SBS1", "SBS2", "SBS3", "SBS4", "SBS5"]
    dr = s.summary(ref, reference_names=names)
    assert list(dr.columns) == ["G", "N", "K", "Signature", "Med_Contribution", "Prop_atleast_1", "Reference_Signature", "Cosine_Similarity"]
    assert dr["Reference_Signature"].tolist() == ["SBS2", "SBS4", "SBS1"] and dr["Cosine_Similarity"].tolist() == [0.9, 0.8, 0.7]
    assert dr["Med_Contribution"][0] == 3.5 and s.summary(ref) is dr and s.reference_comparison["assignments"] is not None
    assert s.summary(np.ones((5, 2))) is not dr                                      # a reference of the wrong K is set aside, as the reference does
    # after get_summary at min_load 1 with the median among the levels the frame gains the posterior columns
    r = s.get_summary(relabel=False)
    c = _SumEngine.calls[-1]
    assert c["last_n"] == 4 and c["probs"] == (0.05, 0.25, 0.5, 0.75, 0.95) and c["min_load"] == 1.0 and c["perm"] is None and c["end_iter"] is None
    assert set(r["prevalence"]) == {"mean", "var", "lower", "upper", "n_valid"} and r["load_present_0.5"]["mean"].shape == (3,) and len(r["names"]) == 19
    dp = s.summary()
    post = ["Med_Contribution_post", "Med_Contribution_lower", "Med_Contribution_upper", "Prop_atleast_1_post", "Prop_atleast_1_lower", "Prop_atleast_1_upper"]
    assert list(dp.columns) == ["G", "N", "K", "Signature", "Med_Contribution", "Prop_atleast_1"] + post
    q = r["names"].index("load_present_0.5")
    assert dp["Med_Contribution_post"].tolist() == r["stat"][q, 0].tolist() and dp["Prop_atleast_1_upper"].tolist() == r["stat"][0, 3].tolist()
    s.get_summary(relabel=False, probs=(0.25, 0.75))                                 # no median among the levels: the columns go
    assert list(s.summary().columns) == ["G", "N", "K", "Signature", "Med_Contribution", "Prop_atleast_1"]
    s.get_summary(relabel=False, min_load=2.0, include=[1] * 8 + [None], end_iter=8, n_samples=3, idx=[6, 8])
    c = _SumEngine.calls[-1]
    assert c["end_iter"] == 8 and c["last_n"] == 3 and np.array_equal(c["used"], [1, 0, 1]) and np.array_equal(c["include"], [1] * 8 + [0])
    assert "Med_Contribution_post" not in s.summary().columns
    with pytest.raises(ValueError, match="include has 3 values"):
        s.get_summary(include=[1, 1, 1], relabel=False)
    # summarize_samplers: Name, the skipped unfinished sampler, the K mismatch
    t = _sampler(tmp_path, "b", G=7, seed=4)
    t.run_gibbs_sampler()
    u = _sampler(tmp_path, "c", G=7, seed=5)                                         # never run
    both = summarize_samplers(dict(first=s, second=t, third=u))
    assert list(both.columns)[-1] == "Name" and both["Name"].tolist() == ["first (9)"] * 3 + ["second (7)"] * 3 and len(both) == 6
    assert both["Med_Contribution"][0] == 3.5
    w = _sampler(tmp_path, "d", K=10, seed=6)
    with pytest.raises(ValueError, match="same number of variables"):
        summarize_samplers(dict(first=s, other=w))
    for x in (s, t, u, w):
        x.close()


def test_new_symbols_declared_exported_bound_and_refused_without_a_device():
    import ctypes as C
    from bayesnmf_amd import engine
    from bayesnmf_amd import sampler
    hdr = open(os.path.join(ROOT, "include", "bnmf.h")).read()
    for name, val in (("BNMF_SUM_MAX_Q", 8), ("BNMF_SUM_NROW", 5), ("BNMF_SUM_NSCAL", 4)):
        assert re.search(r"#define %s\s+%d\b" % (name, val), hdr), name
    assert re.search(r"#define BNMF_VERSION 100\b", hdr)
    for sym in ("bnmf_summary", "bnmf_summary_at"):
        assert re.search(r"\bint\s+%s\s*\(\s*bnmf_handle\s*\*" % sym, hdr), f"{sym} not declared in include/bnmf.h"
        assert sym in engine.ABI_SYMBOLS
    so = os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    L = engine.lib()
    for sym, nargs in (("bnmf_summary", 12), ("bnmf_summary_at", 13)):
        assert re.search(r"\bT %s$" % sym, exported, re.M), f"{sym} not exported by libbnmf.so"
        assert len(getattr(L, sym).argtypes) == nargs
    assert C.sizeof(engine.BnmfSummaryInfo) == 48
    assert engine.SUM_SCALARS == R.SCALARS and engine.SUM_FAMILIES == R.FAMILIES and engine.SUM_ROWS == R.ROWS and engine.SUM_MAX_Q == R.MAX_Q
    assert hasattr(engine.Engine, "summary") and hasattr(engine.Engine, "summary_at")
    assert all(hasattr(sampler.bayesNMF_sampler, n) for n in ("get_summary", "summary")) and callable(sampler.summarize_samplers)
    assert "summary) is out of" not in sampler.__doc__
    shim = open(os.path.join(ROOT, "r", "bnmf_shim.c")).read()
    for sym in ("C_bnmf_summary", "C_bnmf_summary_at"):
        assert re.search(r'\{"%s", \(DL_FUNC\)&%s, \d\}' % (sym, sym), shim), sym
    # what is refused before the handle is looked at needs no device: a null handle, a null info
    info = engine.BnmfSummaryInfo()
    pr = (C.c_double * 1)(0.5)
    assert L.bnmf_summary(None, 4, None, None, None, 1.0, pr, 1, 0.95, None, None, C.byref(info)) == -1 and b"null" in L.bnmf_last_error()
    assert L.bnmf_summary_at(None, 9, 4, None, None, None, 1.0, pr, 1, 0.95, None, None, None) == -1 and b"bnmf_summary_at" in L.bnmf_last_error()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 29." in design and "bnmf_summary" in design
