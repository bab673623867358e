"""bnmf_tradeoff without a device: the numpy restatement of the spec (tests/tradeoff_ref.py) against numpy.cov / numpy.corrcoef evaluated in
longdouble within a derived bound, its laws bit for bit (symmetry, a set of everything is the total, a set of one, exact negatives, a
constant series, the factor order with perm), the library's host finish (csrc/reduce_host.h) under the sanitizers against it, the
declarations and bindings, get_tradeoff over a stub engine, and what the numbers mean on a chain of the CPU oracle: two near-duplicate
signatures trade mutations, so their pair has the smallest, and a negative, mean correlation."""
import os
import re
import subprocess

import numpy as np
import pytest

import tradeoff_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(_bits(np.nan_to_num(x)), _bits(np.nan_to_num(y)))


def _samples(S, K, G, N, seed):
    rng = np.random.default_rng(seed)
    P = rng.dirichlet(0.3 * np.ones(K), size=(S, N)).transpose(0, 2, 1)
    E = rng.gamma(1.0, 30.0, size=(S, N, G))
    return P, E, np.ones((S, N))


OUT = ("tumour", "pair_at", "pair", "setstat", "dense")
INFO = ("n_used", "n_matched", "n_unmatched", "n_included", "n_left_out", "n_sets", "n_query", "n_traded", "strongest_pair_at", "strongest_pair", "mean_ratio",
        "min_corr")


def _same(a, b, keys=OUT + INFO):
    return [k for k in keys if not _same_bits(a[k], b[k])]


def test_the_restatement_is_numpy_cov_in_longdouble_within_the_derived_bound():
    """The yardstick: numpy.cov and numpy.corrcoef of the aligned exposures in longdouble.  The bound of a covariance, u = 2^-53: the sum
    of S' rounded products of rounded differences, then a division: (S' + 4) u sum|d_j d_l| / (S' - 1); the rounding of mu (S' additions
    and a division: e_j <= (S' + 1) u mean|q_j|) shifts every d_j alike, and since the true differences sum to zero only its second order
    S' e_j e_l / (S' - 1) and its products with the roundings u (e_j sum|d_l| + e_l sum|d_j|) / (S' - 1) remain.  A correlation inherits
    B_jl / sqrt(v_j v_l) + |r| (B_jj / (2 v_j) + B_ll / (2 v_l)) to first order, and 3 u |r| for its own product, root and quotient; 1 % is
    added for the higher orders."""
    worst_c = worst_r = 0.0
    for S, G, N, seed in ((40, 9, 4, 1), (1000, 3, 6, 2), (2, 5, 3, 3), (129, 4, 20, 4)):
        P, E, A = _samples(S, 8, G, N, seed)
        E[:, 1] = 0.7 * E[:, 0] + 0.01 * E[:, 1]                                      # a strongly correlated pair
        E[:, 2] = 1e4 - E[:, 0]                                                        # an exact trade against a large level: cancellation in d
        ref = R.tradeoff_reference(P, E, A)
        q = R.loads(P, E, A).astype(np.longdouble)                                     # [S][N][G]
        for g in range(G):
            x = q[:, :, g]
            cov = np.cov(x.T.astype(np.longdouble), ddof=1).reshape(N, N)
            d = x - x.mean(axis=0)
            ad = np.abs(d).sum(axis=0)
            e = (S + 1) * U * np.abs(x).mean(axis=0)
            B = ((S + 4) * U * (np.abs(d)[:, :, None] * np.abs(d)[:, None, :]).sum(axis=0) + S * e[:, None] * e[None, :]
                 + U * (e[:, None] * ad[None, :] + e[None, :] * ad[:, None])) / (S - 1)
            err = np.abs(ref["cov"][:, :, g].astype(np.longdouble) - cov)
            worst_c = max(worst_c, float((err / B).max()))
            assert (err <= B).all(), (S, g, float((err / B).max()))
            v = np.diag(cov)
            sd = np.sqrt(v[:, None] * v[None, :])
            rr = cov / sd
            Br = 1.01 * (B / sd + np.abs(rr) * (np.diag(B)[:, None] / (2 * v[:, None]) + np.diag(B)[None, :] / (2 * v[None, :])) + 3 * U * np.abs(rr))
            off = ~np.eye(N, dtype=bool)
            got = ref["r"][:, :, g].astype(np.longdouble)
            assert not np.isnan(got[off]).any() and np.isnan(np.diag(got)).all()
            errr = np.abs(got - rr)[off]
            worst_r = max(worst_r, float((errr / Br[off]).max()))
            assert (errr <= Br[off]).all(), (S, g, float((errr / Br[off]).max()))
            cc = np.corrcoef(x.T.astype(np.longdouble)).reshape(N, N)
            assert float(np.abs(cc - rr)[off].max()) < 1e-15                           # (corrcoef is that quotient)
    print(f"tradeoff restatement against longdouble: largest error / bound {worst_c:.3g} (covariance), {worst_r:.3g} (correlation)")


def test_the_laws_of_the_restatement_hold_bit_for_bit():
    S, G, N = 9, 70, 5
    P, E, A = _samples(S, 6, G, N, 7)
    A[3, 4] = 0.0
    every = np.zeros(N, dtype=np.int32)
    ref = R.tradeoff_reference(P, E, A, sets=every, query=[0, 69, 0])
    cov = ref["cov"]
    assert np.array_equal(_bits(cov), _bits(cov.transpose(1, 0, 2))) and np.array_equal(np.isnan(ref["pair"]), np.isnan(ref["pair"].transpose(0, 2, 1)))
    assert _same_bits(ref["pair"], ref["pair"].transpose(0, 2, 1)) and np.isnan(ref["pair"][:, np.arange(N), np.arange(N)]).all()
    # a single set of every signature: its variance of the sum is vt, and row 3 is tumour row 2, bit for bit
    vt = np.zeros(G)
    for j in range(N):
        inner = np.zeros(G)
        for l in range(N):
            inner = inner + cov[j, l]
        vt = vt + inner
    assert _same_bits(ref["setstat"][1, 0], vt) and _same_bits(ref["setstat"][3, 0], ref["tumour"][2])
    # a set of one signature: row 1 == row 2 and row 3 == 1 exactly where defined
    one = np.array([-1, 0, -1, 1, 1], dtype=np.int32)
    r1 = R.tradeoff_reference(P, E, A, sets=one)
    assert _same_bits(r1["setstat"][1, 0], cov[1, 1]) and _same_bits(r1["setstat"][2, 0], cov[1, 1]) and (r1["setstat"][3, 0] == 1.0).all()
    assert _same_bits(r1["setstat"][0, 0], ref["mu"][1]) and _same_bits(r1["tumour"], ref["tumour"]) and r1["n_sets"] == 2
    # dense is the tumour's matrices; a repeated query repeats
    assert _same_bits(ref["dense"][0], ref["dense"][2]) and _same_bits(ref["dense"][1, 0], cov[:, :, 69]) and _same_bits(ref["dense"][1, 1], ref["r"][:, :, 69])
    # row 0 is the smallest defined correlation over j > l and pair_at names it
    r = ref["r"]
    low = np.array([np.nanmin([r[j, l, g] for j in range(N) for l in range(j)]) for g in range(G)])
    assert _same_bits(ref["tumour"][0], low) and (ref["tumour"][1] == N * (N - 1) // 2).all()
    assert all(_bits(r[ref["pair_at"][g] // N, ref["pair_at"][g] % N, g]) == _bits(low[g]) for g in range(G))
    assert ref["n_traded"] == int((low <= -0.5).sum()) and ref["n_unmatched"] == 0 and ref["n_query"] == 3
    # include is the cohort cut down
    inc = np.ones(G, dtype=np.int32)
    inc[[0, 33, 69]] = 0
    keep = np.where(inc == 1)[0]
    full, cut = R.tradeoff_reference(P, E, A, include=inc, sets=one, query=[5]), R.tradeoff_reference(P, E[:, :, keep], A, sets=one, query=[4])
    assert not _same(full, cut, ("pair", "dense", "n_traded", "strongest_pair", "strongest_pair_at", "mean_ratio"))
    assert _same_bits(full["tumour"][:, keep], cut["tumour"]) and np.isnan(full["tumour"][:, inc == 0]).all() and (full["pair_at"][inc == 0] == -1).all()
    assert _same_bits(full["setstat"][:, :, keep], cut["setstat"]) and np.isnan(full["setstat"][:, :, inc == 0]).all() and full["n_left_out"] == 3


def test_exact_negatives_a_constant_series_and_an_excluded_factor():
    S, G, N = 8, 3, 4
    P = np.tile(np.full((4, N), 0.25)[None], (S, 1, 1))                                # column sums exactly 1
    A = np.ones((S, N))
    E = np.zeros((S, N, G))
    w = np.array([-3.0, 1.0, 2.0, -4.0, 4.0, 0.5, -0.5, 0.0])                          # sums to 0: the means are exact
    E[:, 0] = (16.0 + w)[:, None]
    E[:, 1] = (32.0 - w)[:, None]                                                      # the exact negative about its mean
    E[:, 2] = 5.0                                                                      # a constant series
    E[:, 3] = np.arange(S)[:, None] * np.array([1.0, 2.0, 3.0])[None, :]
    A[:, 3] = 0.0                                                                      # excluded by A in every sample: variance 0
    ref = R.tradeoff_reference(P, E, A, sets=np.array([0, 0, 1, -1], dtype=np.int32))
    assert (ref["r"][1, 0] == -1.0).all() and (ref["tumour"][0] == -1.0).all() and (ref["pair_at"] == 1 * N + 0).all() and (ref["tumour"][1] == 1).all()
    for j in (2, 3):
        assert np.isnan(ref["r"][j]).all() and np.isnan(ref["r"][:, j]).all() and (ref["cov"][j, j] == 0).all()
    assert (ref["tumour"][2] == 0.0).all() and ref["mean_ratio"] == 0.0               # the two trade everything: the total does not vary
    assert (ref["setstat"][1, 0] == 0.0).all() and (ref["setstat"][3, 0] == 0.0).all() and (ref["setstat"][0, 0] == 48.0).all()
    assert np.isnan(ref["setstat"][3, 1]).all() and (ref["setstat"][0, 1] == 5.0).all() and (ref["setstat"][2, 1] == 0.0).all()
    assert ref["pair"][1, 1, 0] == G and ref["pair"][0, 1, 0] == -1.0 and ref["pair"][2, 1, 0] == 1.0 and ref["pair"][3, 1, 0] == 0.0
    assert ref["pair"][1, 2, 0] == 0 and np.isnan(ref["pair"][[0, 2, 3], 2, 0]).all() and ref["pair"][4, 2, 0] == 0.0
    assert ref["strongest_pair"] == -1.0 and ref["strongest_pair_at"] == N and ref["n_traded"] == G
    # N = 1: no pair
    one = R.tradeoff_reference(P[:, :, :1], E[:, :1], A[:, :1])
    assert np.isnan(one["tumour"][0]).all() and (one["tumour"][1] == 0).all() and (one["pair_at"] == -1).all() and one["strongest_pair_at"] == -1
    assert np.isnan(one["strongest_pair"]) and (one["tumour"][2] == 1.0).all() and np.isnan(one["pair"]).all()


def test_permuting_the_factors_with_perm_changes_no_bit():
    S, G, N = 7, 11, 5
    P, E, A = _samples(S, 6, G, N, 11)
    A[2, 1] = 0.0
    sets, q = np.array([0, 1, 1, -1, 0], dtype=np.int32), [3, 10]
    base = R.tradeoff_reference(P, E, A, sets=sets, query=q)
    rng = np.random.default_rng(3)
    perm = np.stack([rng.permutation(N) for _ in range(S)]).astype(np.int32)           # aligned place of the sample's factor n
    P2, E2, A2 = np.empty_like(P), np.empty_like(E), np.empty_like(A)
    for s in range(S):                                                                 # factor n of the shuffled sample is the base's factor perm[s][n]
        P2[s], E2[s], A2[s] = P[s][:, perm[s]], E[s][perm[s]], A[s][perm[s]]
    assert not _same(R.tradeoff_reference(P2, E2, A2, perm=perm, sets=sets, query=q), base)
    assert _same(R.tradeoff_reference(P2, E2, A2, sets=sets, query=q), base)           # (without perm it is another matrix)
    # an unmatched sample is left out whole: the bits of the remaining samples
    pm = np.tile(np.arange(N, dtype=np.int32), (S, 1))
    pm[4] = -1
    rest = [s for s in range(S) if s != 4]
    a, b = R.tradeoff_reference(P, E, A, perm=pm, sets=sets, query=q), R.tradeoff_reference(P[rest], E[rest], A[rest], sets=sets, query=q)
    assert not _same(a, b, tuple(k for k in OUT + INFO if k not in ("n_used", "n_unmatched"))) and a["n_unmatched"] == 1 and a["n_matched"] == S - 1
    for bad, code in ((dict(perm=np.zeros((S, N), dtype=np.int32)), -1), (dict(sets=np.array([0, 2, 2, 0, 0])), -1), (dict(sets=np.full(N, -2)), -1),
                      (dict(query=[G]), -1), (dict(min_corr=1.5), -1), (dict(min_corr=float("nan")), -1), (dict(include=np.full(G, 2)), -1),
                      (dict(include=np.zeros(G, dtype=int)), -2), (dict(perm=np.where(np.arange(S)[:, None] == 0, np.arange(N)[None], -1)), -2)):
        with pytest.raises(R.Refused) as e:
            R.tradeoff_reference(P, E, A, **bad)
        assert e.value.code == code, bad
    with pytest.raises(R.Refused):
        R.tradeoff_reference(P[:1], E[:1], A[:1])


def test_finish_under_the_sanitizers_is_the_restatement(tmp_path):
    """csrc/reduce_host.h's tradeoff_finish (the library's own code), built as a stand-alone program with -fsanitize=address,undefined: a
    clean run, and every output and info field the restatement's bit for bit, from the per-member rows and the pairs' sums as the device
    leaves them (formed here by the restatement's own steps): tumours left out at both ends, no sets, N = 1, more than a block of members"""
    exe = str(tmp_path / "tradeoff_reduce_check")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tools", "tradeoff_reduce_check.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", p.stderr
    for S, G, N, sets, left, mc in ((6, 70, 5, [0, 1, 1, -1, 0], [0, 33, 69], 0.5), (3, 9, 1, None, [], 0.0), (4, 1100, 3, [0, 0, 0], [5], 1.0),
                                    (5, 4, 4, [1, 0, -1, 1], [], 0.3)):
        P, E, A = _samples(S, 5, G, N, 5 + N)
        if N > 2:
            A[:, 2] = 0.0                                                              # undefined pairs
            E[:, 1] = 100.0 - E[:, 0]
        inc = np.ones(G, dtype=np.int32)
        inc[left] = 0
        st = None if sets is None else np.array(sets, dtype=np.int32)
        ref = R.tradeoff_reference(P, E, A, include=inc, sets=st, min_corr=mc)
        members, C = ref["members"].astype(np.int32), ref["n_sets"]
        m = len(members)
        r, ok = R.correlations(ref["cov"])
        tum, at, sst = R.per_tumour(ref["mu"], ref["cov"], r, ok, st, C)
        run, cnts = np.zeros((N * N, 2)), np.zeros((N * N, 3), dtype=np.int32)
        for j in range(N):
            for l in range(j):
                run[j * N + l] = float(R.canonB(np.where(ok[j, l], r[j, l], 0.0))), float(R.canonB(ref["cov"][j, l]))
                cnts[j * N + l] = int(ok[j, l].sum()), int((ok[j, l] & (r[j, l] <= -mc)).sum()), int((ok[j, l] & (r[j, l] >= mc)).sum())
        blob = (np.array([m, G, N, C], dtype=np.int64).tobytes() + np.array([mc]).tobytes() + members.tobytes() + at.astype(np.int32).tobytes() + cnts.tobytes()
                + np.ascontiguousarray(tum).tobytes() + np.ascontiguousarray(sst).tobytes() + run.tobytes())
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(blob)
        done = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert done.returncode == 0 and done.stderr == "", done.stderr
        out = np.fromfile(dst, dtype=np.float64)
        tu, pa, pr, ss, info = np.split(out, np.cumsum([3 * G, G, 5 * N * N, 4 * C * G]))
        assert _same_bits(tu.reshape(3, G), ref["tumour"]) and np.array_equal(pa, ref["pair_at"]) and _same_bits(pr.reshape(5, N, N), ref["pair"])
        assert _same_bits(ss.reshape(4, C, G), ref["setstat"])
        names = ("n_included", "n_left_out", "n_traded", "strongest_pair", "strongest_pair_at", "mean_ratio")
        assert _same_bits(info, np.array([float(ref[n]) for n in names])), dict(zip(names, info))


def test_near_duplicate_signatures_trade_mutations_on_an_oracle_chain(tmp_path, oracle_lib):
    """get_tradeoff over the oracle-backed chain of tests/test_abi_host.py (_OracleChain with its host window; tradeoff is the restatement
    over that window).  K = 24, G = 12; the data come from two signatures, the first of them planted twice: the fit with N = 3 has two
    near-duplicate columns that exchange mutations from sample to sample.  200 oracle iterations, the last 100 used.  A condition, not a
    number: the planted pair (the two fitted columns nearest the duplicated signature) has the smallest mean correlation of all pairs,
    and a negative one; the set of the two is better determined than its members taken as independent (ratio < 1)."""
    from test_abi_host import _OracleChain
    from bayesnmf_amd.sampler import bayesNMF_sampler
    from bayesnmf_amd.convergence import new_convergence_control

    class _Chain(_OracleChain):
        def tradeoff(self, last_n, include=None, perm=None, sets=None, query=None, min_corr=0.5, used=None, end_iter=None):
            assert end_iter is None
            sel = [s for s in range(last_n) if used is None or used[s]]
            win = {nm: np.stack([np.asarray(self.window(nm, last_n)[s], dtype=np.float64) for s in sel]) for nm in ("P", "E", "A")}
            return R.tradeoff_reference(win["P"], win["E"], win["A"].reshape(len(sel), -1), include=include, perm=None if perm is None else perm[sel], sets=sets,
                                        query=query, min_corr=min_corr)

    rng = np.random.default_rng(4)
    K, G, N = 24, 12, 3
    sig = rng.dirichlet(0.3 * np.ones(K), size=2).T                                    # K x 2
    M = rng.poisson(sig @ rng.gamma(2.0, 400.0, size=(2, G))).astype(np.int32)
    cc = new_convergence_control()
    cc.update(MAP_over=100, MAP_every=100, maxiters=200, miniters=200)
    s = bayesNMF_sampler(M, N, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "o"), engine_factory=_Chain, convergence_control=cc,
                         save_all_samples=False, periodic_save=False, seed=3)
    s.run_gibbs_sampler()
    Pm = np.mean([p / p.sum(axis=0) for p in s._chain.window("P", 100)], axis=0)
    cos = (Pm / np.linalg.norm(Pm, axis=0)).T @ (sig / np.linalg.norm(sig, axis=0))   # N x 2
    dup = int(np.argmax([np.sort(cos[:, t])[-2] for t in range(2)]))                   # the signature that two fitted columns stand for
    a, b = sorted(np.argsort(cos[:, dup])[-2:].tolist(), reverse=True)
    r = s.get_tradeoff(sets={"dup": [a, b]}, relabel=False, idx=None)
    print(f"tradeoff on the oracle chain: cosines\n{cos.round(3)}\npair rows 0\n{r['pair'][0].round(3)}\nplanted pair ({a}, {b}); set ratio "
          f"{np.asarray(r['setstat'])[3, 0].round(3)}; total ratio {r['tumour'][2].round(3)}")
    assert r["n_used"] == 100 and r["strongest_pair_at"] == a * N + b and r["strongest_pair"] < 0 and r["pair"][0, a, b] == r["strongest_pair"]
    assert (np.asarray(r["setstat"])[3, 0] < 1.0).all() and r["mean_ratio"] < 1.0
    assert list(r["pairs"].columns) == ["j", "l", "mean_corr", "n_defined", "p_negative", "p_positive", "mean_cov"] and len(r["pairs"]) == 3
    assert list(r["sets"].columns) == ["set", "tumour", "mean", "sd_sum", "sd_if_independent", "ratio"] and (r["sets"]["sd_sum"] < r["sets"]["sd_if_independent"]).all()
    s.close()


def test_get_tradeoff_ranges_idx_names_sets_and_frames(tmp_path):
    """bayesNMF_sampler.get_tradeoff over a stub engine: the range and idx rules of get_WAIC (_recorded_range), relabel's perm scattered
    into the range's rows, sets as labels or as a dict, include and query as the sampler passes them on, the frames with the data's names"""
    pd = pytest.importorskip("pandas")
    from test_waic_host import _NoWaicEngine
    from bayesnmf_amd.sampler import bayesNMF_sampler
    from bayesnmf_amd.convergence import new_convergence_control
    from bayesnmf_amd.setup import synth_counts

    class _TrdEngine(_NoWaicEngine):
        calls = []

        def _relabel(self, last_n, used=None, end_iter=None, pivot_P=None, max_rounds=10, aligned=False):
            S = last_n if used is None else int(np.sum(used))
            perm = np.tile(np.arange(self.N, dtype=np.int32)[::-1], (S, 1))
            perm[1] = -1                                                               # the second used sample is unmatched
            return dict(perm=perm, P_mean=np.ones((self.K, self.N)), E_mean=np.ones((self.N, self.G)))

        def tradeoff(self, last_n, include=None, perm=None, sets=None, query=None, min_corr=0.5, used=None, end_iter=None):
            type(self).calls.append(dict(last_n=last_n, include=include, perm=perm, sets=sets, query=query, min_corr=min_corr,
                                         used=None if used is None else np.array(used), end_iter=end_iter))
            S, G, N = last_n if used is None else int(np.sum(used)), self.G, self.N
            C = 0 if sets is None else int(np.max(sets)) + 1
            out = dict(n_used=S, n_matched=S - 1, n_unmatched=1, n_included=G, n_left_out=0, n_sets=C, n_query=0 if query is None else len(query), n_traded=2,
                       strongest_pair_at=2 * N + 1, strongest_pair=-0.75, mean_ratio=0.5, min_corr=min_corr, tumour=np.arange(3.0 * G).reshape(3, G),
                       pair_at=np.full(G, 1 * N + 0, dtype=np.int32), pair=np.arange(5.0 * N * N).reshape(5, N, N), setstat=np.full((4, C, G), 4.0))
            if query is not None:
                out.update(dense=np.zeros((len(query), 2, N, N)), query=np.asarray(query))
            return out

    M, _, _ = synth_counts(12, 9, 2, 3, mean_total=200)
    names = [f"PD{g:03d}" for g in range(9)]
    cc = new_convergence_control()
    cc.update(MAP_over=4, MAP_every=2, maxiters=10, miniters=2)
    s = bayesNMF_sampler(pd.DataFrame(M, columns=names), 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "r"), engine_factory=_TrdEngine,
                         convergence_control=cc, save_all_samples=True, periodic_save=False)
    s.run_gibbs_sampler()
    _TrdEngine.relabel = _TrdEngine._relabel                                           # (only now: the run's own relabelling line needs more of it)
    r = s.get_tradeoff()
    c = _TrdEngine.calls[-1]
    assert c["last_n"] == 4 and c["end_iter"] is None and c["min_corr"] == 0.5 and c["include"] is None and c["query"] is None and c["sets"] is None
    assert np.array_equal(c["used"], [1, 1, 1, 1]) and c["perm"].shape == (4, 3) and (c["perm"][1] == -1).all() and c["perm"][0].tolist() == [2, 1, 0]
    t = r["tumours"]
    assert list(t.columns) == ["tumour", "min_corr", "pair_j", "pair_l", "n_defined", "total_ratio", "included"] and t["tumour"].tolist() == names
    assert np.array_equal(t["min_corr"], r["tumour"][0]) and (t["pair_j"] == 1).all() and (t["pair_l"] == 0).all() and t["included"].all()
    assert r["pairs"][["j", "l"]].values.tolist() == [[1, 0], [2, 0], [2, 1]] and r["pairs"].iloc[2]["mean_corr"] == r["pair"][0, 2, 1] and "sets" not in r
    assert [r[k] for k in ("n_used", "n_matched", "n_unmatched", "n_traded", "strongest_pair")] == [4, 3, 1, 2, -0.75] and r["min_corr"] == 0.5
    inc = [1, 1, None, 1, 0, 1, float("nan"), 1, 1]
    r = s.get_tradeoff(sets={"APOBEC": [0, 2]}, include=inc, query=["PD003", "PD000"], relabel=False, min_corr=0.8, end_iter=8, n_samples=5, idx=[4, 6, 8])
    c = _TrdEngine.calls[-1]
    assert c["end_iter"] == 8 and c["last_n"] == 5 and np.array_equal(c["used"], [1, 0, 1, 0, 1]) and c["min_corr"] == 0.8 and c["perm"] is None
    assert np.array_equal(c["include"], [1, 1, 0, 1, 0, 1, 0, 1, 1]) and np.array_equal(c["query"], [3, 0]) and c["sets"].tolist() == [0, -1, 0]
    assert r["set_names"] == ["APOBEC"] and len(r["sets"]) == 9 and r["sets"].iloc[1].tolist() == ["APOBEC", "PD001", 4.0, 2.0, 2.0, 4.0] and r["query"] == ["PD003", "PD000"]
    assert r["tumours"]["included"].tolist() == [bool(v) for v in c["include"]]
    s.get_tradeoff(sets=[1, 0, -1], end_iter=8, n_samples=5, idx=None, relabel=False)
    assert _TrdEngine.calls[-1]["used"] is None and _TrdEngine.calls[-1]["sets"].tolist() == [1, 0, -1]
    with pytest.raises(ValueError, match="names no tumour"):
        s.get_tradeoff(query=["nobody"], relabel=False)
    with pytest.raises(ValueError, match="is empty or names a signature"):
        s.get_tradeoff(sets={"a": [3]}, relabel=False)
    with pytest.raises(ValueError, match="another set holds"):
        s.get_tradeoff(sets={"a": [0, 1], "b": [1]}, relabel=False)
    with pytest.raises(ValueError, match="sets has 2 labels"):
        s.get_tradeoff(sets=[0, 0], relabel=False)
    with pytest.raises(ValueError, match="include has 3 values"):
        s.get_tradeoff(include=[1, 1, 1], relabel=False)
    with pytest.raises(ValueError, match="not all recorded"):
        s.get_tradeoff(end_iter=12, n_samples=3, relabel=False)
    s.close()
    t = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "one"), engine_factory=_NoWaicEngine)
    with pytest.raises(ValueError, match="get_tradeoff needs an engine"):
        t.get_tradeoff()
    t.close()


def test_new_symbols_declared_exported_bound_and_refused_without_a_device():
    import ctypes as C
    from bayesnmf_amd import engine
    hdr = open(os.path.join(ROOT, "include", "bnmf.h")).read()
    for name, val in (("BNMF_TRD_NTUM", 3), ("BNMF_TRD_NPAIR", 5), ("BNMF_TRD_NSET", 4), ("BNMF_TRD_MAX_C", 32), ("BNMF_TRD_MAX_N", 128)):
        assert re.search(r"#define %s\s+%d\b" % (name, val), hdr), name
    assert re.search(r"#define BNMF_VERSION 100\b", hdr) and "info (sizeof = 64)" in hdr
    for sym in ("bnmf_tradeoff", "bnmf_tradeoff_at"):
        assert re.search(r"\bint\s+%s\s*\(\s*bnmf_handle\s*\*" % sym, hdr), f"{sym} not declared in include/bnmf.h"
        assert sym in engine.ABI_SYMBOLS
    so = os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    L = engine.lib()
    for sym, nargs in (("bnmf_tradeoff", 16), ("bnmf_tradeoff_at", 17)):
        assert re.search(r"\bT %s$" % sym, exported, re.M), f"{sym} not exported by libbnmf.so"
        assert len(getattr(L, sym).argtypes) == nargs
    assert C.sizeof(engine.BnmfTradeoffInfo) == 64 and R.MAX_C == 32 and R.MAX_N == 128 and engine.TRD_MAX_C == 32
    assert engine.TRD_TUMOUR_ROWS == ("min_corr", "n_defined", "total_ratio") and engine.TRD_SET_ROWS == ("mean", "var_sum", "sum_var", "ratio")
    assert engine.TRD_PAIR_ROWS == ("mean_corr", "n_defined", "p_negative", "p_positive", "mean_cov")
    assert hasattr(engine.Engine, "tradeoff") and hasattr(engine.Engine, "tradeoff_at")
    shim = open(os.path.join(ROOT, "r", "bnmf_shim.c")).read()
    for sym in ("C_bnmf_tradeoff", "C_bnmf_tradeoff_at"):
        assert re.search(r'\{"%s", \(DL_FUNC\)&%s, \d\}' % (sym, sym), shim), sym
    # what is refused before the handle is looked at needs no device: a null handle, a null info
    info = engine.BnmfTradeoffInfo()
    rest = (None, None, None, None, 0, None, 0, 0.5, None, None, None, None, None)
    assert L.bnmf_tradeoff(None, 4, *rest, C.byref(info)) == -1 and b"null" in L.bnmf_last_error()
    assert L.bnmf_tradeoff_at(None, 9, 4, *rest, None) == -1 and b"bnmf_tradeoff_at" in L.bnmf_last_error()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 27." in design and "bnmf_tradeoff" in design
