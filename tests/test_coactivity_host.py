"""Co-activity of signatures over a recorded range, the parts that need no GPU: the two new symbols; the numpy restatement of the spec
(tests/coactivity_ref.py) against independent yardsticks — scipy's midranks and Spearman correlation, the exact Pearson
correlation of the same doubles, the 2 x 2 formula in Python integers; the pair numbering, the NaN rules and the n_valid bookkeeping; the
library's own host reduction over the samples, built as a stand-alone program under the address and undefined-behaviour sanitizers and held
to the restatement bit for bit; bayesNMF_sampler.get_coactivity over a stub engine."""
import decimal
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import scipy.stats

import coactivity_ref as R
from regress_ref import BLOCK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53                           # the unit roundoff of float64


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _gamma(k):
    return k * U / (1.0 - k * U)


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(_bits(a)[~na], _bits(b)[~nb])


def _samples(S, K, N, G, seed, exclude=()):
    """non-negative P, heavy-tailed E and 0 / 1 A; `exclude`: (sample, factor) pairs with A = 0"""
    rng = np.random.default_rng(seed)
    P = rng.gamma(0.5, 1.0, size=(S, K, N))
    E = rng.gamma(0.4, 30.0, size=(S, N, G))
    A = np.ones((S, N))
    for s, n in exclude:
        A[s, n] = 0.0
    return P, E, A


def test_new_symbols_declared_exported_and_bound():
    import ctypes as C
    from bayesnmf_amd import engine
    hdr = open(os.path.join(ROOT, "include", "bnmf.h")).read()
    assert re.search(r"typedef struct \{ int32_t n_used, n_included, n_left_out, n_pairs, n_blocks, _pad;\s*int64_t n_credible\[3\];\s*(?:/\*.*?\*/)?\s*"
                     r"int64_t max_cosine_at;\s*(?:/\*.*?\*/)?\s*double max_cosine, min_load, credible_interval; \} bnmf_coactivity_info;", hdr)
    for name, v in (("NSTAT", 4), ("NPROW", 7), ("MAX_M", 1000000)):
        assert re.search(r"#define BNMF_COA_%s\s+%d\b" % (name, v), hdr), name
    assert re.search(r"#define BNMF_VERSION 100\b", hdr)
    for sym in ("bnmf_coactivity", "bnmf_coactivity_at"):
        assert re.search(r"\bint\s+%s\s*\(\s*bnmf_handle\s*\*" % sym, hdr), f"{sym} not declared in include/bnmf.h"
        assert sym in engine.ABI_SYMBOLS
    so = os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    L = engine.lib()
    for sym, nargs in (("bnmf_coactivity", 9), ("bnmf_coactivity_at", 10)):
        assert re.search(r"\bT %s$" % sym, exported, re.M), f"{sym} not exported by libbnmf.so"
        assert len(getattr(L, sym).argtypes) == nargs
    assert C.sizeof(engine.BnmfCoactivityInfo) == 24 + 8 * 3 + 8 + 24 and engine.COA_STATS == list(R.STATS) and engine.COA_PAIR_ROWS == list(R.ROWS)
    assert hasattr(engine.Engine, "coactivity") and hasattr(engine.Engine, "coactivity_at") and R.MAX_M == 1000000 and BLOCK == 1024


def test_midranks_are_scipys_exactly():
    """ties of sizes 2 and 3, a run of zeros of both signs, single values"""
    x = np.array([3.5, 0.0, 1.25, -0.0, 1.25, 7.0, 0.0, 2.0, 2.0, 2.0, 0.0, 9.5, 0.25, -0.0, 4.0])
    sizes = np.unique(x, return_counts=True)[1]
    assert (sizes == 2).any() and (sizes == 3).any() and (x == 0).sum() == 5
    assert np.array_equal(R.midranks(x), scipy.stats.rankdata(x, method="average"))
    c = R.rank_c(x)
    assert c.dtype == np.int64 and np.array_equal(c, (2 * scipy.stats.rankdata(x, method="average") - (x.size + 1)).astype(np.int64)) and (np.abs(c) < x.size).all()
    rng = np.random.default_rng(3)
    for m in (3, 64, 65, 1025):
        y = np.round(rng.gamma(0.4, 4.0, size=m))                                   # heavy ties, many zeros
        assert np.array_equal(R.midranks(y), scipy.stats.rankdata(y, method="average")), m
        assert int(R.rank_c(y).sum()) == 0, m                                       # the centred ranks sum to 0


def test_spearman_agrees_with_scipy_inside_a_derived_bound():
    """The restatement's v1 is exact up to its last operations: T is whole numbers, so the error is the three conversions, the product, the
    root and the quotient, at most 6 roundings relative to |v1| <= 1.  scipy.stats.spearmanr is numpy.corrcoef of the midranks: the
    midranks and their mean are half-integers below 2^53 (exact), each of its three sums of m products has a relative error of at most
    gamma(m + 2) against the sum of the absolute terms, which Cauchy-Schwarz bounds by sqrt(T_aa T_bb); so |v1 - spearmanr| <= 2 gamma(m + 4) +
    8 U.  Not tuned: the largest error over the bound is printed."""
    worst = 0.0
    for G, seed in ((70, 1), (1100, 2)):
        P, E, A = _samples(3, 6, 4, G, seed)
        E = np.round(E)                                                             # ties
        ref = R.coactivity_reference(P, E, A)
        bound = 2.0 * _gamma(G + 4) + 8.0 * U
        for s in range(3):
            for p, (a, b) in enumerate(ref["pairs"]):
                want = scipy.stats.spearmanr(ref["x"][s, a], ref["x"][s, b]).statistic
                err = abs(ref["series"][1, s, p] - want)
                assert err <= bound, (G, s, a, b, err, bound)
                worst = max(worst, err / bound)
    print(f"coactivity host: largest |v1 - spearmanr| / bound {worst:.3g}")


def _exact_pearson(xa, xb):
    """the Pearson correlation of the same doubles in exact arithmetic, the last root at 50 digits"""
    fa, fb = [Fraction(float(v)) for v in xa], [Fraction(float(v)) for v in xb]
    m = len(fa)
    ma, mb = sum(fa) / m, sum(fb) / m
    sab = sum((u - ma) * (v - mb) for u, v in zip(fa, fb))
    saa, sbb = sum((u - ma) ** 2 for u in fa), sum((v - mb) ** 2 for v in fb)
    q = sab * sab / (saa * sbb)
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        r = (decimal.Decimal(q.numerator) / decimal.Decimal(q.denominator)).sqrt()
    return float(r) * (1.0 if sab >= 0 else -1.0), float(ma), float(saa)


def _pearson_bound(m, ratio_a, ratio_b):
    """|v0 - exact| for the restatement's route.  k = the roundings a term of canonB passes through (test_regress_host's
    count).  The computed mean is off by e_n with |e_n| <= gamma(k + 1) mean|x_n|; the exact deviations sum to 0, so shifting them all by e_n
    changes S_ab by m e_a e_b only, second order: relative to sqrt(S_aa S_bb) that is gamma(k + 1)^2 rho_a rho_b with rho_n = mean|x_n| / sd_n
    (sd in the m form).  The roundings of the two subtractions, the product and the sum give gamma(k + 4) sum|d_a d_b| <= gamma(k + 4)
    sqrt(S_aa S_bb).  So S_ab / sqrt(S_aa S_bb) is off by eps_ab = gamma(k + 4) + gamma(k + 1)^2 rho_a rho_b, S_aa and S_bb by eps_aa, eps_bb
    relative; the product, the root and the quotient add 3 roundings: |v0 - r| <= (eps_ab + (eps_aa + eps_bb) / 2 + 4 U) (1 + 0.01)."""
    k = 1 + BLOCK // 64 + 6 + (m + BLOCK - 1) // BLOCK
    g1, g4 = _gamma(k + 1), _gamma(k + 4)
    eps = lambda ra, rb: g4 + g1 * g1 * ra * rb
    return 1.01 * (eps(ratio_a, ratio_b) + 0.5 * (eps(ratio_a, ratio_a) + eps(ratio_b, ratio_b)) + 4.0 * U)


def test_pearson_agrees_with_the_exact_value_inside_a_derived_bound():
    """two cohorts (one block; two blocks), one of them shifted far from 0 so that |mean| / sd is large"""
    worst = 0.0
    for G, seed, shift in ((300, 1, 0.0), (1100, 2, 0.0), (300, 3, 1.0e6)):
        P, E, A = _samples(2, 6, 3, G, seed)
        ref = R.coactivity_reference(P, E + shift, A)
        for s in range(2):
            for p, (a, b) in enumerate(ref["pairs"]):
                xa, xb = ref["x"][s, a], ref["x"][s, b]
                want, _, _ = _exact_pearson(xa, xb)
                ra, rb = np.abs(xa).mean() / xa.std(), np.abs(xb).mean() / xb.std()
                bound = _pearson_bound(G, ra, rb)
                err = abs(ref["series"][0, s, p] - want)
                assert err <= bound, (G, shift, s, a, b, err, bound)
                worst = max(worst, err / bound)
                assert abs(ref["series"][0, s, p] - np.corrcoef(xa, xb)[0, 1]) <= bound + 2.0 * _gamma(G + 4) * (1.0 + ra * rb)   # numpy as a second witness
    print(f"coactivity host: largest |v0 - exact| / bound {worst:.3g}")


def test_phi_is_the_two_by_two_formula_in_python_integers():
    P, E, A = _samples(3, 6, 4, 200, 5)
    for ml in (0.0, 1.0, 8.0, 1.0e9):
        ref = R.coactivity_reference(P, E, A, min_load=ml)
        for s in range(3):
            for p, (a, b) in enumerate(ref["pairs"]):
                ba, bb = ref["x"][s, a] >= ml, ref["x"][s, b] >= ml
                n11, n10, n01, n00 = int((ba & bb).sum()), int((ba & ~bb).sum()), int((~ba & bb).sum()), int((~ba & ~bb).sum())
                den = (n11 + n10) * (n01 + n00) * (n11 + n01) * (n10 + n00)
                got = ref["series"][2, s, p]
                if den == 0:
                    assert np.isnan(got)
                else:
                    q = Fraction(n11 * n00 - n10 * n01) ** 2 / den
                    want = float(np.sqrt(float(q))) * (1.0 if n11 * n00 >= n10 * n01 else -1.0)
                    assert abs(got - want) <= 8.0 * U, (ml, s, a, b, got, want)
    assert np.isnan(R.coactivity_reference(P, E, A, min_load=1.0e9)["series"][2]).all()     # nobody is present: a margin is 0


@pytest.mark.filterwarnings("ignore:invalid value encountered")      # the load that is not finite, through the shared restatement of the loads
def test_pair_numbering_nan_rules_and_n_valid():
    S, K, N, G = 6, 5, 4, 40
    P, E, A = _samples(S, K, N, G, 7, exclude=((1, 2), (4, 2), (4, 0)))
    E[3, 1, :] = 2.5                                                                # a constant factor: no variance, no rank spread
    E[5, 3, 7] = np.inf                                                             # a load that is not finite
    ref = R.coactivity_reference(P, E, A, credible_interval=0.8)
    pairs = ref["pairs"]
    assert pairs == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)] and ref["n_pairs"] == 6 and ref["n_blocks"] == 1 and ref["n_included"] == G
    ser, pair = ref["series"], ref["pair"]
    for p, (a, b) in enumerate(pairs):
        for s in range(S):
            out = A[s, a] == 0 or A[s, b] == 0
            const = s == 3 and 1 in (a, b)
            inf = s == 5 and 3 in (a, b)
            assert np.isnan(ser[3, s, p]) == out                                    # the cosine: NaN where A excludes a or b, only there
            assert np.isnan(ser[0, s, p]) == (out or inf) or const, (s, a, b)       # an excluded factor has S_nn = 0; inf - inf is NaN (a constant one: its rounded mean decides)
            assert np.isnan(ser[1, s, p]) == (out or const or inf), (s, a, b)       # an excluded or constant factor has T_nn = 0; the flag of the factor that is not finite
        for q in range(4):
            v = ser[q, :, p]
            ok = v[~np.isnan(v)]
            assert pair[q, 6, p] == ok.size and ok.size >= 2
            assert pair[q, 4, p] == (ok > 0).sum() / ok.size and pair[q, 5, p] == (ok < 0).sum() / ok.size
            assert abs(pair[q, 0, p] - ok.mean()) <= 4 * U * np.abs(ok).sum() and pair[q, 2, p] <= pair[q, 0, p] <= pair[q, 3, p]
            assert abs(pair[q, 1, p] - ok.var(ddof=1)) <= 1e-12
            assert np.allclose([pair[q, 2, p], pair[q, 3, p]], np.quantile(ok, [0.1, 0.9]), rtol=1e-13, atol=1e-14)
    assert pair[3, 6, pairs.index((0, 2))] == S - 2 and pair[3, 6, pairs.index((1, 3))] == S
    # the symmetric statistics do not care which factor is called a: swapping two columns of the chain permutes the pairs
    perm = [1, 0, 2, 3]
    swapped = R.coactivity_reference(P[:, :, perm], E[:, perm], A[:, perm], credible_interval=0.8)
    for p, (a, b) in enumerate(pairs):
        p2 = pairs.index(tuple(sorted((perm.index(a), perm.index(b)))))
        assert _same_bits(swapped["series"][:, :, p2], ser[:, :, p])
    # one valid sample: a mean, no variance; none: six NaN rows and n_valid 0
    one = R.reduce(np.array([[[0.5], [np.nan], [np.nan]]] * 4), 0.9)[0]
    assert one[0, 0, 0] == 0.5 and np.isnan(one[0, 1, 0]) and one[0, 2, 0] == 0.5 and one[0, 3, 0] == 0.5 and one[0, 6, 0] == 1
    none = R.reduce(np.full((4, 3, 2), np.nan), 0.9)
    assert np.isnan(none[0][:, :6]).all() and (none[0][:, 6] == 0).all() and none[1] == [0, 0, 0] and none[2] == -1 and np.isnan(none[3])
    # the refusals of the restatement carry the ABI's codes
    for kw, code in ((dict(min_load=-1.0), -1), (dict(min_load=np.nan), -1), (dict(credible_interval=1.0), -1), (dict(include=np.r_[1, 1, np.zeros(G - 2)]), -2),
                     (dict(include=np.r_[2, np.ones(G - 1)]), -1)):
        with pytest.raises(R.Refused) as ex:
            R.coactivity_reference(P, E, A, **kw)
        assert ex.value.code == code, kw
    with pytest.raises(R.Refused):
        R.coactivity_reference(P[:, :, :1], E[:, :1], A[:, :1])
    with pytest.raises(R.Refused):
        R.coactivity_reference(P[:1], E[:1], A[:1])


def test_leaving_tumours_out_is_a_chain_without_them():
    P, E, A = _samples(3, 5, 3, 1100, 9)
    inc = np.zeros(1100, dtype=np.int32)
    inc[np.random.default_rng(1).permutation(1100)[:1025]] = 1
    a = R.coactivity_reference(P, E, A, include=inc)
    b = R.coactivity_reference(P, E[:, :, inc == 1], A)
    assert a["n_blocks"] == 2 and a["n_left_out"] == 75 and _same_bits(a["series"], b["series"]) and _same_bits(a["pair"], b["pair"])
    # q0, q1 and q3 do not see min_load
    c = R.coactivity_reference(P, E, A, include=inc, min_load=30.0)
    assert _same_bits(a["series"][[0, 1, 3]], c["series"][[0, 1, 3]]) and not _same_bits(a["series"][2], c["series"][2])


def test_host_reduction_under_the_sanitizers_is_the_restatement(tmp_path):
    """csrc/reduce_host.h's coactivity_reduce (the library's own code: con_rows, con_canon64, the thread pool), built as a stand-alone
    program with -fsanitize=address,undefined: a clean run, and every row and count the restatement's bit for bit"""
    exe = str(tmp_path / "coactivity_reduce_check")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tools", "coactivity_reduce_check.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", p.stderr
    rng = np.random.default_rng(4)
    for S, NP, ci in ((9, 190, 0.9), (2, 1, 0.95), (70, 10, 0.0), (130, 36, 0.5)):
        ser = rng.standard_normal((4, S, NP)) * 0.4
        ser[rng.uniform(size=ser.shape) < 0.2] = np.nan
        ser[:, :, 0] = np.nan if NP > 1 else ser[:, :, 0]                           # a pair without a valid sample
        if NP > 2:
            ser[:, 1:, 1] = np.nan                                                  # a pair with one
            ser[0, :, 2] = 0.0                                                      # neither greater nor less
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(np.array([S, NP], dtype=np.int64).tobytes() + np.array([ci]).tobytes() + np.ascontiguousarray(ser).tobytes())
        q = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert q.returncode == 0 and q.stderr == "", q.stderr
        out = np.fromfile(dst, dtype=np.float64)
        pair, n_credible, at, mx = R.reduce(ser, ci)
        assert _same_bits(out[:-5].reshape(4, 7, NP), pair), (S, NP, ci)
        assert [int(v) for v in out[-5:-2]] == n_credible and int(out[-2]) == at and _same_bits(out[-1:], np.array([mx]))


class _StubEngine:
    """an engine that answers coactivity from the restatement over samples it was given"""

    def __init__(self, P, E, A):
        self.P, self.E, self.A = P, E, A
        self.calls = []

    def coactivity(self, last_n, include=None, used=None, end_iter=None, min_load=1.0, credible_interval=0.95, series=False):
        self.calls.append(dict(last_n=last_n, include=include, used=used, end_iter=end_iter))
        sel = slice(None) if used is None else np.asarray(used) == 1
        r = R.coactivity_reference(self.P[-last_n:][sel], self.E[-last_n:][sel], self.A[-last_n:][sel], include=include, min_load=min_load,
                                   credible_interval=credible_interval)
        return {k: v for k, v in r.items() if series or k != "series"}


def test_get_coactivity_over_a_stub_engine():
    from bayesnmf_amd.sampler import bayesNMF_sampler
    S, K, N, G = 5, 6, 4, 30
    P, E, A = _samples(S, K, N, G, 11)
    sm = bayesNMF_sampler.__new__(bayesNMF_sampler)
    sm._chain = _StubEngine(P, E, A)
    sm.dims = dict(K=K, G=G, N=N)
    sm.log = lambda *a, **k: None
    sm._recorded_range = lambda end_iter, n_samples, idx: (S, None, None, {})
    inc = [1.0] * G
    inc[3], inc[8], inc[20] = None, float("nan"), 0
    out = sm.get_coactivity(include=inc, min_load=2.0, credible_interval=0.8, series=True)
    want = R.coactivity_reference(P, E, A, include=np.array([0 if i in (3, 8, 20) else 1 for i in range(G)]), min_load=2.0, credible_interval=0.8)
    assert out["n_included"] == G - 3 and out["n_left_out"] == 3 and out["pairs"] == want["pairs"] and _same_bits(out["series"], want["series"])
    assert np.array_equal(sm._chain.calls[0]["include"], [0 if i in (3, 8, 20) else 1 for i in range(G)])
    for q, stat in enumerate(R.STATS):
        for row, name in ((0, "mean"), (2, "lower"), (3, "upper"), (4, "p_greater"), (6, "n_valid")):
            mat = out[stat][name]
            assert mat.shape == (N, N) and np.isnan(np.diag(mat)).all() and _same_bits(mat, mat.T)
            for p, (a, b) in enumerate(want["pairs"]):
                assert _same_bits(mat[a, b], want["pair"][q, row, p])
    assert out["n_credible"] == want["n_credible"] and out["max_cosine_at"] == want["max_cosine_at"]
    with pytest.raises(ValueError, match="include has 2 values"):
        sm.get_coactivity(include=[1, 1])
    with pytest.raises(ValueError, match="other than 0, 1"):
        sm.get_coactivity(include=[2.0] * G)
    sm._chain = object()
    with pytest.raises(ValueError, match="get_coactivity needs an engine"):
        sm.get_coactivity()
