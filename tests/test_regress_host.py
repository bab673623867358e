"""Regression of exposures on tumour covariates over a recorded range, the parts that need no GPU: the numpy restatement of the spec
(tests/regress_ref.py) against its laws on synthetic rings, numpy.linalg.lstsq as the yardstick of the coefficients,
bayesNMF_sampler.get_regression over a stub engine, and the two new symbols."""
import os
import re
import subprocess

import numpy as np
import pytest

import contrast_ref as CR
import regress_ref as R

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
    """non-negative P, E and 0 / 1 A: the samples in `exclude` include no factor at all"""
    rng = np.random.default_rng(seed)
    P = rng.gamma(0.5, 1.0, size=(S, K, N))
    E = rng.gamma(0.7, 30.0, size=(S, N, G))
    A = (rng.uniform(size=(S, N)) < 0.8).astype(np.float64)
    A[:, 0] = 1.0
    for s in exclude:
        A[s] = 0.0
    return P, E, A


def _unit_P(S, K, N):
    """P whose column sums are exactly 1 (one 1.0 per column): the renormalised exposure x is E itself, bit for bit"""
    P = np.zeros((S, K, N))
    P[:, 0, :] = 1.0
    return P


def _design(G, seed, binary=True):
    """intercept, an age-like covariate (mean 60, sd 12) and a 0 / 1 covariate"""
    rng = np.random.default_rng(seed)
    cols = [np.ones(G), np.round(60.0 + 12.0 * rng.standard_normal(G))]
    if binary:
        cols.append((rng.uniform(size=G) < 0.4).astype(np.float64))
    return np.stack(cols, axis=1)


def _chain_len(m):
    """the most roundings a term of canonB over m members passes through: its product, at most 1,024 / 64 additions in its accumulator,
    the 6 levels of the tree and one addition per block"""
    return 1 + R.BLOCK // 64 + 6 + (m + R.BLOCK - 1) // R.BLOCK


def _normal_equations_bound(D, y, beta_norm):
    """||beta^ - beta||_2 for the restatement's route (Gram matrix, Cholesky, two triangular solves), beta the exact least-squares solution.
    With k = _chain_len(m): the computed Gram matrix is D'D + dG1, |dG1| <= gamma(k) |D'||D|, so ||dG1||_2 <= gamma(k) ||D||_F^2; the computed
    right-hand side is D'y + dw, ||dw||_2 <= gamma(k) ||D||_F ||y||_2; Cholesky and the two solves give (G^ + dG2) beta^ = w^ with |dG2| <=
    gamma(3 Q + 1) |L||L'| (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 10.4) and || |L||L'| ||_2 <= Q ||G^||_2.  So
    (G + dG) beta^ = w + dw with ||dG||_2 <= e_G = gamma(k) ||D||_F^2 + gamma(3 Q + 1) Q (1 + gamma(k)) ||D||_F^2, and with ||G^-1||_2 = 1 /
    sigma_min(D)^2 and d = ||G^-1||_2 e_G < 1:  ||beta^ - beta||_2 <= ||G^-1||_2 (||dw||_2 + e_G ||beta||_2) / (1 - d)."""
    m, Q = D.shape
    k = _chain_len(m)
    fro, smin = np.linalg.norm(D), np.linalg.svd(D, compute_uv=False)[-1]
    e_G = _gamma(k) * fro ** 2 + _gamma(3 * Q + 1) * Q * (1.0 + _gamma(k)) * fro ** 2
    d = e_G / smin ** 2
    assert d < 0.5, "the design is too ill-conditioned for the bound to say anything"
    return (_gamma(k) * fro * np.linalg.norm(y) + e_G * beta_norm) / smin ** 2 / (1.0 - d)


def _lstsq_bound(D, y, beta_norm, resid_norm):
    """the yardstick's own error: LAPACK's least-squares drivers are backward stable: the computed solution is exact for D + dD, y + dy with
    ||dD||_F <= eta ||D||_F, ||dy||_2 <= eta ||y||_2, eta = c m Q U / (1 - c m Q U) with c a small integer (Higham Thm 20.3 for Householder QR;
    taken as 8 here, the SVD route of gelsd is of the same kind).  To first order (Higham Thm 20.1, Wedin) the solution moves by
    D^+ (dy - dD beta) + (D'D)^-1 dD' r:  <= eta (||y||_2 + ||D||_F ||beta||_2) / sigma_min + eta ||D||_F ||r||_2 / sigma_min^2; twice that covers
    the higher-order terms while eta kappa < 1/2."""
    m, Q = D.shape
    eta = 8 * m * Q * U / (1.0 - 8 * m * Q * U)
    fro, sv = np.linalg.norm(D), np.linalg.svd(D, compute_uv=False)
    assert eta * sv[0] / sv[-1] < 0.5
    return 2.0 * (eta * (np.linalg.norm(y) + fro * beta_norm) / sv[-1] + eta * fro * resid_norm / sv[-1] ** 2)


def test_coefficients_agree_with_lstsq():
    """every (sample, response, factor) of two designs — three columns at m = 300 and the age column squared and cubed beside it at m = 2,100
    (three blocks), condition numbers of a few hundred, printed — against numpy.linalg.lstsq on the same y, inside the sum of the two bounds above"""
    worst = 0.0
    for G, seed, extra in ((300, 1, False), (2100, 2, True)):
        S, K, N = 4, 6, 3
        P, E, A = _samples(S, K, N, G, seed)
        D = _design(G, seed)
        if extra:
            age = (D[:, 1] - 60.0) / 12.0
            D = np.concatenate([D, (age ** 2)[:, None], (age ** 3)[:, None]], axis=1)
        ref = R.regress_reference(P, E, A, D)
        Y = ref["Y"].reshape(G, -1)
        B = ref["coef_series"]                                                       # [3][S][N][Q]
        want, _, rank, sv = np.linalg.lstsq(D, Y, rcond=None)
        assert rank == D.shape[1]
        print(f"regress host: m {G} Q {D.shape[1]} condition number {sv[0] / sv[-1]:.3g} min_pivot_ratio {ref['min_pivot_ratio']:.3g}")
        for c in range(Y.shape[1]):
            q, s, n = np.unravel_index(c, (3, S, N))
            y, b = Y[:, c], want[:, c]
            bound = _normal_equations_bound(D, y, np.linalg.norm(b)) + _lstsq_bound(D, y, np.linalg.norm(b), np.linalg.norm(y - D @ b))
            err = np.linalg.norm(B[q, s, n] - b)
            assert err <= bound, (G, q, s, n, err, bound)
            worst = max(worst, err / bound if bound > 0 else 0.0)
    print(f"regress host: largest error / bound against lstsq {worst:.3g}")


def test_an_exactly_linear_response_is_recovered():
    """x = 7 + 3 age - 40 flag in whole numbers with unit column sums of P: every product and sum of the Gram matrix and of the moments is a
    whole number below 2^53, so w and the Gram matrix are exact and beta^ differs from the truth by the Cholesky route alone, inside
    _normal_equations_bound (which also allows for rounding in the sums).  The residuals are then e_i = D_i (beta - beta^) up to the gamma(Q + 1)
    |D_i||beta^| of forming yhat, so 1 - r2 = rss / tss <= (1 + gamma(k)) sum_i (||D_i||_2 bound + gamma(Q + 1) |D_i||beta^|)^2 / (tss (1 - gamma(k + 3))), the
    denominator for the rounding of the restatement's own tss."""
    S, K, N, G = 3, 4, 2, 130
    D = _design(G, 3)
    truth = np.array([[7.0, 3.0, -40.0], [500.0, -2.0, 11.0]])                       # [N][Q]; x stays positive for ages 20 .. 100
    x = (D @ truth.T).T                                                              # [N][G], whole numbers
    assert (x > 0).all() and (x == np.round(x)).all()
    E = np.repeat(x[None], S, axis=0)
    ref = R.regress_reference(_unit_P(S, K, N), E, np.ones((S, N)), D)
    assert np.array_equal(ref["Y"][:, 0, 0, :], x.T)
    for n in range(N):
        bound = _normal_equations_bound(D, x[n], np.linalg.norm(truth[n]))
        for s in range(S):
            b = ref["coef_series"][0, s, n]
            assert np.linalg.norm(b - truth[n]) <= bound
            tss = float(((x[n] - x[n].mean()) ** 2).sum())
            e = np.linalg.norm(D, axis=1) * bound + _gamma(D.shape[1] + 1) * (np.abs(D) @ np.abs(b))
            lim = (1.0 + _gamma(_chain_len(G))) * float((e ** 2).sum()) / (tss * (1.0 - _gamma(_chain_len(G) + 3)))
            r2 = ref["r2_series"][0, s, n]
            assert 0.0 <= 1.0 - r2 <= lim + U, (1.0 - r2, lim)                       # (+ U: the rounding of 1 - rss / tss itself)
    assert (ref["fit"][0, 3] == S).all()


def test_a_group_indicator_gives_the_difference_of_the_group_means():
    """design [1, 1{group a}]: beta_1 is mean_a(y) - mean_b(y) and beta_0 is mean_b(y).  contrast_ref forms the two means by canonical sums of
    non-negative terms (relative error gamma(ceil(m_c / 64) + 7) each, the division included); the regression's route is inside
    _normal_equations_bound."""
    S, K, N, G = 5, 6, 3, 150
    P, E, A = _samples(S, K, N, G, 4, exclude=(2,))
    groups = (np.random.default_rng(9).uniform(size=G) < 0.35).astype(np.int32)      # 1 = group a
    D = np.stack([np.ones(G), groups.astype(np.float64)], axis=1)
    ref = R.regress_reference(P, E, A, D)
    con = CR.contrast_reference(P, E, A, 1 - groups)                                 # contrast's group 0 = a, group 1 = b
    for q in range(2):                                                               # load and share are contrast's v0 and v1
        va, vb = con["series"][q, :, :, 0], con["series"][q, :, :, 1]
        for s in range(S):
            for n in range(N):
                y = ref["Y"][:, q, s, n]
                b = ref["coef_series"][q, s, n]
                g = max(_gamma(int(np.ceil(c / 64)) + 7) for c in con["sizes"])
                bound = _normal_equations_bound(D, y, np.hypot(va[s, n] - vb[s, n], vb[s, n])) + g * (2 * vb[s, n] + va[s, n])
                assert abs(b[1] - (va[s, n] - vb[s, n])) <= bound and abs(b[0] - vb[s, n]) <= bound, (q, s, n)
    # the sample without any factor: y = +0.0 everywhere, beta = 0, rss = tss = 0 and no r2
    assert (ref["coef_series"][:, 2] == 0).all() and np.isnan(ref["r2_series"][:, 2]).all() and (ref["sigma2_series"][:, 2] == 0).all()
    assert (ref["fit"][:, 3] <= S - 1).all() and ref["fit"][0, 3, 0] == S - 1


def test_scaling_a_column_by_a_power_of_two_divides_its_coefficient_exactly():
    S, K, N, G = 4, 6, 3, 1100
    P, E, A = _samples(S, K, N, G, 5)
    D = _design(G, 5)
    a = R.regress_reference(P, E, A, D, credible_interval=0.9)
    D2 = D.copy()
    D2[:, 1] *= 2.0 ** 7
    D2[:, 2] *= 2.0 ** -3
    b = R.regress_reference(P, E, A, D2, credible_interval=0.9)
    scale = np.array([1.0, 2.0 ** -7, 2.0 ** 3])
    assert _same_bits(b["coef_series"], a["coef_series"] * scale)
    assert _same_bits(b["coef"][:, [0, 2, 3]], a["coef"][:, [0, 2, 3]] * scale) and _same_bits(b["coef"][:, 1], a["coef"][:, 1] * scale ** 2)
    assert _same_bits(b["coef"][:, 4:], a["coef"][:, 4:])
    for k in ("fit", "r2_series", "sigma2_series"):
        assert _same_bits(b[k], a[k]), k
    assert np.array_equal(b["n_credible"], a["n_credible"]) and b["min_pivot_ratio"] == a["min_pivot_ratio"] and b["min_pivot_at"] == a["min_pivot_at"]


def test_leaving_tumours_out_is_removing_them():
    S, K, N, G = 4, 6, 3, 1200
    P, E, A = _samples(S, K, N, G, 6)
    D = _design(G, 6)
    inc = np.ones(G, dtype=np.int32)
    inc[np.random.default_rng(1).choice(G, 150, replace=False)] = 0
    D_nan = D.copy()
    D_nan[inc == 0] = np.nan                                                         # the cells of left-out rows are not read
    a = R.regress_reference(P, E, A, D_nan, include=inc)
    keep = inc == 1
    b = R.regress_reference(P, E[:, :, keep], A, D[keep])
    assert a["n_included"] == 1050 and a["n_left_out"] == 150 and a["n_blocks"] == 2 and b["n_left_out"] == 0
    for k in ("coef", "fit", "coef_series", "r2_series", "sigma2_series"):
        assert _same_bits(a[k], b[k]), k
    assert np.array_equal(a["n_credible"], b["n_credible"]) and a["min_pivot_ratio"] == b["min_pivot_ratio"]
    # the shares, though, are shares of the tumour's own total: leaving tumours out does not change the others'
    assert not _same_bits(a["coef"], R.regress_reference(P, E, A, D)["coef"])


def test_a_planted_slope_is_found_and_an_unrelated_covariate_is_not():
    """Signature 0 grows by 2 mutations per year of age, signature 1 does not; a second covariate is drawn independently of everything.
    Every sample jitters the truth by 5 %."""
    rng = np.random.default_rng(8)
    S, K, N, G = 40, 5, 2, 400
    age = np.round(60.0 + 12.0 * rng.standard_normal(G))
    other = rng.standard_normal(G)
    truth = np.stack([20.0 + 2.0 * age, np.full(G, 80.0)])
    E = truth[None] * (1.0 + 0.05 * rng.standard_normal((S, N, G)))
    D = np.stack([np.ones(G), age, other], axis=1)
    ref = R.regress_reference(_unit_P(S, K, N), E, np.ones((S, N)), D, credible_interval=0.95)
    load = ref["coef"][0]                                                            # [6][N][Q]
    assert load[2, 0, 1] > 0 and load[4, 0, 1] == 1.0 and load[5, 0, 1] == 0.0 and abs(load[0, 0, 1] - 2.0) < 0.1
    assert load[2, 0, 2] < 0 < load[3, 0, 2] and load[2, 1, 1] < 0 < load[3, 1, 1] and load[2, 1, 2] < 0 < load[3, 1, 2]
    assert ref["n_credible"][0].tolist() == [2, 1, 0]                                 # the intercepts, the slope, nothing for the unrelated one
    assert ref["fit"][0, 0, 0] > 0.8 and ref["fit"][0, 0, 1] < 0.1 and (ref["fit"][0, 3] == S).all()
    none = R.regress_reference(_unit_P(S, K, N), E, np.ones((S, N)), D, credible_interval=0.0)
    assert np.isnan(none["coef"][:, 2:4]).all() and np.isnan(none["fit"][:, 1:3]).all() and (none["n_credible"] == 0).all()
    assert _same_bits(none["coef"][:, [0, 1, 4, 5]], ref["coef"][:, [0, 1, 4, 5]]) and _same_bits(none["fit"][:, [0, 3, 4]], ref["fit"][:, [0, 3, 4]])


def test_the_restatement_refuses_what_the_call_refuses():
    """The duplicated column is the column of ones over m = 64 tumours, where the arithmetic of the factor is exact: L[0][0] = 8, L[j][0] =
    Gm[j][0] / 8 without rounding, so the second column of ones has L[3][0] = 8, L[3][1] = L[3][2] = 0 / L[j][j] = 0 and the pivot d_3 = 64 - 64 is
    0: refused.  (The spec invents no threshold: a dependent column whose pivot rounds to a positive number is not refused, it shows as a
    min_pivot_ratio of the order of the unit roundoff.)"""
    S, K, N, G = 3, 4, 2, 64
    P, E, A = _samples(S, K, N, G, 7)
    D = _design(G, 7)
    dup = np.concatenate([D, D[:, 0:1]], axis=1)
    with pytest.raises(R.Refused, match=r"full column rank \(column 3\)") as e:
        R.regress_reference(P, E, A, dup)
    assert e.value.code == -1
    inc = np.zeros(G, dtype=np.int32)
    inc[:3] = 1
    for include, code in ((inc, -2), (np.where(np.arange(G) < 4, 1, 0), None)):      # m = Q is refused, m = Q + 1 is the smallest fit
        if code:
            with pytest.raises(R.Refused, match="3 included tumours for Q = 3") as e:
                R.regress_reference(P, E, A, D, include=include)
            assert e.value.code == code
        else:
            ok = R.regress_reference(P, E, A, D, include=include)
            assert ok["n_included"] == 4 and np.isfinite(ok["coef_series"]).all()
    bad = D.copy()
    bad[5, 2] = np.inf
    with pytest.raises(R.Refused, match=r"design\[5, 2\]"):
        R.regress_reference(P, E, A, bad)
    bad[5, 2] = 0.0
    inc = np.ones(G, dtype=np.int32)
    inc[9] = 2
    with pytest.raises(R.Refused, match="include"):
        R.regress_reference(P, E, A, bad, include=inc)
    with pytest.raises(R.Refused, match="Q = 17"):
        R.regress_reference(P, E, A, np.ones((G, 17)))
    for ci in (1.0, float("nan")):
        with pytest.raises(R.Refused, match="credible_interval"):
            R.regress_reference(P, E, A, D, credible_interval=ci)
    with pytest.raises(R.Refused, match="1 used samples"):
        R.regress_reference(P[:1], E[:1], A[:1], D)


def test_regression_design():
    from bayesnmf_amd.sampler import regression_design
    nan = float("nan")
    X, inc, names = regression_design({"age": [50, 60, None, 70, 80], "dose": [1.0, nan, 2.0, 0.0, 4.0]}, 5)
    assert names == ["(Intercept)", "age", "dose"] and X.shape == (5, 3) and X.flags.f_contiguous and (X[:, 0] == 1).all()
    assert inc.tolist() == [1, 0, 0, 1, 1] and inc.dtype == np.int32 and X[0].tolist() == [1.0, 50.0, 1.0] and np.isnan(X[2, 1])
    X, inc, names = regression_design(np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 7.0]]), 3, intercept=False)
    assert names == ["x1", "x2"] and inc is None and X.tolist() == [[1.0, 2.0], [3.0, 4.0], [5.0, 7.0]]
    X, inc, names = regression_design([1.0, 2.0, 3.0], 3)                            # one covariate as a vector
    assert names == ["(Intercept)", "x1"] and X[:, 1].tolist() == [1.0, 2.0, 3.0]
    X, inc, names = regression_design({"age": [50.0, 60.0, nan, 70.0]}, 4, standardize=True)
    v = np.array([50.0, 60.0, 70.0])
    assert inc.tolist() == [1, 1, 0, 1] and np.array_equal(X[[0, 1, 3], 1], (v - v.mean()) / v.std(ddof=1)) and (X[:, 0] == 1).all()
    import pandas as pd
    X, inc, names = regression_design(pd.DataFrame({"a": [1.0, None, 3.0], "b": [0, 1, 1]}), 3)
    assert names == ["(Intercept)", "a", "b"] and inc.tolist() == [1, 0, 1] and X[2].tolist() == [1.0, 3.0, 1.0]
    with pytest.raises(ValueError, match="covariate age has 2 values for 3 tumours"):
        regression_design({"age": [1, 2]}, 3)
    with pytest.raises(ValueError, match="covariate b is constant"):
        regression_design({"a": [1.0, 2.0, 3.0], "b": [4.0, 4.0, 4.0]}, 3, standardize=True)


def test_get_regression_ranges_idx_and_result(tmp_path):
    """bayesNMF_sampler.get_regression over a stub engine: the design, the range and idx rules of get_WAIC, the shape of the result, the log line"""
    from test_waic_host import _NoWaicEngine
    from bayesnmf_amd.sampler import bayesNMF_sampler
    from bayesnmf_amd.convergence import new_convergence_control
    from bayesnmf_amd.setup import synth_counts

    class _RegEngine(_NoWaicEngine):
        calls = []

        def regress(self, last_n, design, include=None, used=None, end_iter=None, credible_interval=0.95, series=False):
            type(self).calls.append(dict(last_n=last_n, design=np.array(design), include=None if include is None else np.array(include),
                                         used=None if used is None else np.array(used), end_iter=end_iter, ci=credible_interval, series=series))
            S = last_n if used is None else int(np.sum(used))
            N, Q = self.N, design.shape[1]
            m = design.shape[0] if include is None else int(np.sum(include))
            out = dict(n_used=S, Q=Q, n_included=m, n_left_out=design.shape[0] - m, n_blocks=1, min_pivot_at=Q - 1, min_pivot_ratio=0.25,
                       n_credible=np.arange(3 * Q).reshape(3, Q), credible_interval=credible_interval,
                       coef=np.arange(3 * 6 * N * Q, dtype=float).reshape(3, 6, N, Q), fit=np.arange(3 * 5 * N, dtype=float).reshape(3, 5, N))
            if series:
                out.update(coef_series=np.zeros((3, S, N, Q)), r2_series=np.zeros((3, S, N)))
            return out

    M, _, _ = synth_counts(12, 9, 2, 3, mean_total=200)
    cc = new_convergence_control()
    cc.update(MAP_over=4, MAP_every=2, maxiters=10, miniters=2)
    s = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "r"), engine_factory=_RegEngine,
                         convergence_control=cc, save_all_samples=True, periodic_save=False)
    s.run_gibbs_sampler()
    cov = {"age": [50, 61, None, 47, 70, 66, float("nan"), 58, 49], "smoker": [0, 1, 1, 0, 0, 1, 0, 1, 1]}
    msgs, log = [], s.log
    s.log = lambda m, **kw: (msgs.append(m), log(m, **kw))[1]
    r = s.get_regression(cov)
    c = _RegEngine.calls[-1]
    assert c["last_n"] == 4 and c["end_iter"] is None and c["ci"] == 0.95 and not c["series"] and np.array_equal(c["used"], [1, 1, 1, 1])
    assert c["design"].shape == (9, 3) and (c["design"][:, 0] == 1).all() and c["design"][1].tolist() == [1.0, 61.0, 1.0]
    assert c["include"].tolist() == [1, 1, 0, 1, 1, 1, 0, 1, 1]
    assert r["names"] == ["(Intercept)", "age", "smoker"] and r["n_included"] == 7 and r["n_left_out"] == 2 and r["Q"] == 3 and r["n_used"] == 4
    assert "coef_series" not in r and r["min_pivot_ratio"] == 0.25 and r["n_credible"].shape == (3, 3)
    cf, ft = np.arange(3 * 6 * 3 * 3, dtype=float).reshape(3, 6, 3, 3), np.arange(3 * 5 * 3, dtype=float).reshape(3, 5, 3)
    for q, stat in enumerate(("load", "share", "sqrt_load")):
        for i, row in enumerate(("mean", "var", "lower", "upper", "p_greater", "p_less")):
            assert np.array_equal(r[stat][row], cf[q, i]), (stat, row)
        for i, row in enumerate(("r2_mean", "r2_lower", "r2_upper", "r2_samples", "sigma2_mean")):
            assert np.array_equal(r[stat][row], ft[q, i]), (stat, row)
    assert msgs == ["Regression: 7 tumours included, 2 left out; Q = 3, min_pivot_ratio 0.25 (column smoker); n_credible for the load "
                    "(Intercept) 0, age 1, smoker 2"]
    X = np.arange(18, dtype=float).reshape(9, 2) ** 2
    r = s.get_regression(X, end_iter=8, n_samples=5, idx=[4, 6, 8], intercept=False, standardize=True, credible_interval=0.5, series=True)
    c = _RegEngine.calls[-1]
    assert c["end_iter"] == 8 and c["last_n"] == 5 and np.array_equal(c["used"], [1, 0, 1, 0, 1]) and c["ci"] == 0.5 and c["series"] and c["include"] is None
    assert r["names"] == ["x1", "x2"] and r["coef_series"].shape == (3, 3, 3, 2) and r["r2_series"].shape == (3, 3, 3) and r["include"] is None
    assert np.allclose(c["design"].mean(axis=0), 0.0, atol=1e-12) and np.allclose(c["design"].std(axis=0, ddof=1), 1.0, rtol=1e-12)
    r = s.get_regression(X, end_iter=8, n_samples=5, idx=None)
    assert _RegEngine.calls[-1]["used"] is None and r["names"] == ["(Intercept)", "x1", "x2"]
    with pytest.raises(ValueError, match="covariate x1 has 3 values for 9 tumours"):
        s.get_regression(np.ones((3, 1)))
    with pytest.raises(ValueError, match="not all recorded"):
        s.get_regression(cov, end_iter=12, n_samples=3)
    with pytest.raises(ValueError, match="idx must lie in"):
        s.get_regression(cov, end_iter=8, n_samples=3, idx=[2])
    s.close()
    t = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "one"), engine_factory=_NoWaicEngine)
    with pytest.raises(ValueError, match="get_regression needs an engine"):
        t.get_regression(cov)
    t.close()


def test_new_symbols_declared_exported_and_bound():
    import ctypes as C
    from bayesnmf_amd import engine
    hdr = open(os.path.join(ROOT, "include", "bnmf.h")).read()
    assert re.search(r"typedef struct \{ int32_t n_used, Q, n_included, n_left_out, n_blocks, min_pivot_at;\s*"
                     r"int64_t n_credible\[BNMF_REG_NSTAT\]\[BNMF_REG_MAX_Q\];\s*double credible_interval, min_pivot_ratio; \} bnmf_regress_info;", hdr)
    for name, v in (("MAX_Q", 16), ("BLOCK", 1024), ("NSTAT", 3), ("NCROW", 6), ("NFIT", 5)):
        assert re.search(r"#define BNMF_REG_%s\s+%d\b" % (name, v), hdr), name
    assert re.search(r"#define BNMF_VERSION 100\b", hdr)
    for sym in ("bnmf_regress", "bnmf_regress_at"):
        assert re.search(r"\bint\s+%s\s*\(\s*bnmf_handle\s*\*" % sym, hdr), f"{sym} not declared in include/bnmf.h"
        assert sym in engine.ABI_SYMBOLS
    so = os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    L = engine.lib()
    for sym, nargs in (("bnmf_regress", 12), ("bnmf_regress_at", 13)):
        assert re.search(r"\bT %s$" % sym, exported, re.M), f"{sym} not exported by libbnmf.so"
        assert len(getattr(L, sym).argtypes) == nargs
    assert C.sizeof(engine.BnmfRegressInfo) == 24 + 8 * 3 * 16 + 16 and engine.REG_MAX_Q == R.MAX_Q == 16 and R.BLOCK == 1024
    assert hasattr(engine.Engine, "regress")
