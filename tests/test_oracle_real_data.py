"""The oracle on real-valued Normal data (orc_create_f64): its data path, its metric rows against a numpy restatement of
R/utils.R, and the committed golden chain of real data.  The laws of the Normal full conditionals on real data are in
test_oracle_laws.py; the engine's parity with all of this is in test_gpu_real_data.py."""
import math
import os

import numpy as np
import pytest
import scipy.stats as st

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PRIOR_IDS = dict(exponential=["Lambda_p", "Lambda_e"], truncnormal=["Mu_p", "Sigmasq_p", "Mu_e", "Sigmasq_e"])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b, what):
    assert np.array_equal(_bits(a), _bits(b)), what


def _real(K, G, seed, sd=0.5):
    """P E + N(0, sd^2) with magnitudes around 1: fractional everywhere, negative cells, and cells at the edges of the padded KL"""
    rng = np.random.default_rng(seed)
    M = rng.gamma(4.0, 0.06, size=(K, 3)) @ rng.gamma(4.0, 0.3, size=(3, G)) + rng.normal(0.0, sd, size=(K, G))
    M = np.asfortranarray(M)
    M[:7, 0] = [0.0, -0.0, 5e-7, 1e-6, np.nextafter(1.0, 0.0), -0.5, 0.7]
    return M


RANKS = [("fixed", False, "SBFI"), ("SBFI", True, "SBFI"), ("BFI", True, "BFI")]


@pytest.mark.parametrize("fresh", [False, True], ids=["maintained", "fresh_mhat"])
@pytest.mark.parametrize("rank", RANKS, ids=[r[0] for r in RANKS])
@pytest.mark.parametrize("prior", ["truncnormal", "exponential"])
def test_integer_data_same_chain_as_float64_or_int32(oracle_lib, prior, rank, fresh):
    """Whole numbers as float64 (orc_create_f64) and as int32 (orc_create): the same oracle chain, bit for bit, metric rows included."""
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    O = oracle_lib
    _, lr, method = rank
    K, G, N = 12, 40, 4
    M, _, _ = synth_counts(K, G, 2, 99)
    M[0, :] = 0
    temp = np.array([1e-4] * 5 + [1.0] * 10) if lr else None
    names = ["P", "E", "A", "R", "sigmasq", "Alpha", "Beta"] + PRIOR_IDS[prior]
    runs = []
    for data in (M.astype(np.int32), M.astype(np.float64)):
        o = O.Oracle(data, N, likelihood="normal", prior=prior, learning_rank=lr, rank_method=method, seed=5, temperature=temp, nthreads=2)
        assert o.M.dtype == data.dtype
        apply_hyperprior_params(o, prior, M, N)
        o.set_fresh_mhat(fresh)
        rows, states = [o.init()], []
        for n in (1, 4, 7):
            rows += list(o.run(n))
            states.append({nm: o.get(nm).copy() for nm in names})
        runs.append((np.array(rows), states))
        o.close()
    (ri, si), (rf, sf) = runs
    _same(np.nan_to_num(ri), np.nan_to_num(rf), "metric rows")
    for c, (a, b) in enumerate(zip(si, sf)):
        for nm in names:
            _same(a[nm], b[nm], f"{nm} after call {c}")
    if lr:
        assert len(np.unique(ri[:, 7])) >= 2, "the rank never moved: the rank sweep tests nothing"


def test_data_rules_of_either_entry_point(oracle_lib):
    """Normal keeps float64 as float64; Poisson refuses counts that are not whole numbers in [0, 2^31 - 1] (bnmf_create_f64's rule),
    in the constructor and in set_M; non-finite Normal data are refused; set_M swaps the data with the constructor's rules."""
    O = oracle_lib
    M = _real(8, 5, 1)
    o = O.Oracle(M, 2, likelihood="normal", prior="exponential")
    assert o.M.dtype == np.float64 and np.array_equal(_bits(o.M), _bits(M))
    o.set_M(np.ones((8, 5), dtype=np.int32))
    assert o.M.dtype == np.int32
    o.set_M(M)
    assert o.M.dtype == np.float64
    for bad in (np.nan, np.inf):
        X = M.copy(); X[2, 3] = bad
        with pytest.raises(ValueError, match=r"M\[2, 3\]"):
            O.Oracle(X, 2, likelihood="normal", prior="exponential")
        with pytest.raises(ValueError):
            o.set_M(X)
    o.close()
    counts = np.full((6, 5), 3.0)
    p = O.Oracle(counts, 2, prior="gamma")
    assert p.M.dtype == np.int32 and (p.M == 3).all()
    for v in (2.5, -1.0, 2.0 ** 31, np.nan):
        X = counts.copy(); X[1, 4] = v
        with pytest.raises(ValueError, match=r"M\[1, 4\]"):
            O.Oracle(X, 2, prior="gamma")
        with pytest.raises(ValueError):
            p.set_M(X)
    p.close()


def _fsum_close(got, terms, what):
    """got against the exact sum of the terms: rtol 1e-12 of the sum (or of the sum of magnitudes, where the terms cancel)"""
    ref = math.fsum(np.ravel(terms))
    scale = max(abs(ref), math.fsum(np.abs(np.ravel(terms))))
    assert abs(got - ref) <= 1e-12 * scale, f"{what}: {got!r} vs {ref!r}"


@pytest.mark.parametrize("lr", [False, True], ids=["fixed", "SBFI"])
@pytest.mark.parametrize("prior", ["truncnormal", "exponential"])
def test_metric_rows_of_real_data_are_the_reference_metrics(oracle_lib, prior, lr):
    """Every metric row of the oracle on real data, restated in numpy from the oracle's own state at that iteration: RMSE, KL with
    pmax(M, 1e-6) and pmax(Mhat, 1e-6) (padded_KL_, R/utils.R:467-470), the dnorm log-likelihood (R/utils.R:72-97), the log-posterior
    (R/utils.R:132-175), the parameter count and BIC."""
    from bayesnmf_amd.setup import apply_hyperprior_params
    K, G, N = 20, 30, 4
    M = _real(K, G, 3)
    assert (M < 0).sum() > 20 and ((M > 1e-6) & (M < 1)).sum() > 20
    temp = np.concatenate([np.full(3, 1e-3), np.ones(20)]) if lr else None
    o = oracle_lib.Oracle(M, N, likelihood="normal", prior=prior, learning_rank=lr, seed=8, temperature=temp, nthreads=2)
    apply_hyperprior_params(o, prior, M, N)
    rows = [o.init()]
    names = ["P", "E", "A", "sigmasq"] + PRIOR_IDS[prior]
    states = [{nm: o.get(nm) for nm in names}]
    for _ in range(10):
        rows.append(o.run(1)[0])
        states.append({nm: o.get(nm) for nm in names})
    for i, (row, s) in enumerate(zip(rows, states)):
        P, E, A, sg = s["P"], s["E"], s["A"][0], s["sigmasq"]
        Mhat = (P * A[None, :]) @ E
        se = (Mhat - M) ** 2
        mt, mh = np.maximum(M, 1e-6), np.maximum(Mhat, 1e-6)
        kl = mt * (np.log(mt) - np.log(mh))
        ll = st.norm.logpdf(M, Mhat, np.sqrt(sg)[None, :])
        if prior == "exponential":
            lp = [np.log(s["Lambda_p"]) - s["Lambda_p"] * P, np.log(s["Lambda_e"]) - s["Lambda_e"] * E]
        else:
            lp = []
            for X, mu, s2 in ((P, s["Mu_p"], s["Sigmasq_p"]), (E, s["Mu_e"], s["Sigmasq_e"])):
                sd = np.sqrt(s2)
                lp.append(st.norm.logpdf(X, mu, sd) - st.norm.logcdf(mu / sd))      # truncated at 0
        assert row[0] == i + 1
        assert row[1] == pytest.approx(math.sqrt(math.fsum(se.ravel()) / (K * G)), rel=1e-12, abs=0), f"RMSE, row {i}"
        _fsum_close(row[2], kl, f"KL, row {i}")
        _fsum_close(row[3], ll, f"loglikelihood, row {i}")
        _fsum_close(row[4], np.concatenate([ll.ravel()] + [x.ravel() for x in lp]), f"logposterior, row {i}")
        assert row[5] == A.sum() * (G + K) and row[7] == A.sum()
        assert row[6] == pytest.approx(-2.0 * row[3] + row[5] * np.log(G), rel=1e-14)
    o.close()


def test_golden_chain_of_real_data(oracle_lib):
    """The committed real-data chain (tests/golden/make_golden.py normal_golden: Normal-TruncNormal, SBFI with tempering) regenerates
    bit for bit."""
    from bayesnmf_amd.setup import apply_hyperprior_params
    g = np.load(os.path.join(GOLD, "nt_sbfi_real_k12_g10_n3.npz"))
    M, N = g["M"], g["P"].shape[1]
    assert M.dtype == np.float64 and (M < 0).any() and (M != np.floor(M)).any()
    o = oracle_lib.Oracle(M, N, likelihood="normal", prior="truncnormal", learning_rank=True, seed=5, temperature=g["temperature"])
    apply_hyperprior_params(o, "truncnormal", M, N)
    rows = [o.init()] + list(o.run(g["metrics"].shape[0] - 1))
    _same(np.array(rows)[:, :9], g["metrics"][:, :9], "metric rows")
    for nm in ("P", "E", "A", "R", "sigmasq") + tuple(PRIOR_IDS["truncnormal"]):
        _same(o.get(nm), g[nm], nm)
    # the chain learned, not just ran: A moved under the tempering
    assert len(np.unique(g["metrics"][:, 7])) >= 2
    o.close()
