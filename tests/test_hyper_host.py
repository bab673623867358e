"""The oracle's side of tests/test_gpu_hyper.py: with per-element hyper-prior matrices (HY(id, e) read with stride 1) its hyper sweep still
draws from the laws of R/sample_priors.R — method and thresholds of tests/test_oracle_laws.py —, a matrix of equal entries is the scalar,
and a hyper array of any other length is refused."""
import numpy as np
import pytest
import scipy.special as sp
import scipy.stats as st

from test_gpu_hyper import matrices, HYPER


def _apply(o, prior, M, N, user):
    from bayesnmf_amd.setup import apply_hyperprior_params
    return apply_hyperprior_params(o, prior, M, N, user)


def _data(K=7, G=9, seed=5):
    rng = np.random.default_rng(seed)
    return rng.poisson(rng.gamma(2.0, 8.0, size=(K, G))).astype(np.int32)


def test_gamma_hyper_sweep_law_with_matrices(oracle_lib):
    """sample_Beta_* (R/sample_priors.R:323-345): Beta[e] ~ Gamma(A[e] + Alpha[e], B[e] + v[e]), by probability-integral transform pooled
    over elements; sample_Alpha_* (:356-397): Alpha[e] from f(x) ~ x^(C[e] - 1) exp(-tau[e] x) / Gamma(x) on [1e-3, 1e4] with
    tau[e] = D[e] - log Beta[e] - log v[e], by the transform through the numerical CDF of each element's own target."""
    M, N = _data(), 3
    o = oracle_lib.Oracle(M, N, prior="gamma", seed=6, save_Z=True)
    U = matrices("gamma", M, N, 3)
    _apply(o, "gamma", M, N, U)
    o.init(); o.run(5)
    xs = np.exp(np.linspace(np.log(1e-3), np.log(1e4), 40001))
    lx, lgx, dx = np.log(xs), sp.gammaln(xs), np.diff(xs)

    def pit_alpha(x, c, tau):
        out = np.empty(x.size)
        for i, (xi, ci, ti) in enumerate(zip(x.ravel(), c.ravel(), tau.ravel())):
            h = (ci - 1.0) * lx - ti * xs - lgx
            f = np.exp(h - h.max())
            cdf = np.concatenate([[0.0], np.cumsum(0.5 * (f[1:] + f[:-1]) * dx)])
            out[i] = np.interp(xi, xs, cdf) / cdf[-1]
        return out
    uB, uA = [], []
    for rep in range(60):
        t = 50 + rep
        P0, E0, Alp0, Ale0 = o.get("P"), o.get("E"), o.get("Alpha_p"), o.get("Alpha_e")
        o.step("hyper", t)
        for side, X, Al0 in (("p", P0, Alp0), ("e", E0, Ale0)):
            Be, Al = o.get("Beta_" + side), o.get("Alpha_" + side)
            uB.append(st.gamma.cdf(Be, U["A_" + side] + Al0, scale=1.0 / (U["B_" + side] + X)).ravel())
            uA.append(pit_alpha(Al, U["C_" + side], U["D_" + side] - np.log(Be) - np.log(X)))
        for what in ("P", "E", "Z"):
            o.step(what, t)
    assert st.kstest(np.concatenate(uB), "uniform").pvalue > 1e-3
    assert st.kstest(np.concatenate(uA), "uniform").pvalue > 1e-3


def test_exponential_hyper_sweep_law_with_matrices(oracle_lib):
    """sample_Lambda_* (R/sample_priors.R:284-308): Lambda[e] ~ Gamma(A[e] + 1, B[e] + v[e])."""
    M, N = _data(), 3
    o = oracle_lib.Oracle(M, N, prior="exponential", seed=6, save_Z=True)
    U = matrices("exponential", M, N, 4)
    _apply(o, "exponential", M, N, U)
    o.init(); o.run(5)
    us = []
    for rep in range(300):
        t = 50 + rep
        P0, E0 = o.get("P"), o.get("E")
        o.step("hyper", t)
        us.append(st.gamma.cdf(o.get("Lambda_p"), U["A_p"] + 1.0, scale=1.0 / (U["B_p"] + P0)).ravel())
        us.append(st.gamma.cdf(o.get("Lambda_e"), U["A_e"] + 1.0, scale=1.0 / (U["B_e"] + E0)).ravel())
        for what in ("P", "E", "Z"):
            o.step(what, t)
    assert st.kstest(np.concatenate(us), "uniform").pvalue > 1e-3


def test_truncnormal_hyper_sweep_law_with_matrices(oracle_lib):
    """sample_Mu_* / sample_Sigmasq_* exactly as the reference writes them (sd = 1 / denom; the E side adds A_e where B_e is meant:
    tests/test_oracle_laws.py test_truncnormal_hyper_sweep_quirks_law), from per-element M, S, A, B."""
    rng = np.random.default_rng(9)
    K, G, N = 6, 5, 2
    M = rng.poisson(30.0, size=(K, G)).astype(np.int32)
    o = oracle_lib.Oracle(M, N, prior="truncnormal", MH=True, seed=3)
    U = matrices("truncnormal", M, N, 5)
    _apply(o, "truncnormal", M, N, U)
    o.init()
    P, E = o.get("P"), o.get("E")
    Sp0, Se0 = np.full((K, N), 1.7), np.full((N, G), 0.6)
    zs, us = [], []
    for rep in range(400):
        o.set("Sigmasq_p", Sp0); o.set("Sigmasq_e", Se0)
        o.step("hyper", 10 + rep)
        for side, X, S0, rate0 in (("p", P, Sp0, U["B_p"]), ("e", E, Se0, U["A_e"])):   # A_e quirk
            m, s, a = U["M_" + side], U["S_" + side], U["A_" + side]
            mu = o.get("Mu_" + side)
            den = 1.0 / s + 1.0 / S0
            num = m / s + X / S0
            zs.append(((mu - num / den) * den).ravel())
            us.append(st.gamma.cdf((rate0 + (X - mu) ** 2 / 2.0) / o.get("Sigmasq_" + side), a + 0.5).ravel())
    assert st.kstest(np.concatenate(zs), "norm").pvalue > 1e-3
    assert st.kstest(np.concatenate(us), "uniform").pvalue > 1e-3


@pytest.mark.parametrize("prior,kw", [("gamma", {}), ("exponential", {}), ("truncnormal", dict(MH=True)), ("exponential", dict(likelihood="normal"))])
def test_matrix_of_equal_entries_is_the_scalar(oracle_lib, prior, kw):
    from bayesnmf_amd.setup import default_hyperprior_params
    M, N = _data(12, 10, 2), 3
    K, G = M.shape
    hp = default_hyperprior_params(prior, M, N)
    full = {k[0].upper() + k[1:]: np.full((K, N) if k.endswith("_p") else (N, G), v) for k, v in hp.items()}
    assert set(full) == {f"{nm.upper()}_{s}" for nm in HYPER[prior] for s in "pe"}
    chains = []
    for user in (None, full):
        o = oracle_lib.Oracle(M, N, prior=prior, seed=4, **kw)
        _apply(o, prior, M, N, user)
        r0 = o.init()
        rows = np.vstack([r0[None, :], o.run(6)])
        chains.append((rows, o.get("P"), o.get("E")))
    for a, b in zip(*chains):
        assert np.array_equal(np.nan_to_num(a).view(np.uint64), np.nan_to_num(b).view(np.uint64))


def test_hyper_array_of_another_length_is_refused(oracle_lib):
    M, N = _data(), 3
    K, G = M.shape
    o = oracle_lib.Oracle(M, N, prior="gamma", seed=4)
    for name, full in (("A_p", K * N), ("C_e", N * G), ("D_e", N * G)):
        for n in (2, N, full - 1, full + 1):
            with pytest.raises(ValueError):
                o.set(name, np.ones(n))
        o.set(name, np.ones(full)); o.set(name, [2.0])
