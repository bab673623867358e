"""The restatement of the stream spec's Poisson sampler and of bnmf_ppc (tests/ppc_ref.py, written from DESIGN.md 4 and 14) against
the Poisson law and on planted misfits, on the CPU.  The device is compared with this restatement bit for bit (tests/test_gpu_ppc.py),
so these tests are what stands between "the two agree" and "they are right".  All seeds fixed (deterministic).

Bounds.  Goodness of fit: Pearson chi-square with cells merged to an expected count of 5 and p > 1e-4, the manner and level of
tests/test_oracle_laws.py.  Mean and variance: within 4.5 standard errors, se(mean) = sqrt(lam / n) and se(var) = sqrt((mu4 - lam^2
(n - 3) / (n - 1)) / n) with the Poisson's mu4 = lam + 3 lam^2 (18 such comparisons: 4.5 sigma leaves 1e-4 for all of them).
Attempts of the rejection branch: the hat of PTRS has the area alpha = 1.1239 + 1.1328 / (b - 3.4), b = 0.931 + 2.53 sqrt(lam), over a
density of area 1, so an attempt is accepted with probability 1 / alpha and the attempts of a draw are geometric with mean alpha (1.33 at
lam = 10, 1.124 in the limit).  The mean over 60,000 draws must lie within 2 % of alpha (the constants of the hat are given to four
digits and fitted to the continuous density, the draw is its floor) plus 4.5 standard errors sqrt(alpha (alpha - 1) / n)."""
import math

import numpy as np
import pytest
import scipy.stats as st

import ppc_ref as R

N_DRAWS = 20000
SEEDS = (1, 2, 3)


def _chi2_p(obs, exp):
    """tests/test_oracle_laws.py's: Pearson chi-square p-value with small expected cells merged (expected >= 5 each)"""
    obs, exp = np.asarray(obs, float), np.asarray(exp, float)
    order = np.argsort(exp)
    obs, exp = obs[order], exp[order]
    o2, e2, ao, ae = [], [], 0.0, 0.0
    for o_, e_ in zip(obs, exp):
        ao += o_; ae += e_
        if ae >= 5:
            o2.append(ao); e2.append(ae); ao = ae = 0.0
    if ae > 0:
        if e2:
            o2[-1] += ao; e2[-1] += ae
        else:
            o2.append(ao); e2.append(ae)
    o2, e2 = np.array(o2), np.array(e2)
    if len(o2) < 2:
        return 1.0
    x2 = ((o2 - e2) ** 2 / e2).sum()
    return float(st.chi2.sf(x2, len(o2) - 1))


_DRAWS = {}


def _draws(lam, seed):
    if (lam, seed) not in _DRAWS:
        _DRAWS[(lam, seed)] = R.rpois_vec(np.full(N_DRAWS, lam), seed=seed, chain=0, elem0=0, it=1)
    return _DRAWS[(lam, seed)]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("lam", [0.3, 4.0, 9.9, 10.0, 37.0, 1000.0])
def test_goodness_of_fit(oracle_lib, lam, seed):
    x, att = _draws(lam, seed)
    assert (x >= 0).all() and (x == np.floor(x)).all()
    hi = int(max(x.max(), st.poisson.ppf(1 - 1e-12, lam))) + 1
    obs = np.bincount(x.astype(np.int64), minlength=hi + 1)
    exp = N_DRAWS * st.poisson.pmf(np.arange(hi + 1), lam)
    exp[-1] += N_DRAWS * st.poisson.sf(hi, lam)
    pv = _chi2_p(obs, exp)
    print(f"rpois lam={lam} seed={seed}: chi2 p {pv:.4f}, mean {x.mean():.4f}, var {x.var(ddof=1):.4f}, attempts/draw {att.mean():.4f}")
    assert pv > 1e-4, (lam, seed, pv)
    if lam < 10.0:
        assert (att == 1).all()                     # inversion: one block per draw


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("lam", [1e-6, 1e6, 1.6e7])
def test_mean_and_variance(oracle_lib, lam, seed):
    x, att = _draws(lam, seed)
    n = float(N_DRAWS)
    assert (x >= 0).all() and (x == np.floor(x)).all()
    se_m = math.sqrt(lam / n)
    se_v = math.sqrt(((lam + 3.0 * lam * lam) - lam * lam * (n - 3.0) / (n - 1.0)) / n)
    print(f"rpois lam={lam} seed={seed}: mean err {(x.mean() - lam) / se_m:+.2f} se, var err {(x.var(ddof=1) - lam) / se_v:+.2f} se, attempts/draw {att.mean():.4f}")
    assert abs(x.mean() - lam) < 4.5 * se_m
    assert abs(x.var(ddof=1) - lam) < 4.5 * se_v


@pytest.mark.parametrize("lam", [10.0, 37.0, 1000.0, 1e6, 1.6e7])
def test_attempts_of_the_rejection_branch(oracle_lib, lam):
    att = np.concatenate([_draws(lam, seed)[1] for seed in SEEDS])
    rate = 1.0 / att.mean()
    print(f"rpois lam={lam}: {att.mean():.4f} attempts per draw (acceptance {rate:.4f}), most {att.max()}")
    alpha = 1.1239 + 1.1328 / ((0.931 + 2.53 * math.sqrt(lam)) - 3.4)
    print(f"    alpha {alpha:.4f}, 1 / alpha {1.0 / alpha:.4f}")
    assert att.min() >= 1 and att.max() < 60         # (1 - 1 / 1.33)^59 ~ 1e-36
    assert abs(att.mean() - alpha) <= 0.02 * alpha + 4.5 * math.sqrt(alpha * (alpha - 1.0) / att.size)


def test_the_loop_ends_for_the_extreme_uniforms(oracle_lib):
    top, low = 1.0 - 2.0 ** -53, 2.0 ** -53          # the largest and smallest value of u52
    assert oracle_lib.lib().orc_t_u52(0xFFFFFFFF, 0xFFFFFFFF) == top and oracle_lib.lib().orc_t_u52(0, 0) == low
    for lam in (1e-6, 0.3, 9.999999999999998):
        x, att = R.rpois_from(iter([(top, top)]), lam)
        print(f"rpois lam={lam}: the largest uniform gives {x}")
        # the search ends where the rounded sum of the masses reaches the uniform, at the stated cap if it never does; either way far in the tail
        assert att == 1 and x == math.floor(x) and st.poisson.ppf(1.0 - 1e-12, lam) <= x <= R.RPOIS_CAP
        assert R.rpois_from(iter([(low, low)]), lam) == (0.0, 1)
    mid = (0.5, 0.1)                                  # us = 0.5, V = 0.1 <= vr (0.405 at lam = 10, more above): the squeeze accepts k = floor(lam + 0.43)
    for lam in (10.0, 37.0, 1e6, 2.0 ** 24):
        for u in (top, low):
            for v in (top, low, 0.5):
                x, att = R.rpois_from(iter([(u, v), mid]), lam)   # the extreme attempt is rejected, the next one decides
                assert att == 2 and x == math.floor(lam + 0.43), (lam, u, v, x, att)
    # no acceptance at all: the attempt limit ends the loop with floor(lam)
    assert R.rpois_from(iter([(top, top)] * R.MAX_ATTEMPTS), 37.5) == (37.0, R.MAX_ATTEMPTS)


def test_a_draw_depends_on_its_stream_coordinates_alone(oracle_lib):
    a, _ = R.rpois_vec([3.0, 50.0, 3.0, 50.0], seed=7, chain=2, elem0=10, it=5)
    b0 = R.rpois(3.0, seed=7, chain=2, elem=12, it=5)[0]
    b1 = R.rpois(50.0, seed=7, chain=2, elem=13, it=5)[0]
    assert a[2] == b0 and a[3] == b1
    x = np.array([R.rpois(50.0, seed=7, chain=c, elem=e, it=t)[0] for c in (0, 1) for e in (0, 1) for t in (1, 2)])
    assert len(set(x)) > 1


def _fit_samples(P, E, S, rng, jitter=0.02):
    """S 'posterior samples' around (P, E): the signatures as given, the exposures jittered"""
    K, N = P.shape
    Ps = np.repeat(P[None], S, axis=0)
    Es = np.stack([E * rng.gamma(1.0 / jitter ** 2, jitter ** 2, size=E.shape) for _ in range(S)])
    return Ps, Es, np.ones((S, N))


def test_ppc_of_a_well_specified_fit_and_of_planted_misfits(oracle_lib):
    rng = np.random.default_rng(5)
    K, G, N, S = 16, 40, 3, 50
    P = rng.dirichlet(np.full(K, 0.5), size=N).T                    # K x N signatures
    E = rng.gamma(2.0, 150.0, size=(N, G))
    M = rng.poisson(P @ E).astype(np.int32)
    Ps, Es, As = _fit_samples(P, E, S, rng)
    iters = np.arange(101, 101 + S)
    good = R.ppc_reference(Ps, Es, As, None, M, "poisson", iters, seed=3)
    p1 = good["col"][2]
    ks = st.kstest(p1, "uniform").pvalue
    print(f"well specified: column p(T1) min {p1.min():.2f} max {p1.max():.2f} KS p {ks:.3f}; p_T1 {good['p_T1']:.2f}; tail cells {good['n_tail_cells']} of {K * G}")
    assert ks > 1e-3 and p1.min() < 0.25 and p1.max() > 0.75        # spread over (0, 1)
    assert np.array_equal(good["pit"], good["p_less_cell"] + 0.5 * good["p_equal_cell"])
    assert np.allclose(good["mean_cell"], (P @ E), rtol=0.35, atol=3.0) and good["n_used"] == S
    # (a) a column generated from a signature the fixed P lacks: the refit can only match its total
    q = rng.dirichlet(np.full(K, 0.5))
    Mb = M.copy()
    Mb[:, 0] = rng.poisson(q * E[:, 0].sum())
    bad = R.ppc_reference(Ps, Es, As, None, Mb, "poisson", iters, seed=3)
    print(f"absent signature: p(T1) of column 0 {bad['col'][2, 0]:.3f} (T1 data {bad['col'][0, 0]:.1f}, replicate {bad['col'][1, 0]:.1f})")
    assert bad["col"][2, 0] <= 0.02 and bad["col"][0, 0] > 3.0 * bad["col"][1, 0]
    assert np.array_equal(bad["col"][:, 1:], good["col"][:, 1:])      # the other columns: the same replicates, the same data
    # (b) data with twice the Poisson variance (a gamma-mixed Poisson): E (sqrt(x) - sqrt(lam))^2 doubles from about 1/4 per cell, so the
    # whole-matrix T1 of the data lies some ten standard deviations of the replicates' above theirs, and the mid-PITs move outwards:
    # 1.96 / sqrt(2) standard deviations leave 17 % of the cells outside the central 95 % of their replicates instead of 5 %
    lam = P @ E
    Mo = rng.poisson(rng.gamma(lam, 1.0)).astype(np.int32)           # var = 2 lam
    over = R.ppc_reference(Ps, Es, As, None, Mo, "poisson", iters, seed=3)
    print(f"overdispersed: median column p(T1) {np.median(over['col'][2]):.3f}, whole-matrix p_T1 {over['p_T1']:.3f}, tail cells {over['n_tail_cells']}")
    assert over["p_T1"] <= 0.02
    assert over["n_tail_cells"] > good["n_tail_cells"]
    # the replicate of a cell and iteration does not depend on the range: the last 20 samples alone
    sub = R.ppc_reference(Ps[30:], Es[30:], As[30:], None, M, "poisson", iters[30:], seed=3)
    assert np.array_equal(sub["series"], good["series"][:, 30:]) and np.array_equal(sub["T"], good["T"][:, 30:])


def test_ppc_normal_restatement(oracle_lib):
    rng = np.random.default_rng(8)
    K, G, N, S = 12, 30, 2, 40
    P, E = rng.gamma(1.0, 1.0, size=(K, N)), rng.gamma(2.0, 2.0, size=(N, G))
    sig = np.full((S, G), 0.25)
    M = P @ E + rng.normal(0.0, 0.5, size=(K, G))
    Ps, Es, As = np.repeat(P[None], S, axis=0), np.repeat(E[None], S, axis=0), np.ones((S, N))
    iters = np.arange(1, S + 1)
    r = R.ppc_reference(Ps, Es, As, sig, M, "normal", iters, seed=9, chain=1)
    p1 = r["col"][2]
    ks = st.kstest(p1, "uniform").pvalue
    print(f"normal: column p(T1) KS p {ks:.3f}, p_T2 {r['p_T2']:.2f}, mean T1 data {r['mean_T1_obs']:.1f} replicate {r['mean_T1_rep']:.1f} (K G = {K * G})")
    assert ks > 1e-3
    assert abs(r["mean_T1_rep"] - K * G) < 4.5 * math.sqrt(2.0 * K * G / S) + 1e-9      # a chi-square with K G degrees per sample
    M2 = M.copy()
    M2[:, 4] += rng.normal(0.0, 2.0, size=K)                                              # a column with 17 times the variance
    b = R.ppc_reference(Ps, Es, As, sig, M2, "normal", iters, seed=9, chain=1)
    assert b["col"][2, 4] == 0.0 and b["col"][5, 4] <= 0.05


def test_get_PPC_ranges_idx_and_result(tmp_path):
    """bayesNMF_sampler.get_PPC over a stub engine: the range and idx rules of get_WAIC (_recorded_range), the shape of the result"""
    from test_waic_host import _NoWaicEngine
    from bayesnmf_amd.sampler import bayesNMF_sampler
    from bayesnmf_amd.convergence import new_convergence_control
    from bayesnmf_amd.setup import synth_counts

    class _PpcEngine(_NoWaicEngine):
        calls = []

        def ppc(self, last_n, used=None, end_iter=None, pointwise=False):
            type(self).calls.append(dict(last_n=last_n, used=None if used is None else np.array(used), end_iter=end_iter, pointwise=pointwise))
            S = last_n if used is None else int(np.sum(used))
            K, G = self.K, self.G
            out = dict(n_used=S, n_tail_cells=3, p_T1=0.5, p_T2=0.25, mean_T1_obs=1.0, mean_T1_rep=2.0, mean_T2_obs=3.0, mean_T2_rep=4.0)
            out.update({k: np.full(G, float(i)) for i, k in enumerate(("T1_obs_col", "T1_rep_col", "p_T1_col", "T2_obs_col", "T2_rep_col", "p_T2_col"))})
            out.update({k: np.full(S, float(i)) for i, k in enumerate(("T1_obs", "T1_rep", "T2_obs", "T2_rep"))})
            if pointwise:
                out.update({k: np.full((K, G), 0.25) for k in ("mean_cell", "var_cell", "p_less_cell", "p_equal_cell")})
                out["pit"] = out["p_less_cell"] + 0.5 * out["p_equal_cell"]
            return out

    M, _, _ = synth_counts(12, 9, 2, 3, mean_total=200)
    cc = new_convergence_control()
    cc.update(MAP_over=4, MAP_every=2, maxiters=10, miniters=2)
    s = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "r"), engine_factory=_PpcEngine,
                         convergence_control=cc, save_all_samples=True, periodic_save=False)
    s.run_gibbs_sampler()
    log_before = open(s.log_file).read() if hasattr(s, "log_file") and s.log_file else None
    r = s.get_PPC()
    assert _PpcEngine.calls[-1]["last_n"] == 4 and not _PpcEngine.calls[-1]["pointwise"]
    assert r["p_T1"] == 0.5 and r["n_tail_cells"] == 3 and "pit" not in r
    assert list(r["col"].columns) == ["T1_obs", "T1_rep", "p_T1", "T2_obs", "T2_rep", "p_T2"] and len(r["col"]) == 9
    assert list(r["series"].columns) == ["T1_obs", "T1_rep", "T2_obs", "T2_rep"] and len(r["series"]) == r["n_used"]
    r = s.get_PPC(end_iter=8, n_samples=5, idx=[4, 6, 8], pointwise=True)
    c = _PpcEngine.calls[-1]
    assert c["end_iter"] == 8 and c["last_n"] == 5 and np.array_equal(c["used"], [1, 0, 1, 0, 1]) and c["pointwise"]
    assert r["pit"].shape == (12, 9) and len(r["series"]) == 3
    s.get_PPC(end_iter=8, n_samples=5, idx=None)
    assert _PpcEngine.calls[-1]["used"] is None
    with pytest.raises(ValueError, match="not all recorded"):
        s.get_PPC(end_iter=12, n_samples=3)
    if log_before is not None:
        assert open(s.log_file).read() == log_before            # no new log lines
    s.close()
    t = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "one"), engine_factory=_NoWaicEngine)
    with pytest.raises(ValueError, match="get_PPC needs an engine"):
        t.get_PPC()
    t.close()
