"""Real-valued data for the Normal likelihood on the device (bnmf_create_f64).

* integer data give the same chain, bit for bit, through bnmf_create_f64 (fp64) and bnmf_create (int32), in every form of the
  Normal kernels — and both equal the CPU oracle;
* on real data — fractional and negative cells, values that truncation and floor map differently, signed zeros, cells in (0, 1e-6),
  at 1e-6 and just below 1, an all-negative row and column, a cell of 1e6 — every form of the Normal kernels, and the edge shapes
  (K = 97, K = 130, G = 1, N = 1, rank learning whose inclusion draws flip), equal the oracle bit for bit, which reads the same fp64
  data: the init row, every metric row, the state after calls of uneven length and every sample of the recorded window; so do the
  committed real-data golden chain and a run with every side-stream kernel held back;
* on real data with fractional parts and negative cells the metric rows are the reference's metrics of the recorded samples;
* the full conditionals of P and sigmasq are the reference's laws of the REAL data (a floored copy of the data is detected);
* bayesNMF() on P E + noise of small magnitude recovers the signatures."""
import ctypes as C

import numpy as np
import pytest
import scipy.stats as st
from scipy.optimize import linear_sum_assignment
from scipy.special import gammaincc, ndtr

pytestmark = pytest.mark.gpu


def _engine_i32(M, N, likelihood="normal", prior="exponential", learning_rank=False, seed=1, window=0, device=0):
    """an Engine whose handle comes from bnmf_create (int32 data) whatever the likelihood: the entry point the Normal model had before"""
    from bayesnmf_amd.engine import Engine, BnmfConfig, LIKELIHOOD, PRIOR, lib, _chk, _run_fn
    M = np.asfortranarray(M, dtype=np.int32)
    e = Engine.__new__(Engine)
    e.K, e.G = M.shape
    e.N, e._temp = int(N), None
    cfg = BnmfConfig(e.K, e.G, e.N, LIKELIHOOD[likelihood], PRIOR[prior], 0, int(learning_rank), 0, 0, int(window), int(seed), 0,
                     int(device), None, 0)
    h = C.c_void_p()
    _chk(lib().bnmf_create(C.byref(cfg), M.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(h)))
    e._h, e._hv, e._run, e.M = h, h.value, _run_fn(), M
    return e


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b, what):
    assert np.array_equal(_bits(a), _bits(b)), what


PRIOR_IDS = dict(exponential=["Lambda_p", "Lambda_e"], truncnormal=["Mu_p", "Sigmasq_p", "Mu_e", "Sigmasq_e"])

# (name, K, G, N, prior, learning_rank, environment at bnmf_create): every form a Normal handle can take
FORMS = [
    ("fixed-truncnormal", 96, 400, 5, "truncnormal", False, {}),                        # k_mh_prow REG, k_mh_ecol16 16 lanes / 96 rows
    ("fixed-exponential", 96, 400, 5, "exponential", False, {}),
    ("rank-half-block", 96, 300, 5, "exponential", True, {}),                           # k_rank_sweep register form, half blocks
    ("rank-whole-block", 96, 300, 5, "truncnormal", True, {"BNMF_RANKHALF": "0"}),     # ... whole blocks
    ("rank-general", 100, 200, 4, "exponential", True, {}),                             # K > 96: general form; 128-row k_mh_ecol16
    ("ecol16-32-lanes", 96, 300, 5, "exponential", False, {"BNMF_MHE_GW": "32"}),
    ("ecol16-128-rows", 96, 300, 5, "truncnormal", False, {"BNMF_MHE_K128": "1"}),
    ("ecol16-32-lanes-128-rows", 120, 300, 5, "exponential", False, {"BNMF_MHE_GW": "32"}),
    ("ecol", 150, 200, 4, "exponential", False, {}),                                    # K > MHE16_KMAX: k_mh_ecol
    ("prow-segments", 64, 5200, 3, "exponential", False, {}),                           # G > MH_SEG * MHP_W: k_mh_prow without registers
]


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_integer_data_same_bits_through_either_entry_point(form, monkeypatch):
    import oracle as O
    from bayesnmf_amd import Engine
    from bayesnmf_amd.convergence import new_convergence_control
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    name, K, G, N, prior, lr, env = form
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    M, _, _ = synth_counts(K, G, 3, 20251016, mean_total=600.0)
    W = 6
    kw = dict(likelihood="normal", prior=prior, learning_rank=lr, seed=7)
    a = _engine_i32(M, N, window=W, **kw)                                  # int32 counts
    b = Engine(M.astype(np.float64), N, window=W, **kw)                    # the same values as fp64 (bnmf_create_f64)
    assert b.M.dtype == np.float64
    o = O.Oracle(M, N, nthreads=8, **kw)
    for c in (a, b, o):
        apply_hyperprior_params(c, prior, M, N)
    ra, rb, ro = a.init(), b.init(), o.init()
    _same(ra, rb, "init row")
    _same(ra[:9], ro[:9], "init row vs oracle")
    names = ["P", "E", "A", "sigmasq", "Alpha", "Beta"] + PRIOR_IDS[prior]
    for step in range(3):
        ma, mb, mo = a.run(4), b.run(4), o.run(4)
        _same(ma, mb, f"metrics rows, call {step}")
        _same(ma[:, :9], mo[:, :9], f"metrics rows vs oracle, call {step}")
        for nm in names:
            _same(a.get(nm), b.get(nm), f"{nm}, call {step}")
        for nm in ("P", "E", "A", "sigmasq"):
            _same(a.get(nm), o.get(nm), f"{nm} vs oracle, call {step}")
    for nm in ["P", "E", "A", "R", "sigmasq"] + PRIOR_IDS[prior]:
        _same(np.stack(a.window(nm, W)), np.stack(b.window(nm, W)), f"window {nm}")
    pa, pb = a.map(W), b.map(W)
    for key in ("P", "E", "A", "P_lower", "P_upper", "E_lower", "E_upper", "rmse", "kl"):
        _same(pa[key], pb[key], f"map {key}")
    assert np.array_equal(pa["used"], pb["used"]) and pa["n_used"] == pb["n_used"]
    cc = new_convergence_control(MAP_over=W, MAP_every=4, miniters=0, maxiters=a.iter + 12, tol=1e-12)
    ua, ub = a.run_until(cc), b.run_until(cc)
    _same(ua[0], ub[0], "run_until metrics rows")
    _same(ua[1], ub[1], "run_until MAP rows")
    assert bytes(ua[2]) == bytes(ub[2]), "run_until state"
    assert len(ua[1]) >= 2
    for e in (a, b, o):
        e.close()


def test_poisson_integer_float64_data_same_as_bnmf_create():
    """bnmf_create_f64 with whole-number Poisson data converts and continues as bnmf_create: the same chain."""
    from bayesnmf_amd.engine import Engine, BnmfConfig, LIKELIHOOD, PRIOR, lib, _chk, _run_fn
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    M, _, _ = synth_counts(96, 300, 3, 5)
    a = Engine(M, 5, prior="gamma", seed=3, window=4)
    b = Engine.__new__(Engine)
    b.K, b.G, b.N, b._temp = 96, 300, 5, None
    cfg = BnmfConfig(96, 300, 5, LIKELIHOOD["poisson"], PRIOR["gamma"], 0, 0, 0, 0, 4, 3, 0, 0, None, 0)
    h = C.c_void_p()
    Mf = np.asfortranarray(M, dtype=np.float64)
    _chk(lib().bnmf_create_f64(C.byref(cfg), Mf.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h)))
    b._h, b._hv, b._run, b.M = h, h.value, _run_fn(), Mf
    for c in (a, b):
        apply_hyperprior_params(c, "gamma", M, 5)
    _same(a.init(), b.init(), "init row")
    for step in range(3):
        _same(a.run(5), b.run(5), f"metrics rows, call {step}")
        for nm in ("P", "E", "Alpha_p", "Beta_e"):
            _same(a.get(nm), b.get(nm), nm)
        assert np.array_equal(a.get("ZsumK"), b.get("ZsumK"))
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------- real data: parity with the oracle
EDGE = [-0.5, 0.7, 0.0, -0.0, 5e-7, 1e-6, np.nextafter(1.0, 0.0), 0.999999]   # trunc / floor differ; signed zeros; the KL's pmax edge
RANK_TEMP = np.concatenate([np.zeros(3), 10.0 ** np.linspace(-4, 0, 9), np.ones(10)])   # cold start: the inclusion draws flip


def _edge_real(K, G, seed, big=False):
    """P E + N(0, 0.5^2) with magnitudes around 1, fractional everywhere, some cells negative, plus the EDGE values (down column 0,
    wrapping to the next columns), an all-negative last column and last row (where the shape leaves others), and with big one cell
    of magnitude 1e6"""
    rng = np.random.default_rng(seed)
    M = rng.gamma(4.0, 0.06, size=(K, 3)) @ rng.gamma(4.0, 0.3, size=(3, G)) + rng.normal(0.0, 0.5, size=(K, G))
    M = np.asfortranarray(M)
    for i, v in enumerate(EDGE[:K * G]):
        M[i % K, i // K] = v
    if G >= 3:
        M[:, G - 1] = -np.abs(M[:, G - 1]) - 0.01
    if K >= 3:
        M[K - 1, :] = -np.abs(M[K - 1, :]) - 0.01
    if big:
        M[K // 2, G // 2] = 1.234567e6
    if M.mean() <= 0:                                     # the default hyper-priors take sqrt(mean(M))
        M[K // 2, 0] += 1.0 - M.sum()
    return M


def _parity_real(M, N, prior, learning_rank=False, rank_method="SBFI", temperature=None, seed=3, calls=(1, 4, 7), W=7):
    """Engine (bnmf_create_f64) against the oracle (orc_create_f64) on real data, bit for bit: the init row, every metric row, P, E, A, R,
    sigmasq and the prior-parameter arrays after each call, and every sample of the recorded window against the oracle's state at that
    iteration.  Returns the metric rows."""
    import oracle as O
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import apply_hyperprior_params
    kw = dict(likelihood="normal", prior=prior, learning_rank=learning_rank, rank_method=rank_method, temperature=temperature, seed=seed)
    o = O.Oracle(M, N, nthreads=8, **kw)
    e = Engine(M, N, window=W, **kw)
    assert o.M.dtype == np.float64 and e.M.dtype == np.float64
    for c in (o, e):
        apply_hyperprior_params(c, prior, M, N)
    ro, re_ = o.init(), e.init()
    _same(re_[:9], ro[:9], "init row")
    names = ["P", "E", "A", "R", "sigmasq", "Alpha", "Beta"] + PRIOR_IDS[prior]
    hist, rows = [], [ro]
    for c, n in enumerate(calls):
        me = e.run(n)
        mo = []
        for _ in range(n):
            mo.append(o.run(1)[0])
            hist.append({nm: o.get(nm).copy() for nm in names})
        mo = np.array(mo)
        rows += list(mo)
        for i in range(n):
            _same(me[i, :9], mo[i, :9], f"metric row {i} of call {c} (iteration {o.iter - n + i + 1})")
        for nm in names:
            _same(e.get(nm), o.get(nm), f"{nm} after call {c}")
    for nm in ("P", "E", "A", "R", "sigmasq") + tuple(PRIOR_IDS[prior]):
        win = e.window(nm, W)
        for j in range(W):
            _same(win[j], hist[len(hist) - W + j][nm], f"window {nm}, sample {j}")
    o.close(); e.close()
    return np.array(rows)


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_real_data_parity_with_the_oracle_in_every_form(form, monkeypatch):
    """Every form a Normal handle can take, on real data with the EDGE cells and an all-negative row and column, against the oracle that
    reads the same fp64 data.  The rank forms run with a cold start, so that the inclusion draws flip."""
    name, K, G, N, prior, lr, env = form
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    M = _edge_real(K, G, 1000 + K + G)
    rows = _parity_real(M, N, prior, learning_rank=lr, temperature=RANK_TEMP if lr else None, seed=7)
    if lr:
        assert len(np.unique(rows[:, 7])) >= 2, "the rank never moved: the rank sweep's decisions are untested"


EDGE_SHAPES = [
    ("K97", 97, 60, 3, "exponential", False, False),                  # wave tails of the column kernels
    ("K97-rank", 97, 60, 4, "truncnormal", True, False),
    ("K130", 130, 40, 3, "truncnormal", False, False),                # above MHE16_KMAX: k_mh_ecol
    ("K130-rank", 130, 40, 3, "exponential", True, False),
    ("G1", 12, 1, 3, "truncnormal", False, False),
    ("N1", 40, 30, 1, "exponential", False, False),
    ("cell-1e6", 64, 80, 3, "exponential", False, True),
    ("BFI", 40, 50, 4, "exponential", True, False),
]


@pytest.mark.parametrize("case", EDGE_SHAPES, ids=[c[0] for c in EDGE_SHAPES])
def test_real_data_parity_at_edge_shapes(case):
    name, K, G, N, prior, lr, big = case
    M = _edge_real(K, G, 2000 + K + G, big=big)
    rows = _parity_real(M, N, prior, learning_rank=lr, rank_method="BFI" if name == "BFI" else "SBFI",
                        temperature=RANK_TEMP if lr else None, seed=11)
    if lr:
        assert len(np.unique(rows[:, 7])) >= 2, "the rank never moved"


def test_real_data_with_every_side_stream_kernel_held_back(monkeypatch):
    """test_gpu_parity.py's test_every_side_stream_kernel_held_back on real data: a 400 us delay in front of every side-stream kernel."""
    monkeypatch.setenv("BNMF_DEBUG_ALLSIDE_DELAY_US", "400")
    _parity_real(_edge_real(60, 400, 991), 4, "truncnormal", calls=(7, 6), W=6)


def test_randomised_parity_sweep_with_real_data():
    """tools/fuzz_parity.py with FUZZ_REAL=1: the 60 cases of test_gpu_configs.py's sweep, half of the Normal ones on real-valued data
    (fractional and negative cells, large ones among them), engine against the oracle, bit-exact."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FUZZ_N="60", FUZZ_SEED="77", FUZZ_REAL="1")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_parity.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_engine_matches_golden_chain_of_real_data():
    """The HIP engine against the committed real-data golden chain (tests/golden/make_golden.py normal_golden)."""
    import os
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import apply_hyperprior_params
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nt_sbfi_real_k12_g10_n3.npz"))
    M, N = g["M"], g["P"].shape[1]
    e = Engine(M, N, likelihood="normal", prior="truncnormal", learning_rank=True, seed=5, temperature=g["temperature"])
    apply_hyperprior_params(e, "truncnormal", M, N)
    rows = [e.init()] + list(e.run(g["metrics"].shape[0] - 1))
    _same(np.array(rows)[:, :9], g["metrics"][:, :9], "metric rows")
    for nm in ("P", "E", "A", "R", "sigmasq") + tuple(PRIOR_IDS["truncnormal"]):
        _same(e.get(nm), g[nm], nm)
    e.close()


# ---------------------------------------------------------------------------------------------- real data: metrics
def _real_data(K, G, R, seed, sd=0.4, e_scale=8.0):
    """M = P E + N(0, sd^2): magnitudes around 1 (e_scale = 8; 4: around 0.5), fractional everywhere, some cells negative"""
    rng = np.random.default_rng(seed)
    P = rng.dirichlet(0.5 * np.ones(K), size=R).T
    E = rng.gamma(4.0, e_scale * K / 96.0, size=(R, G))
    M = P @ E + rng.normal(0.0, sd, size=(K, G))
    return np.asfortranarray(M), P, E


def _fit_terms(M, Mhat):
    mt, mh = np.maximum(M, 1e-6), np.maximum(Mhat, 1e-6)
    return (Mhat - M) ** 2, mt * (np.log(mt) - np.log(mh))


def _close(dev, terms, what):
    """dev against the exact sum of the terms: rtol 1e-12 of the sum (or of the sum of magnitudes, where the terms cancel)"""
    import math
    ref = math.fsum(np.ravel(terms))
    scale = max(abs(ref), math.fsum(np.abs(np.ravel(terms))))
    assert abs(dev - ref) <= 1e-12 * scale, f"{what}: {dev!r} vs {ref!r}"


@pytest.mark.parametrize("prior", ["exponential", "truncnormal"])
def test_metrics_of_real_data_are_the_reference_metrics(prior):
    """RMSE, KL (pmax(M, 1e-6), R/utils.R:467-470), log-likelihood (dnorm, R/utils.R:84-96) and log-posterior of every recorded
    iteration, and the MAP's RMSE / KL, restated in numpy from the recorded samples and the REAL data.  On truncated data they
    would not match."""
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import apply_hyperprior_params
    K, G, N, W = 96, 300, 4, 12
    M, _, _ = _real_data(K, G, 3, 11)
    assert (M < 0).sum() > 50 and (M < 1).mean() > 0.2
    e = Engine(M, N, likelihood="normal", prior=prior, seed=5, window=W)
    apply_hyperprior_params(e, prior, M, N)
    e.init()
    e.run(20)
    rows = e.run(W)
    rec = {nm: e.window(nm, W) for nm in ["P", "E", "A", "sigmasq"] + PRIOR_IDS[prior]}
    for i in range(W):
        P, E, A, sg = rec["P"][i], rec["E"][i], rec["A"][i], rec["sigmasq"][i]
        Mhat = (P * A) @ E
        se, kl = _fit_terms(M, Mhat)
        assert rows[i, 1] == pytest.approx(np.sqrt(se.sum() / (K * G)), rel=1e-12, abs=0)
        _close(rows[i, 2], kl, f"KL, row {i}")
        ll = st.norm.logpdf(M, Mhat, np.sqrt(sg)[None, :])
        _close(rows[i, 3], ll, f"loglikelihood, row {i}")
        if prior == "exponential":
            lp = [np.log(rec["Lambda_p"][i]) - rec["Lambda_p"][i] * P, np.log(rec["Lambda_e"][i]) - rec["Lambda_e"][i] * E]
        else:
            lp = []
            for X, mu, s2 in ((P, rec["Mu_p"][i], rec["Sigmasq_p"][i]), (E, rec["Mu_e"][i], rec["Sigmasq_e"][i])):
                sd = np.sqrt(s2)
                lp.append(st.norm.logpdf(X, mu, sd) - st.norm.logcdf(mu / sd))      # truncated at 0
        _close(rows[i, 4], np.concatenate([ll.ravel()] + [x.ravel() for x in lp]), f"logposterior, row {i}")
    m = e.map(W)
    Mhat = (m["P"] * m["A"]) @ m["E"]
    se, kl = _fit_terms(M, Mhat)
    assert m["rmse"] == pytest.approx(np.sqrt(se.sum() / (K * G)), rel=1e-12, abs=0)
    _close(m["kl"], kl, "MAP KL")
    e.close()


# ---------------------------------------------------------------------------------------------- real data: laws
def _law_pits(M_device, M_law, n_rep, seed):
    """Repeat `set P, E, sigmasq and the hyper arrays; run(1)` on a small Normal-Exponential handle holding M_device; return the PIT
    values of P[:, 0] under its truncated-normal full conditional (R/sample_Pn.R:131-181) and of sigmasq under
    InvGamma(Alpha + K/2, Beta + ss/2) (R/sample_params.R:275-286), both computed with M_law."""
    from bayesnmf_amd import Engine
    K, G = M_law.shape
    N = 3
    rng = np.random.default_rng(seed)
    P0 = rng.gamma(4.0, 0.04, size=(K, N))
    E0 = rng.gamma(4.0, 0.5, size=(N, G))
    sg0 = np.full(G, 0.15)
    hyper = dict(A_p=[8.0], B_p=[4.0], A_e=[8.0], B_e=[4.0], Alpha=[3.0], Beta=[3.0])
    e = Engine(M_device, N, likelihood="normal", prior="exponential", seed=seed)
    for k, v in hyper.items():
        e.set(k, v)
    e.set("P", P0); e.set("E", E0); e.set("sigmasq", sg0)
    e.init()
    pit_p, pit_s = [], []
    # P[:, 0] is the first factor the row sweep draws: its conditional involves only the state that was set and this call's Lambda_p
    Mno0 = M_law - P0[:, 1:] @ E0[1:, :]
    num1 = (Mno0 * E0[0][None, :] / sg0[None, :]).sum(1)
    den = (E0[0] ** 2 / sg0).sum() * np.ones(K)
    for _ in range(n_rep):
        for k, v in hyper.items():
            e.set(k, v)
        e.set("P", P0); e.set("E", E0); e.set("sigmasq", sg0)
        e.run(1)
        lam = e.get("Lambda_p")[:, 0]
        mu, sd = (num1 - lam) / den, 1.0 / np.sqrt(den)
        lo = ndtr(-mu / sd)
        pit_p.append((ndtr((e.get("P")[:, 0] - mu) / sd) - lo) / (1.0 - lo))
        P, E, sg = e.get("P"), e.get("E"), e.get("sigmasq")
        ss = ((M_law - P @ E) ** 2).sum(0)
        pit_s.append(gammaincc(3.0 + K / 2.0, (3.0 + ss / 2.0) / sg))           # P(X <= x) for X ~ InvGamma(a, b) = Q(a, b / x)
    e.close()
    return np.concatenate(pit_p), np.concatenate(pit_s)


def test_full_conditionals_of_real_data_and_floored_control():
    K, G = 12, 10
    rng = np.random.default_rng(21)
    M = np.asfortranarray(rng.gamma(4.0, 0.04, size=(K, 3)) @ rng.gamma(4.0, 0.5, size=(3, G)) + rng.normal(0.0, 0.5, size=(K, G)))
    assert (M < 0).any() and (M != np.floor(M)).all()
    pp, ps = _law_pits(M, M, 2000, 31)
    assert st.kstest(pp, "uniform").pvalue > 1e-3, "P[:, 0] under its full conditional"
    assert st.kstest(ps, "uniform").pvalue > 1e-3, "sigmasq under its full conditional"
    # negative control: the device holds floor(M), the laws are those of M — the test must see it
    cp, cs = _law_pits(np.asfortranarray(np.floor(M)), M, 2000, 31)
    assert st.kstest(cp, "uniform").pvalue < 1e-6
    assert st.kstest(cs, "uniform").pvalue < 1e-6


# ---------------------------------------------------------------------------------------------- end to end
# measured (tools/normal_real_e2e.py): at e_scale = 40, sd = 1.5 engine seeds 1-4 learned rank 3 with every assigned cosine
# >= 0.988 (seed 5: rank 2, cosines 0.971 / 0.843); the test runs seed 1 and its threshold keeps margin.  At magnitudes below about 3 (e_scale = 4, sd = 0.3) the model — with the reference's
# fixed InvGamma(3, 3) prior on sigmasq, which then dominates the residual sum of squares — learned rank 1 on every seed: there only
# the run itself is asserted.
COS_MIN = 0.9


@pytest.mark.parametrize("e_scale,sd,recover", [(40.0, 1.5, True), (4.0, 0.3, False)])
def test_bayesNMF_on_real_data(tmp_path, e_scale, sd, recover):
    """M = P E + N(0, sd^2), real-valued with negative cells: bayesNMF(M, rank = 1:6, likelihood = "normal") ends with finite metrics;
    where the signal stands above the noise prior, its MAP recovers the three signatures (Hungarian assignment of the cosines)."""
    from bayesnmf_amd.sampler import bayesNMF
    M, Ptrue, _ = _real_data(96, 200, 3, 7, sd=sd, e_scale=e_scale)
    assert (M < 0).mean() > 0.05 and (M != np.floor(M)).all()
    s = bayesNMF(M, rank=np.arange(1, 7), likelihood="normal", output_dir=str(tmp_path / "n"), periodic_save=False, seed=1)
    sm = s.state["sample_metrics"]
    assert np.isfinite(sm[["RMSE", "KL", "loglikelihood", "logposterior"]].to_numpy()).all()
    P = np.asarray(s.MAP["P"])
    assert P.shape[1] >= 1 and np.isfinite(P).all()
    if recover:
        assert P.shape[1] >= 3
        cos = (P / np.linalg.norm(P, axis=0)).T @ (Ptrue / np.linalg.norm(Ptrue, axis=0))
        r, c = linear_sum_assignment(-cos)
        assert len(c) == 3 and (cos[r, c] >= COS_MIN).all(), cos[r, c]
    s.close()
