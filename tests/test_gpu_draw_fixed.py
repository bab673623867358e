"""The geometry-fixed form of the merged draw kernel (csrc/kernels.h k_draw_fixed<DrawFixed<96, 20, 896, Gamma, recording>>)
against the dynamic form of the same body (BNMF_DRAWFIXED=0) and against the oracle, bit for bit: P, E, ZsumK, ZsumG, the prior parameters,
every recorded array of every retained sample and the metrics rows, over 6 iterations in two calls (3 + 3: a call boundary, both t & 1
slots).  K = 96 and N = 20 are what the fixed form is built for; BNMF_GATE=1 forces the merged draw kernel at these small G and
BNMF_DRAWBW=896 the workgroup width the fixed form needs (at full size the host chooses it by itself).  The switches are read at
bnmf_create (BNMF_DRAWBW at the handle's first merged launch): the forms are handles of one process.
WHICH FORM A HANDLE LAUNCHED IS INFERRED, NOT OBSERVED (no stat index reports it; the export list and the stat list are pinned): _takes_fixed
is a Python copy of sweep.h draw_fixed_form and asserts only on its own constants.  Statistic 10 shows that the merged draw kernel ran, not
which form of it.  If the BNMF_DRAWBW override or the selection rule quietly fell back to k_draw, the fixed-against-dynamic comparisons
here would pass trivially: that the rule does select k_draw_fixed rests ONLY on the kernel names in
profiles/r07_bench_kernel_stats_after.csv, which come from the bench shape (G = 10,000), not from the shapes of this file."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
K, N, W = 96, 20, 8
CALLS = (3, 3)
PRIORS = dict(gamma=["Alpha_p", "Beta_p", "Alpha_e", "Beta_e"], exponential=["Lambda_p", "Lambda_e"])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _takes_fixed(k, n, prior, window, n_fixed, drawfixed_env, bw=896):
    return k == 96 and n == 20 and prior == "gamma" and bw == 896 and window > 0 and n_fixed == 0 and drawfixed_env != "0"


def _data(k, g, nzero=0):
    from bayesnmf_amd.setup import synth_counts
    M = synth_counts(k, g, 3, 21, mean_total=1500)[0].copy()
    if nzero:
        M[:, np.random.default_rng(5).choice(g, size=nzero, replace=False)] = 0
    return np.asfortranarray(M)


def _setup(c, prior, M, n, a_off, P0, mask):
    from bayesnmf_amd.setup import apply_hyperprior_params
    apply_hyperprior_params(c, prior, M, n)
    if a_off is not None:
        A = np.ones(n)
        A[a_off] = 0.0
        c.set("A", A)
    if P0 is not None:
        c.set("P", P0)
    if mask is not None and hasattr(c, "set_fixed"):
        c.set_fixed("P", mask)


def _names(prior):
    return ["P", "E", "A", "R"] + PRIORS[prior]


def _engine_chain(M, n, prior, window, drawfixed, monkeypatch, a_off=None, no_p=False, P0=None, mask=None):
    """{"metrics": 6 rows, "state": after each call, "samples": name -> the 6 recorded samples}"""
    from bayesnmf_amd import Engine
    monkeypatch.setenv("BNMF_GATE", "1")
    monkeypatch.setenv("BNMF_DRAWBW", "896")
    if no_p:
        monkeypatch.setenv("BNMF_DEBUG_DRAW_NO_P", "1")
    if drawfixed is None:
        monkeypatch.delenv("BNMF_DRAWFIXED", raising=False)
    else:
        monkeypatch.setenv("BNMF_DRAWFIXED", drawfixed)
    e = Engine(M, n, prior=prior, seed=3, window=window)
    _setup(e, prior, M, n, a_off, P0, mask)
    e.init()
    rows, state = [], []
    for c in CALLS:
        rows.append(e.run(c)[:, :9].copy())
        state.append({nm: e.get(nm).copy() for nm in _names(prior) + ["ZsumK", "ZsumG"]})
    assert e.stat(10) > 0, "the merged draw kernel never ran"
    samples = {nm: [s.copy() for s in e.window(nm, sum(CALLS))] for nm in _names(prior)} if window else {}
    e.close()
    for v in ("BNMF_GATE", "BNMF_DRAWBW", "BNMF_DEBUG_DRAW_NO_P", "BNMF_DRAWFIXED"):
        monkeypatch.delenv(v, raising=False)
    return {"metrics": np.concatenate(rows), "state": state, "samples": samples}


def _oracle_chain(M, n, prior, a_off=None, P0=None, fixed_cols=None):
    """the oracle one iteration at a time: what the engine records is the state behind each iteration.  fixed_cols: the composed reference of
    tests/test_gpu_fixed.py (the P step, then the fixed columns restored)"""
    import oracle as O
    o = O.Oracle(M, n, prior=prior, seed=3, nthreads=8)
    _setup(o, prior, M, n, a_off, P0, None)
    o.init()
    rows, per_iter = [], []
    for t in range(2, sum(CALLS) + 2):
        if fixed_cols is None:
            rows.append(o.run(1)[0, :9].copy())
        else:
            for what in ("hyper", "P", "E", "Z"):
                o.step(what, t)
                if what == "P":
                    P = o.get("P"); P[:, fixed_cols] = P0[:, fixed_cols]; o.set("P", P)
        per_iter.append({nm: o.get(nm).copy() for nm in _names(prior) + ["ZsumK", "ZsumG"]})
    o.close()
    return {"metrics": np.array(rows) if rows else None, "per_iter": per_iter}


def _same_forms(a, b):
    assert np.array_equal(_bits(a["metrics"]), _bits(b["metrics"])), "metrics rows"
    for i, (x, y) in enumerate(zip(a["state"], b["state"])):
        for nm in x:
            assert np.array_equal(_bits(x[nm]), _bits(y[nm])), (nm, "call", i)
    assert a["samples"].keys() == b["samples"].keys()
    for nm in a["samples"]:
        for i, (x, y) in enumerate(zip(a["samples"][nm], b["samples"][nm])):
            assert np.array_equal(_bits(x), _bits(y)), (nm, "sample", i)


def _same_as_oracle(a, o, prior):
    if o["metrics"] is not None:
        assert np.array_equal(_bits(a["metrics"]), _bits(o["metrics"])), "metrics rows"
    ends = np.cumsum(CALLS) - 1
    for i, st in enumerate(a["state"]):
        for nm in st:
            assert np.array_equal(_bits(st[nm]), _bits(o["per_iter"][ends[i]][nm])), (nm, "call", i)
    for nm in a["samples"]:
        for i, x in enumerate(a["samples"][nm]):
            assert np.array_equal(_bits(x), _bits(o["per_iter"][i][nm])), (nm, "sample", i)


CASES = {
    # G = 131: N G = 2,620 = 2 x 896 + 828, the last wave with 60 live lanes
    "ragged": dict(g=131), "one_workgroup": dict(g=40), "no_p": dict(g=131, no_p=True), "factor_off": dict(g=131, a_off=3),
    "zero_columns": dict(g=131, nzero=100),
}


@pytest.mark.parametrize("case", list(CASES))
def test_fixed_form_is_the_dynamic_form_and_the_oracle(case, monkeypatch):
    c = CASES[case]
    M = _data(K, c["g"], c.get("nzero", 0))
    if "nzero" in c:
        assert (M.sum(0) == 0).sum() >= 100
    kw = dict(a_off=c.get("a_off"), no_p=c.get("no_p", False))
    assert _takes_fixed(K, N, "gamma", W, 0, None) and not _takes_fixed(K, N, "gamma", W, 0, "0")
    fx = _engine_chain(M, N, "gamma", W, None, monkeypatch, **kw)
    dyn = _engine_chain(M, N, "gamma", W, "0", monkeypatch, **kw)
    _same_forms(fx, dyn)
    _same_as_oracle(fx, _oracle_chain(M, N, "gamma", a_off=c.get("a_off")), "gamma")
    if "a_off" in c:
        assert all(np.asarray(s).ravel()[3] == 0.0 for s in fx["samples"]["A"])
    assert fx["state"][-1]["ZsumK"].sum() == M.sum()


@pytest.mark.parametrize("case", ["N = 19", "K = 95", "exponential", "window = 0", "fixed column", "BNMF_DRAWFIXED=0"])
def test_other_configurations_stay_dynamic(case, monkeypatch):
    """What the selection rule must leave to the dynamic form: each is still the oracle's bits, with the switch at its default."""
    k, n = (95 if case == "K = 95" else K), (19 if case == "N = 19" else N)
    prior = "exponential" if case == "exponential" else "gamma"
    window = 0 if case == "window = 0" else W
    env = "0" if case == "BNMF_DRAWFIXED=0" else None
    M = _data(k, 131)
    P0 = mask = cols = None
    if case == "fixed column":
        mask = np.zeros(n, dtype=np.int32); mask[[2, 7]] = 1
        cols = np.flatnonzero(mask)
        P0 = np.asfortranarray(np.random.default_rng(17).gamma(1.0, 1.0, size=(k, n)) * 0.05)
    assert not _takes_fixed(k, n, prior, window, 0 if mask is None else int(mask.sum()), env)
    a = _engine_chain(M, n, prior, window, env, monkeypatch, P0=P0, mask=mask)
    _same_as_oracle(a, _oracle_chain(M, n, prior, P0=P0, fixed_cols=cols), prior)
