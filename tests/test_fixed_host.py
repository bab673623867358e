"""Fixed columns of P (refit to a known catalogue), the parts that need no GPU: the two new symbols are declared, exported, bound and
registered; the CPU oracle composed one conditional at a time (Oracle.step) is the chain Oracle.run gives — which makes "the sweep
without STEP_P" a fair reference for tests/test_gpu_fixed.py; and bayesNMF_sampler's fixed_P argument: every refusal, and placement."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIOR_NAMES = dict(gamma=["Alpha_p", "Beta_p", "Alpha_e", "Beta_e"], exponential=["Lambda_p", "Lambda_e"],
                   truncnormal=["Mu_p", "Sigmasq_p", "Mu_e", "Sigmasq_e"])


def test_new_symbols_declared_exported_bound_and_registered():
    from bayesnmf_amd import engine
    hdr = open(os.path.join(ROOT, "include", "bnmf.h")).read()
    for sym in ("bnmf_set_fixed", "bnmf_get_fixed"):
        assert re.search(r"\bint\s+%s\s*\(\s*bnmf_handle\s*\*" % sym, hdr), f"{sym} not declared in include/bnmf.h"
        assert sym in engine.ABI_SYMBOLS
    so = os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    L = engine.lib()
    for sym in ("bnmf_set_fixed", "bnmf_get_fixed"):
        assert re.search(r"\bT %s$" % sym, exported, re.M), f"{sym} not exported by libbnmf.so"
        assert getattr(L, sym).argtypes is not None and len(getattr(L, sym).argtypes) == 4
    assert hasattr(engine.Engine, "set_fixed") and hasattr(engine.Engine, "get_fixed")
    from rshim import RShim
    R = RShim()
    assert R.routines["C_bnmf_set_fixed"] == 3 and R.routines["C_bnmf_get_fixed"] == 3


# name: likelihood, prior, MH, learning_rank, rank_method
MODELS = {
    "poisson_gamma": ("poisson", "gamma", False), "poisson_exponential": ("poisson", "exponential", False),
    "poisson_exponential_mh": ("poisson", "exponential", True), "poisson_truncnormal_mh": ("poisson", "truncnormal", True),
    "normal_truncnormal": ("normal", "truncnormal", False), "normal_exponential": ("normal", "exponential", False),
}


def _temps():
    return np.concatenate([np.zeros(3), 10.0 ** np.linspace(-6, 0, 12), np.ones(100)])


def _names(lk, prior, MH):
    return ["P", "E", "A", "R"] + PRIOR_NAMES[prior] + (["sigmasq"] if lk == "normal" else ["ZsumK", "ZsumG"] if not MH else [])


def _oracle(model, rank, seed=3):
    import oracle as O
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    lk, prior, MH = MODELS[model]
    K, G, N = 24, 18, 4
    if lk == "normal":
        rng = np.random.default_rng(5)
        M = np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, 2)) @ rng.gamma(2.0, 3.0, size=(2, G)) + rng.normal(0.0, 0.5, size=(K, G)))
    else:
        M, _, _ = synth_counts(K, G, 2, 13, mean_total=300)
    o = O.Oracle(M, N, likelihood=lk, prior=prior, MH=MH, learning_rank=rank is not None, rank_method=rank or "SBFI", seed=seed,
                 temperature=_temps() if rank else None, save_Z=(lk == "poisson" and not MH))
    apply_hyperprior_params(o, prior, M, N)
    o.init()
    return o


def composed_steps(lk, MH, learning_rank, skip_P=False):
    """the order of one iteration of the loop body, as conditionals of Oracle.step"""
    steps = ["hyper"] + ([] if skip_P else ["P"]) + ["E"] + (["R", "A"] if learning_rank else [])
    if lk == "normal":
        steps.append("sigmasq")
    elif not MH:
        steps.append("Z")
    return steps


@pytest.mark.parametrize("rank", [None, "SBFI", "BFI"])
@pytest.mark.parametrize("model", list(MODELS))
def test_oracle_composed_from_steps_is_the_oracle_run(model, rank):
    """Oracle.step in the order HYPER, P, E, [R, A], Z | SIGMASQ over t = 2..T gives the bits of Oracle.run(T - 1), for every state array;
    for the MH models before convergence and after it."""
    lk, prior, MH = MODELS[model]
    T = 12
    for converged in ([False, True] if MH else [False]):
        a, b = _oracle(model, rank), _oracle(model, rank)
        a.run(T - 1, converged=converged)
        for t in range(2, T + 1):
            for what in composed_steps(lk, MH, rank is not None):
                b.step(what, t, converged=converged)
        for nm in _names(lk, prior, MH) + (["Z"] if lk == "poisson" and not MH else []):
            x, y = np.ascontiguousarray(a.get(nm), dtype=np.float64), np.ascontiguousarray(b.get(nm), dtype=np.float64)
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (nm, converged)
        a.close(); b.close()


class _NoFixEngine:
    """what bayesNMF_sampler needs of an engine up to the end of its constructor; records what it was given.  No set_fixed."""
    made = []

    def __init__(self, M, N, **kw):
        self.K, self.G = M.shape
        self.N = N
        self.sets, self.fixed, self.inited_with = {}, None, None
        _NoFixEngine.made.append(self)

    def set(self, name, value):
        self.sets[name] = np.array(value, dtype=float)

    def get(self, name):
        shp = dict(P=(self.K, self.N), E=(self.N, self.G), A=(1, self.N), R=(1,)).get(name, (self.K, self.N) if name.endswith("_p") else (self.N, self.G))
        return np.zeros(shp)

    def init(self):
        self.inited_with = (None if "P" not in self.sets else self.sets["P"].copy(), self.fixed)
        return np.zeros(11)

    def close(self):
        pass


class _StubEngine(_NoFixEngine):
    def set_fixed(self, name, mask):
        assert self.inited_with is None and name == "P"
        self.fixed = np.array(mask)


def _sampler(tmp_path, rank, fixed_P, factory=_StubEngine, **kw):
    from bayesnmf_amd.sampler import bayesNMF_sampler
    from bayesnmf_amd.setup import synth_counts
    M, _, _ = synth_counts(12, 9, 2, 3, mean_total=200)
    return bayesNMF_sampler(M, rank, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "out"), overwrite=True,
                            engine_factory=factory, fixed_P=fixed_P, **kw)


def _sig(K, F, seed=1):
    return np.random.default_rng(seed).dirichlet(np.ones(K), size=F).T


def test_fixed_P_is_placed_in_the_first_columns(tmp_path):
    fp = _sig(12, 2)
    s = _sampler(tmp_path, 5, fp)
    e = _StubEngine.made[-1]
    P0, mask = e.inited_with
    assert np.array_equal(mask, [1, 1, 0, 0, 0])
    assert np.array_equal(P0[:, :2].view(np.uint64), np.asfortranarray(fp).view(np.uint64)) and np.isnan(P0[:, 2:]).all()
    assert np.array_equal(s.specs["fixed_P"], fp)
    s.close()
    # a rank range: the top of the range counts; F == N: a pure refit
    s = _sampler(tmp_path, range(0, 4), fp)                     # ranks 0..3: N = 3
    assert np.array_equal(_StubEngine.made[-1].inited_with[1], [1, 1, 0])
    s.close()
    s = _sampler(tmp_path, 2, fp)
    P0, mask = _StubEngine.made[-1].inited_with
    assert np.array_equal(mask, [1, 1]) and np.array_equal(P0, fp)
    s.close()
    # init_params["P"] that agrees is kept whole (its other columns are the caller's)
    full = np.concatenate([fp, _sig(12, 1, seed=9)], axis=1)
    s = _sampler(tmp_path, 3, fp, init_params={"P": full})
    P0, mask = _StubEngine.made[-1].inited_with
    assert np.array_equal(P0, full) and np.array_equal(mask, [1, 1, 0])
    s.close()


@pytest.mark.parametrize("what,match", [
    ("rows", "fixed_P has 11 rows, but data has 12 rows"),
    ("too_many", "fixed_P has 3 columns, but the rank"),
    ("too_many_range", "fixed_P has 3 columns, but the rank"),
    ("nan", "NaN"), ("negative", "finite and non-negative"), ("inf", "finite and non-negative"),
    ("zero_column", "column 2 sums to 0"), ("contradicts", "contradicts fixed_P"), ("contradicts_shape", "contradicts fixed_P"),
])
def test_fixed_P_refusals(tmp_path, what, match):
    fp, rank, kw = _sig(12, 2), 4, {}
    if what == "rows":
        fp = fp[:11]
    elif what == "too_many":
        fp, rank = _sig(12, 3), 2
    elif what == "too_many_range":
        fp, rank = _sig(12, 3), range(0, 3)
    elif what == "nan":
        fp[3, 1] = np.nan
    elif what == "negative":
        fp[3, 1] = -0.1
    elif what == "inf":
        fp[3, 0] = np.inf
    elif what == "zero_column":
        fp[:, 1] = 0.0
    elif what == "contradicts":
        P = np.concatenate([fp, _sig(12, 2, seed=4)], axis=1)
        P[0, 1] += 1e-9
        kw = dict(init_params={"P": P})
    elif what == "contradicts_shape":
        kw = dict(init_params={"P": fp})
    with pytest.raises(ValueError, match=match) as ei:
        _sampler(tmp_path, rank, fp, **kw)
    assert str(ei.value).startswith("ERROR: ")
    assert "ERROR: " in open(tmp_path / "out" / "log.txt").read()


def test_engine_without_set_fixed_is_refused(tmp_path):
    with pytest.raises(ValueError, match="set_fixed"):
        _sampler(tmp_path, 4, _sig(12, 2), factory=_NoFixEngine)
    s = _sampler(tmp_path, 4, None, factory=_NoFixEngine)      # ... and is fine without fixed_P
    s.close()


def test_bic_sweep_drops_the_ranks_below_F(tmp_path, capsys):
    from bayesnmf_amd import sampler as S
    from bayesnmf_amd.setup import synth_counts
    M, _, _ = synth_counts(12, 9, 2, 3, mean_total=200)
    seen = []

    class Fake:
        def __init__(self, data, rank, **kw):
            seen.append(int(rank))
            self.specs = dict(output_dir=kw["output_dir"])
            import pandas as pd
            self.state = dict(MAP_metrics=pd.DataFrame([dict(BIC=float(rank))]))
            self.time = dict(total=0.0)

        def run_gibbs_sampler(self):
            return self

    real, S.bayesNMF_sampler = S.bayesNMF_sampler, Fake
    try:
        out = S.bayesNMF(M, range(1, 6), likelihood="poisson", prior="gamma", rank_method="BIC", fixed_P=_sig(12, 3), devices=[0],
                         engine_factory=_StubEngine, output_dir=str(tmp_path / "bic"))
    finally:
        S.bayesNMF_sampler = real
    assert sorted(seen) == [3, 4, 5] and out["best_rank"] == 3
    assert "dropping ranks [1, 2]" in capsys.readouterr().out
