"""CPU tests of the mirror's posterior inference on any recorded range (get_MAP(end_iter, n_samples), get_MAP_ R/utils.R:194-230)
and of assign_signatures_ensemble(idxs) range checks, with the CPU oracle standing in for the engine (host path of the mirror)."""
from collections import Counter

import numpy as np
import pytest


class _OracleHistory:
    """Test adapter: the CPU oracle behind the Engine method names; its window keeps the whole history."""

    def __init__(self, M, N, **kw):
        import oracle as O
        self._o = O.Oracle(M, N, nthreads=4, **kw)
        self._hist = {}

    def set(self, name, v):
        self._o.set(name, v)

    def get(self, name):
        return self._o.get(name)

    def _rec(self):
        self._hist[self._o.iter] = {n: self._o.get(n) for n in ("P", "E", "A", "R", "Alpha_p", "Beta_p", "Alpha_e", "Beta_e")}

    def init(self):
        r = self._o.init(); self._rec(); return r

    def run(self, n, converged=False):
        rows = []
        for _ in range(n):
            rows.append(self._o.run(1, converged)[0]); self._rec()
        return np.array(rows)

    def window(self, name, last_n):
        it = self._o.iter
        if last_n > it:
            raise ValueError("more samples than recorded")
        return [self._hist[i][name] for i in range(it - last_n + 1, it + 1)]

    def close(self):
        self._o.close()


def _run(tmp_path, save_all_samples, name="o"):
    from bayesnmf_amd.sampler import bayesNMF
    from bayesnmf_amd.convergence import new_convergence_control
    from bayesnmf_amd.setup import synth_counts
    M, _, _ = synth_counts(16, 20, 2, 3, mean_total=1200)
    cc = new_convergence_control(MAP_over=30, MAP_every=15, miniters=75, maxiters=90)
    return bayesNMF(M, range(1, 4), likelihood="poisson", prior="gamma", convergence_control=cc, output_dir=str(tmp_path / name),
                    periodic_save=False, save_all_samples=save_all_samples, engine_factory=_OracleHistory, seed=5)


def _np_map(chain, first, last, ci):
    h = chain._hist
    its = list(range(first, last + 1))
    keys = ["".join(str(int(v)) for v in np.ravel(h[t]["A"])) for t in its]
    mode = sorted(Counter(keys).items(), key=lambda kv: (-kv[1], kv[0]))[0][0]
    used = [t for t, k in zip(its, keys) if k == mode]
    keep = [n for n, c in enumerate(mode) if c == "1"]
    Pn = np.stack([h[t]["P"] / h[t]["P"].sum(0)[None, :] for t in used], axis=2)[:, keep]
    En = np.stack([h[t]["E"] * h[t]["P"].sum(0)[:, None] for t in used], axis=2)[keep]
    return dict(idx=used, keep=keep, P=Pn.mean(2), E=En.mean(2), P_lower=np.quantile(Pn, 0.5 - ci / 2, axis=2),
                E_upper=np.quantile(En, 0.5 + ci / 2, axis=2))


def test_get_MAP_over_an_earlier_range_matches_numpy(tmp_path):
    s = _run(tmp_path, True)
    assert s.state["iter"] == 90
    MAP = s.get_MAP(end_iter=50, n_samples=25, final=True, credible_interval=0.9)
    want = _np_map(s._chain, 26, 50, 0.9)
    assert list(MAP["idx"]) == want["idx"] and list(MAP["keep_sigs"]) == want["keep"]
    assert np.allclose(MAP["P"], want["P"], rtol=1e-12, atol=0) and np.allclose(MAP["E"], want["E"], rtol=1e-12, atol=0)
    assert np.allclose(s.credible_intervals["P"]["lower"], want["P_lower"], rtol=1e-12, atol=0)
    assert np.allclose(s.credible_intervals["E"]["upper"], want["E_upper"], rtol=1e-12, atol=0)
    # n_samples defaults to MAP_over
    MAP = s.get_MAP(end_iter=70, final=True, credible_interval=0.9)
    assert list(MAP["idx"]) == _np_map(s._chain, 41, 70, 0.9)["idx"]
    # a range that was never recorded
    with pytest.raises(ValueError, match="not all recorded"):
        s.get_MAP(end_iter=95, n_samples=10)
    with pytest.raises(ValueError, match="not all recorded"):
        s.get_MAP(end_iter=20, n_samples=30)
    s.close()


def test_end_iter_needs_save_all_samples(tmp_path):
    s = _run(tmp_path, False)
    with pytest.raises(ValueError, match=r"end_iter cannot be provided unless self\$specs\$save_all_samples is TRUE"):
        s.get_MAP(end_iter=50, n_samples=10)
    s.get_MAP(end_iter=s.state["iter"], final=True)                       # end_iter == iter is always allowed
    s.close()


def test_end_iter_equal_to_iter_ignores_n_samples(tmp_path):
    """the reference's quirk: with end_iter == iter the window is state$MAP_idx, whatever n_samples says"""
    s = _run(tmp_path, True)
    a = {k: np.copy(v) for k, v in s.get_MAP(final=True).items() if k in ("P", "E", "idx")}
    b = s.get_MAP(end_iter=s.state["iter"], n_samples=5, final=True)
    assert np.array_equal(a["idx"], b["idx"]) and np.array_equal(a["P"], b["P"]) and np.array_equal(a["E"], b["E"])
    assert min(b["idx"]) >= s.state["iter"] - 30 + 1 and len(b["idx"]) > 5
    s.close()


def test_assign_refuses_indices_outside_the_kept_range(tmp_path):
    """Without save_all_samples only the last MAP_over samples are kept: an earlier index is an error, not a wrapped-round mask."""
    s = _run(tmp_path, False)
    s.get_MAP(final=True)
    ref = np.random.default_rng(0).dirichlet(np.ones(16), size=4).T
    for idxs in ([1], [s.state["iter"] - 30], [s.state["iter"] + 1], [s.state["iter"] - 40, s.state["iter"]]):
        with pytest.raises(ValueError, match=r"kept: 61\.\.90"):
            s.assign_signatures_ensemble(ref, idxs=idxs)
    s.close()
