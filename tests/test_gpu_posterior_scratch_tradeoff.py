"""bnmf_tradeoff among the other posterior calls on one handle: they share the handle's one scratch buffer (csrc/posterior.h), so a call
must leave nothing in it that a later call reads and must not depend on what an earlier one left.  The calls run in changing order and
every result is compared with the first of its kind, bit for bit (tests/test_gpu_posterior_scratch_similarity.py's recipe)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _flat(r):
    """every array and number of a result dict as one vector of bit patterns, NaN as one pattern"""
    parts = []
    for k in sorted(r):
        v = r[k]
        if k == "pairs" or v is None:
            continue
        try:
            a = np.asarray(v, dtype=np.float64).ravel()
        except (TypeError, ValueError):
            continue
        parts.append(_bits(np.where(np.isnan(a), -9.0, a)))
    return np.concatenate(parts)


def test_tradeoff_among_its_neighbours_in_changing_order(monkeypatch):
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    K, G, N = 8, 200, 5
    M, _, _ = synth_counts(K, G, 3, 21, mean_total=1500)
    e = Engine(M, N, prior="gamma", seed=4, window=16)
    apply_hyperprior_params(e, "gamma", M, N)
    e.init(); e.run(13)
    groups = (np.arange(G) % 3).astype(np.int32)
    q = np.array([0, 64, 199], dtype=np.int32)
    E = np.asarray(e.get("E"), dtype=np.float64)
    c0 = np.asfortranarray((E / E.sum(axis=0))[:, [3, 90, 170]])

    def banded():
        monkeypatch.setenv("BNMF_TRD_BAND", "70")                                    # a smaller scratch: 3 bands of members
        try:
            return e.tradeoff(12, sets=sets, query=q)
        finally:
            monkeypatch.delenv("BNMF_TRD_BAND")

    sets = np.array([0, 1, 1, -1, 0], dtype=np.int32)
    calls = {
        "tradeoff": lambda: e.tradeoff(12, sets=sets, query=q),
        "tradeoff_banded": banded,
        "tradeoff_short": lambda: e.tradeoff(6, end_iter=11, min_corr=0.3),
        "subtypes": lambda: e.subtypes(12, c0, query=q, labels=True),
        "similarity": lambda: e.similarity(12, query=q, top_k=4),
        "stability": lambda: e.stability(12),
        "contrast": lambda: e.contrast(12, groups, series=True),
        "waic": lambda: e.waic(12, pointwise=True),
        "map": lambda: e.map(12),
    }
    first = {k: _flat(f()) for k, f in calls.items()}
    assert np.array_equal(first["tradeoff"], first["tradeoff_banded"])
    for order in (["map", "tradeoff", "stability", "tradeoff_banded", "contrast", "tradeoff", "waic", "tradeoff_short", "similarity", "subtypes", "tradeoff"],
                  ["tradeoff_short", "similarity", "tradeoff", "map", "tradeoff_banded", "subtypes", "stability", "waic", "contrast"]):
        for k in order:
            assert np.array_equal(_flat(calls[k]()), first[k]), (k, order)
    e.close()
