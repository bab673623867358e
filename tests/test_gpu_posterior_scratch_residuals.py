"""bnmf_residuals among the other posterior calls on one handle: they share the handle's one scratch buffer (csrc/posterior.h), so a call
must leave nothing in it that a later call reads and must not depend on what an earlier one left.  The calls run in changing order and
every result is compared with the first of its kind, bit for bit (tests/test_gpu_posterior_scratch_subtypes.py's recipe)."""
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


def test_residuals_among_its_neighbours_in_changing_order(monkeypatch):
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
        monkeypatch.setenv("BNMF_RES_BATCH", "5")                                    # a smaller scratch: 3 batches of samples
        try:
            return e.residuals(12, n_steps=30)
        finally:
            monkeypatch.delenv("BNMF_RES_BATCH")

    calls = {
        "residuals": lambda: e.residuals(12, n_steps=30),
        "residuals_banded": banded,
        "residuals_short": lambda: e.residuals(6, end_iter=11, n_steps=3, include=(np.arange(G) % 2).astype(np.int32)),
        "subtypes": lambda: e.subtypes(12, c0, query=q, labels=True),
        "similarity": lambda: e.similarity(12, query=q, top_k=4),
        "contrast": lambda: e.contrast(12, groups, series=True),
        "waic": lambda: e.waic(12, pointwise=True),
        "map": lambda: e.map(12),
    }
    first = {k: _flat(f()) for k, f in calls.items()}
    assert np.array_equal(first["residuals"], first["residuals_banded"])
    for order in (["map", "residuals", "subtypes", "residuals_banded", "contrast", "residuals", "waic", "residuals_short", "similarity", "residuals"],
                  ["residuals_short", "similarity", "residuals", "map", "residuals_banded", "subtypes", "waic", "contrast"]):
        for k in order:
            assert np.array_equal(_flat(calls[k]()), first[k]), (k, order)
    e.close()
