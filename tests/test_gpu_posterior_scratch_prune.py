"""bnmf_prune among the other posterior calls on one handle: they share the handle's one scratch buffer (csrc/posterior.h), so a call
must leave nothing in it that a later call reads and must not depend on what an earlier one left.  The calls run in changing order and
every result is compared with the first of its kind, bit for bit (tests/test_gpu_posterior_scratch_tradeoff.py's recipe)."""
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


def test_prune_among_its_neighbours_in_changing_order(monkeypatch):
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    K, G, N = 8, 200, 5
    M, _, _ = synth_counts(K, G, 3, 21, mean_total=1500)
    e = Engine(M, N, prior="gamma", seed=4, window=16)
    apply_hyperprior_params(e, "gamma", M, N)
    e.init(); e.run(13)
    groups = (np.arange(G) % 3).astype(np.int32)
    q = np.array([0, 64, 199], dtype=np.int32)
    sets = np.array([0, 1, 1, -1, 0], dtype=np.int32)
    inc = (np.arange(G) % 4 != 1).astype(np.int32)

    def other(name, value):
        monkeypatch.setenv(name, value)                                              # a smaller scratch, or the other form of the kernel
        try:
            return e.prune(12, n_steps=5, exposures=True)
        finally:
            monkeypatch.delenv(name)

    calls = {
        "prune": lambda: e.prune(12, n_steps=5, exposures=True),
        "prune_batched": lambda: other("BNMF_PRN_BATCH", "5"),
        "prune_lds": lambda: other("BNMF_PRN_FORM", "1"),
        "prune_short": lambda: e.prune(6, include=inc, end_iter=11, n_steps=3, max_loss=0.05),
        "tradeoff": lambda: e.tradeoff(12, sets=sets, query=q),
        "reconstruction": lambda: e.reconstruction(12),
        "similarity": lambda: e.similarity(12, query=q, top_k=4),
        "contrast": lambda: e.contrast(12, groups, series=True),
        "waic": lambda: e.waic(12, pointwise=True),
        "map": lambda: e.map(12),
    }
    first = {k: _flat(f()) for k, f in calls.items()}
    assert np.array_equal(first["prune"], first["prune_batched"]) and np.array_equal(first["prune"], first["prune_lds"])
    for order in (["map", "prune", "reconstruction", "prune_batched", "contrast", "prune", "waic", "prune_short", "similarity", "prune_lds", "tradeoff", "prune"],
                  ["prune_short", "similarity", "prune", "map", "prune_batched", "tradeoff", "reconstruction", "prune_lds", "waic", "contrast"]):
        for k in order:
            assert np.array_equal(_flat(calls[k]()), first[k]), (k, order)
    e.close()
