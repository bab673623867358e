"""bnmf_summary among the other posterior calls on one handle: they share the handle's one scratch buffer (csrc/posterior.h), so a call
must leave nothing in it that a later call reads and must not depend on what an earlier one left.  The calls run in changing order and
every result is compared with the first of its kind, bit for bit (tests/test_gpu_posterior_scratch_prune.py's recipe)."""
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
        if k in ("pairs", "names") or v is None:
            continue
        try:
            a = np.asarray(v, dtype=np.float64).ravel()
        except (TypeError, ValueError):
            continue
        parts.append(_bits(np.where(np.isnan(a), -9.0, a)))
    return np.concatenate(parts)


def test_summary_among_its_neighbours_in_changing_order(monkeypatch):
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

    def other(env):
        for name, value in env.items():
            monkeypatch.setenv(name, value)                                          # a smaller scratch, or the general form of the kernel
        try:
            return e.summary(12, series=True)
        finally:
            for name in env:
                monkeypatch.delenv(name)

    calls = {
        "summary": lambda: e.summary(12, series=True),
        "summary_batched": lambda: other(dict(BNMF_SUM_BATCH="5")),
        "summary_chunks": lambda: other(dict(BNMF_SUM_CHUNK="64", BNMF_SUM_BATCH="7")),
        "summary_short": lambda: e.summary(6, probs=(0.0, 0.5, 1.0), include=inc, end_iter=11, min_load=2.0, series=True),
        "prune": lambda: e.prune(12, n_steps=5, exposures=True),
        "tradeoff": lambda: e.tradeoff(12, sets=sets, query=q),
        "coactivity": lambda: e.coactivity(12, series=True),
        "contrast": lambda: e.contrast(12, groups, series=True),
        "waic": lambda: e.waic(12, pointwise=True),
        "map": lambda: e.map(12),
    }
    first = {k: _flat(f()) for k, f in calls.items()}
    assert np.array_equal(first["summary"], first["summary_batched"]) and np.array_equal(first["summary"], first["summary_chunks"])
    for order in (["map", "summary", "coactivity", "summary_batched", "contrast", "summary", "waic", "summary_short", "prune", "summary_chunks", "tradeoff", "summary"],
                  ["summary_short", "prune", "summary", "map", "summary_batched", "tradeoff", "coactivity", "summary_chunks", "waic", "contrast"]):
        for k in order:
            assert np.array_equal(_flat(calls[k]()), first[k]), (k, order)
    e.close()
