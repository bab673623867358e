"""bnmf_similarity among the other posterior calls on one handle: they share the handle's one scratch buffer (csrc/posterior.h), so a call
must leave nothing in it that a later call reads and must not depend on what an earlier one left.  The calls run in changing order and
every result is compared with the first of its kind, bit for bit (tests/test_gpu_posterior_scratch_reconstruction.py's recipe)."""
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


def test_similarity_among_its_neighbours_in_changing_order(monkeypatch):
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    K, G, N = 8, 200, 5                                                           # four tiles of columns, the last one ragged
    M, _, _ = synth_counts(K, G, 3, 21, mean_total=1500)
    e = Engine(M, N, prior="gamma", seed=4, window=16)
    apply_hyperprior_params(e, "gamma", M, N)
    e.init(); e.run(13)
    groups = (np.arange(G) % 3).astype(np.int32)
    q = np.array([0, 64, 199], dtype=np.int32)

    def banded():
        monkeypatch.setenv("BNMF_SIM_BAND", "70")                                   # a smaller scratch: 3 bands of rows
        try:
            return e.similarity(12, query=q, top_k=4)
        finally:
            monkeypatch.delenv("BNMF_SIM_BAND")

    calls = {
        "similarity": lambda: e.similarity(12, query=q, top_k=4),
        "similarity_banded": banded,
        "similarity_short": lambda: e.similarity(6, end_iter=11, query=q, top_k=0, tumour=False, min_cosine=0.95),
        "stability": lambda: e.stability(12),
        "reconstruction": lambda: e.reconstruction(12),
        "contrast": lambda: e.contrast(12, groups, series=True),
        "attribution": lambda: e.attribution(12),
        "waic": lambda: e.waic(12, pointwise=True),
        "map": lambda: e.map(12),
    }
    first = {k: _flat(f()) for k, f in calls.items()}
    assert np.array_equal(first["similarity"], first["similarity_banded"])
    for order in (["map", "similarity", "stability", "similarity_banded", "contrast", "similarity", "waic", "similarity_short", "attribution", "reconstruction",
                   "similarity"],
                  ["similarity_short", "attribution", "similarity", "map", "reconstruction", "similarity_banded", "stability", "waic", "contrast"]):
        for k in order:
            assert np.array_equal(_flat(calls[k]()), first[k]), (k, order)
    e.close()
