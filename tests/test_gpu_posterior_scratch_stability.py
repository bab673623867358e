"""bnmf_stability among the other posterior calls on one handle: they share the handle's one scratch buffer (csrc/posterior.h), so a call
must leave nothing in it that a later call reads and must not depend on what an earlier one left.  The calls run in changing order and
every result is compared with the first of its kind, bit for bit (tests/test_gpu_posterior_scratch_coactivity.py's recipe)."""
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


def test_stability_among_its_neighbours_in_changing_order():
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    K, G, N = 8, 1100, 5
    M, _, _ = synth_counts(K, G, 3, 21, mean_total=1500)
    e = Engine(M, N, prior="gamma", seed=4, window=16)
    apply_hyperprior_params(e, "gamma", M, N)
    e.init(); e.run(13)
    rng = np.random.default_rng(2)
    groups = (np.arange(G) % 3).astype(np.int32)
    ex = np.asfortranarray(rng.gamma(0.5, 1.0, size=(K, 1100)))
    el = (np.arange(1100) % 2).astype(np.int32)
    calls = {
        "stability": lambda: e.stability(12),
        "stability_extras": lambda: e.stability(10, extra_P=ex, extra_label=el),        # a larger scratch: two blocks in cluster 0 and 1
        "coactivity": lambda: e.coactivity(12, series=True),
        "contrast": lambda: e.contrast(12, groups, series=True),
        "attribution": lambda: e.attribution(12),
        "relabel": lambda: e.relabel(12),
        "map": lambda: e.map(12),
    }
    first = {k: _flat(f()) for k, f in calls.items()}
    for order in (["map", "stability", "coactivity", "stability_extras", "contrast", "stability", "relabel", "stability_extras", "attribution", "stability"],
                  ["stability_extras", "attribution", "stability", "map", "stability_extras", "coactivity", "relabel", "contrast"]):
        for k in order:
            assert np.array_equal(_flat(calls[k]()), first[k]), (k, order)
    e.close()
