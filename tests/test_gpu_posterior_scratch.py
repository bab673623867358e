"""The posterior calls share one scratch buffer per handle (csrc/posterior.h): every call carves the buffer anew, so a call must give the
same bits whatever ran before it on the handle, and whether it grows the buffer or carves a smaller piece of a grown one.  A
self-consistency test: the bits themselves are pinned by the tests against tests/*_ref.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
K, G, N, W = 6, 5, 3, 12


def _engine(likelihood):
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    if likelihood == "normal":                      # the sigmasq ring, k_waic<true>, k_ppc<true>
        rng = np.random.default_rng(11)
        M = np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, 2)) @ rng.gamma(2.0, 1.0, size=(2, G)) + rng.normal(0.0, 0.5, size=(K, G)))
        prior = "exponential"
    else:
        M, _, _ = synth_counts(K, G, 2, 21, mean_total=300)
        prior = "gamma"
    e = Engine(M, N, likelihood=likelihood, prior=prior, seed=4, window=W)
    apply_hyperprior_params(e, prior, M, N)
    e.init()
    e.run(12)
    return e


def _calls(e, ref):
    """name -> call(last_n), in the order of the first pass"""
    return {
        "map": lambda n: e.map(n),
        "relabel": lambda n: e.relabel(n, aligned=True),
        "waic": lambda n: e.waic(n, pointwise=True),
        "attribution": lambda n: e.attribution(n, prob=True),
        "ppc": lambda n: e.ppc(n, pointwise=True),
        "mixing": lambda n: e.mixing(n),
        "assign": lambda n: e.assign(n, ref),
        "label_switching": lambda n: e.label_switching(np.arange(e.iter - n + 1, e.iter + 1), ref),
    }


def _same(a, b, where):
    assert a.keys() == b.keys(), where
    for k, x in a.items():
        y = b[k]
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), f"{where}: {k}"
        elif isinstance(x, float):
            assert x == y or (x != x and y != y), f"{where}: {k} = {x!r}, first {y!r}"
        else:
            assert x == y, f"{where}: {k} = {x!r}, first {y!r}"


@pytest.mark.parametrize("likelihood", ["poisson", "normal"])
def test_a_call_gives_the_same_bits_whatever_carved_the_scratch_before(likelihood, monkeypatch):
    monkeypatch.setenv("BNMF_ATTR_BATCH", "2")      # several batches of attribution reuse their part of the scratch
    e = _engine(likelihood)
    ref = np.asfortranarray(np.random.default_rng(5).gamma(1.0, 1.0, size=(K, 4)))
    calls = _calls(e, ref)
    names = list(calls)
    first = {(name, W): calls[name](W) for name in names}                       # first pass: every call grows or re-carves the buffer
    for name in reversed(names):                                                # second pass: the reverse order ...
        _same(calls[name](W), first[name, W], f"{name}, second pass")
    for name in names:                                                          # ... then a smaller carve of the grown buffer
        first[name, 4] = calls[name](4)
    for name in names:                                                          # third pass
        _same(calls[name](W), first[name, W], f"{name}, third pass")
    for name in reversed(names):
        _same(calls[name](4), first[name, 4], f"{name}, last_n = 4 again")
    for name in ("map", "relabel", "waic", "attribution", "ppc", "mixing"):
        assert first[name, W]["n_used"] > 0 and first[name, 4]["n_used"] > 0, name
    assert first["relabel", W]["aligned_P"].shape[1:] == (K, N) and first["attribution", W]["prob"].shape == (K, N, G)
    e.close()
