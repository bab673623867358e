"""bnmf_contrast among its neighbours on one handle's shared scratch buffer (csrc/posterior.h), in changing order: every call carves the
buffer anew, so each gives the same bits whatever ran before it and whether it grows the buffer or carves a smaller piece of a grown one.
A self-consistency test beside tests/test_gpu_posterior_scratch.py: the bits themselves are pinned against tests/*_ref.py."""
import numpy as np
import pytest

from test_gpu_posterior_scratch import K, G, N, W, _engine, _same

pytestmark = pytest.mark.gpu
GROUPS = np.array([0, 1, -1, 1, 0], dtype=np.int32)


def _calls(e, ref):
    return {
        "contrast": lambda n: e.contrast(n, GROUPS, series=True),
        "map": lambda n: e.map(n),
        "attribution": lambda n: e.attribution(n, prob=True),
        "contrast_lean": lambda n: e.contrast(n, GROUPS, credible_interval=0.0),
        "mixing": lambda n: e.mixing(n),
        "decompose": lambda n: e.decompose(n, ref, weights=True),
        "relabel": lambda n: e.relabel(n, aligned=True),
        "waic": lambda n: e.waic(n, pointwise=True),
    }


def _flat(r):
    return {k: (np.asarray(v) if isinstance(v, list) else v) for k, v in r.items()}


@pytest.mark.parametrize("likelihood", ["poisson", "normal"])
def test_contrast_and_its_neighbours_give_the_same_bits_in_any_order(likelihood):
    e = _engine(likelihood)
    ref = np.asfortranarray(np.random.default_rng(5).gamma(1.0, 1.0, size=(K, 4)))
    calls = _calls(e, ref)
    names = list(calls)
    first = {(name, W): _flat(calls[name](W)) for name in names}                # first pass: every call grows or re-carves the buffer
    for name in reversed(names):                                                # the reverse order ...
        _same(_flat(calls[name](W)), first[name, W], f"{name}, second pass")
    for name in names:                                                          # ... a smaller carve of the grown buffer ...
        first[name, 4] = _flat(calls[name](4))
    for name in names[1::2] + names[::2]:                                       # ... and an interleaved order
        _same(_flat(calls[name](W)), first[name, W], f"{name}, third pass")
    for name in reversed(names):
        _same(_flat(calls[name](4)), first[name, 4], f"{name}, last_n = 4 again")
    c = first["contrast", W]
    assert c["n_used"] == W and c["sizes"].tolist() == [2, 2] and c["n_left_out"] == 1 and c["series"].shape == (3, W, N, 2) and c["pair"].shape == (3, 6, N, 1)
    assert np.isnan(first["contrast_lean", W]["group"][:, 2:]).all() and not np.isnan(c["group"]).any()
    e.close()
