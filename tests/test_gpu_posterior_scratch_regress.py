"""bnmf_regress among its neighbours on one handle's shared scratch buffer (csrc/posterior.h), in changing order: every call carves the
buffer anew, so each gives the same bits whatever ran before it and whether it grows the buffer or carves a smaller piece of a grown one.
A self-consistency test beside tests/test_gpu_posterior_scratch.py: the bits themselves are pinned against tests/*_ref.py."""
import numpy as np
import pytest

from test_gpu_posterior_scratch import K, G, N, W, _engine, _same

pytestmark = pytest.mark.gpu
GROUPS = np.array([0, 1, -1, 1, 0], dtype=np.int32)
DESIGN = np.asfortranarray(np.array([[1.0, 61.0], [1.0, 47.0], [1.0, 70.0], [1.0, 55.0], [1.0, 66.0]]))
INCLUDE = np.array([1, 1, 1, 0, 1], dtype=np.int32)


def _calls(e, ref):
    return {
        "regress": lambda n: e.regress(n, DESIGN, series=True),
        "map": lambda n: e.map(n),
        "contrast": lambda n: e.contrast(n, GROUPS, series=True),
        "regress_lean": lambda n: e.regress(n, DESIGN, include=INCLUDE, credible_interval=0.0),
        "attribution": lambda n: e.attribution(n, prob=True),
        "mixing": lambda n: e.mixing(n),
        "decompose": lambda n: e.decompose(n, ref, weights=True),
        "relabel": lambda n: e.relabel(n, aligned=True),
        "waic": lambda n: e.waic(n, pointwise=True),
    }


def _flat(r):
    return {k: (np.asarray(v) if isinstance(v, list) else v) for k, v in r.items()}


@pytest.mark.parametrize("likelihood", ["poisson", "normal"])
def test_regress_and_its_neighbours_give_the_same_bits_in_any_order(likelihood):
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
    r, lean = first["regress", W], first["regress_lean", W]
    assert r["n_used"] == W and r["Q"] == 2 and r["n_included"] == G and r["n_blocks"] == 1 and r["coef_series"].shape == (3, W, N, 2) and r["r2_series"].shape == (3, W, N)
    assert lean["n_included"] == 4 and lean["n_left_out"] == 1 and np.isnan(lean["coef"][:, 2:4]).all() and not np.isnan(r["coef"][:2]).any()
    e.close()
