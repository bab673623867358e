"""The `.Call` routines of the group contrasts (C_bnmf_contrast / C_bnmf_contrast_at in r/bnmf_shim.c), compiled against the stand-in R
runtime of tests/r_stub/ and run: warning-free and registered with their parameter count (CPU); their result is the ctypes binding's,
bit for bit (GPU)."""
import os
import re

import numpy as np
import pytest

from rshim import RShim, RError, ROOT, syntax_check

NA_INTEGER = -2 ** 31


@pytest.fixture(scope="module")
def R():
    if not os.path.exists(os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")):
        import __graft_entry__ as g
        g.build()
    return RShim()


def test_shim_compiles_without_warnings():
    p = syntax_check()
    assert p.returncode == 0 and p.stderr == "", p.stderr


def test_routines_are_registered_with_their_parameter_count(R):
    src = open(os.path.join(ROOT, "r", "bnmf_shim.c")).read()
    for name in ("C_bnmf_contrast", "C_bnmf_contrast_at"):
        m = re.search(r"^SEXP %s\(([^)]*)\)\s*\{" % name, src, re.M)
        assert m and len([p for p in m.group(1).split(",") if p.strip()]) == 9, name
        assert R.routines[name] == 9
    rsrc = open(os.path.join(ROOT, "r", "bayesNMF_hip.R")).read()
    assert '.Call("C_bnmf_contrast"' in rsrc and "get_contrast = function(groups" in rsrc


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.gpu
def test_shim_result_is_the_ctypes_result(R):
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import IDS
    from bayesnmf_amd.setup import synth_counts, default_hyperprior_params, apply_hyperprior_params
    v0 = R.L.rstub_violations()
    K, G, N, W = 70, 9, 3, 8
    M, _, _ = synth_counts(K, G, 3, 7, mean_total=1500)
    ptr = R.call("C_bnmf_create", R.int_matrix(M), R.integer([K, G, N]), R.integer([0, 2, 0, 0, 0, 0, W]), R.real(np.ones(1)), R.real([9.0]),
                 R.integer([0]), R.integer([0]))
    for k, v in default_hyperprior_params("gamma", M, N).items():
        R.call("C_bnmf_set_array", ptr, R.integer([IDS[k[0].upper() + k[1:]]]), R.real([float(v)]))
    e = Engine(M, N, prior="gamma", seed=9, window=W, temperature=np.ones(1))   # the shim passes a schedule of one 1.0
    apply_hyperprior_params(e, "gamma", M, N)
    R.take(R.call("C_bnmf_init", ptr)); e.init()
    R.take(R.call("C_bnmf_run", ptr, R.integer([12]), R.logical([False]))); e.run(12)
    used = np.array([1, 0, 1, 1, 0, 1, 1], dtype=np.int32)
    groups = np.array([0, 1, 2, 1, 0, -1, 2, 1, 0], dtype=np.int32)
    dims = [K, G, N]

    def same(got, want, series):
        for k in ("n_used", "n_groups", "n_pairs", "n_left_out"):
            assert got[k][0] == want[k], k
        assert got["n_credible"].tolist() == want["n_credible"] and got["min_load"][0] == want["min_load"] and got["credible_interval"][0] == want["credible_interval"]
        S, Cn, NP = want["n_used"], want["n_groups"], want["n_pairs"]
        assert got["sizes"].tolist() == want["sizes"].tolist() and got["group"].shape == (N * Cn, 12)
        for q in range(3):
            for i in range(4):
                assert np.array_equal(_bits(got["group"][:, 4 * q + i].reshape((N, Cn), order="F")), _bits(want["group"][q, i])), (q, i)
            for i in range(6 if NP else 0):
                x, y = got["pair"][:, 6 * q + i].reshape((N, NP), order="F"), want["pair"][q, i]
                assert np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(_bits(x)[~np.isnan(x)], _bits(y)[~np.isnan(y)]), (q, i)
        if NP == 0:
            assert got["pair"] is None
        if series:
            assert got["series"].shape == (N * Cn, 3 * S)
            for q in range(3):
                for s in range(S):
                    assert np.array_equal(_bits(got["series"][:, S * q + s].reshape((N, Cn), order="F")), _bits(want["series"][q, s]))
        else:
            assert got["series"] is None

    want = e.contrast(7, groups, used=used, end_iter=12, min_load=2.0, credible_interval=0.9, series=True)
    gna = groups.copy(); gna[5] = NA_INTEGER                                     # NA is -1: left out
    got = R.take(R.call("C_bnmf_contrast", ptr, R.integer([12]), R.integer([7]), R.logical(used), R.integer(gna), R.real([2.0]), R.real([0.9]),
                        R.logical([True]), R.integer(dims)))
    assert want["n_used"] == 5 and want["n_groups"] == 3 and want["n_left_out"] == 1
    same(got, want, True)
    # used = NULL, no series, one group
    one = np.zeros(G, dtype=np.int32)
    lean = R.take(R.call("C_bnmf_contrast", ptr, R.integer([13]), R.integer([5]), R.nil(), R.integer(one), R.real([1.0]), R.real([0.95]), R.logical([False]),
                         R.integer(dims)))
    same(lean, e.contrast(5, one), False)
    now = R.take(R.call("C_bnmf_contrast", ptr, R.nil(), R.integer([5]), R.nil(), R.integer(groups), R.real([1.0]), R.real([0.95]), R.logical([False]), R.integer(dims)))
    at = R.take(R.call("C_bnmf_contrast_at", ptr, R.integer([13]), R.integer([5]), R.nil(), R.integer(groups), R.real([1.0]), R.real([0.95]), R.logical([False]),
                       R.integer(dims)))
    assert np.array_equal(_bits(now["group"]), _bits(at["group"])) and np.array_equal(_bits(now["pair"]), _bits(at["pair"]))
    same(now, e.contrast(5, groups), False)
    # refusals arrive as R errors with the library's message, the PROTECT stack empty
    with pytest.raises(RError, match="used has 3 entries"):
        R.call("C_bnmf_contrast", ptr, R.integer([12]), R.integer([7]), R.logical([1, 1, 1]), R.integer(groups), R.real([1.0]), R.real([0.95]), R.logical([False]), R.integer(dims))
    with pytest.raises(RError, match="groups has 3 labels for 9 tumours"):
        R.call("C_bnmf_contrast", ptr, R.integer([12]), R.integer([7]), R.nil(), R.integer([0, 1, 0]), R.real([1.0]), R.real([0.95]), R.logical([False]), R.integer(dims))
    with pytest.raises(RError, match="are kept"):
        R.call("C_bnmf_contrast", ptr, R.integer([14]), R.integer([7]), R.nil(), R.integer(groups), R.real([1.0]), R.real([0.95]), R.logical([False]), R.integer(dims))
    bad = groups.copy(); bad[2] = 70
    with pytest.raises(RError, match=r"groups\[2\] = 70"):
        R.call("C_bnmf_contrast", ptr, R.integer([12]), R.integer([3]), R.nil(), R.integer(bad), R.real([1.0]), R.real([0.95]), R.logical([False]), R.integer(dims))
    with pytest.raises(RError, match="group 1 has no member"):
        R.call("C_bnmf_contrast", ptr, R.integer([12]), R.integer([3]), R.nil(), R.integer(np.where(groups == 1, -1, groups)), R.real([1.0]), R.real([0.95]),
               R.logical([False]), R.integer(dims))
    with pytest.raises(RError, match="credible_interval"):
        R.call("C_bnmf_contrast", ptr, R.integer([12]), R.integer([3]), R.nil(), R.integer(groups), R.real([1.0]), R.real([1.0]), R.logical([False]), R.integer(dims))
    assert R.L.rstub_protect_depth() == 0
    R.call("C_bnmf_destroy", ptr)
    R.release(ptr)
    e.close()
    assert R.L.rstub_violations() == v0
