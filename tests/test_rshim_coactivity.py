"""The `.Call` routines of the co-activity of signatures (C_bnmf_coactivity / C_bnmf_coactivity_at in r/bnmf_shim.c), compiled against the
stand-in R runtime of tests/r_stub/ and run: warning-free and registered with their parameter count (CPU); their result is the ctypes
binding's, bit for bit (GPU)."""
import os
import re

import numpy as np
import pytest

from rshim import RShim, RError, ROOT, syntax_check


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
    for name in ("C_bnmf_coactivity", "C_bnmf_coactivity_at"):
        m = re.search(r"^SEXP %s\(([^)]*)\)\s*\{" % name, src, re.M)
        assert m and len([p for p in m.group(1).split(",") if p.strip()]) == 9, name
        assert R.routines[name] == 9
    rsrc = open(os.path.join(ROOT, "r", "bayesNMF_hip.R")).read()
    assert '.Call("C_bnmf_coactivity"' in rsrc and "get_coactivity = function(include" in rsrc


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(_bits(x)[~np.isnan(x)], _bits(y)[~np.isnan(y)])


@pytest.mark.gpu
def test_shim_result_is_the_ctypes_result(R):
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import IDS
    from bayesnmf_amd.setup import synth_counts, default_hyperprior_params, apply_hyperprior_params
    v0 = R.L.rstub_violations()
    K, G, N, W = 70, 9, 3, 8
    NP = N * (N - 1) // 2
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
    inc = np.array([1, 1, 1, 1, 1, 0, 1, 1, 1], dtype=np.int32)
    dims = [K, G, N]

    def same(got, want, series):
        for k in ("n_used", "n_included", "n_left_out", "n_pairs", "n_blocks", "max_cosine_at"):
            assert got[k][0] == want[k], k
        S = want["n_used"]
        for k in ("max_cosine", "min_load", "credible_interval"):
            assert _same_bits(got[k], np.array([want[k]])), k
        assert [int(v) for v in got["n_credible"]] == want["n_credible"]
        assert got["pair"].shape == (NP, 28)
        for q in range(4):
            for i in range(7):
                assert _same_bits(got["pair"][:, 7 * q + i], want["pair"][q, i]), (q, i)
        if series:
            assert got["series"].shape == (NP, 4 * S)
            for q in range(4):
                for s in range(S):
                    assert _same_bits(got["series"][:, S * q + s], want["series"][q, s])
        else:
            assert got["series"] is None

    want = e.coactivity(7, include=inc, used=used, end_iter=12, min_load=2.0, credible_interval=0.9, series=True)
    got = R.take(R.call("C_bnmf_coactivity", ptr, R.integer([12]), R.integer([7]), R.logical(used), R.logical(inc), R.real([2.0]), R.real([0.9]),
                        R.logical([True]), R.integer(dims)))
    assert want["n_used"] == 5 and want["n_included"] == 8 and want["n_left_out"] == 1 and want["n_pairs"] == NP
    same(got, want, True)
    # used = NULL, include = NULL, no series
    lean = R.take(R.call("C_bnmf_coactivity", ptr, R.integer([13]), R.integer([5]), R.nil(), R.nil(), R.real([1.0]), R.real([0.95]), R.logical([False]),
                         R.integer(dims)))
    same(lean, e.coactivity(5), False)
    now = R.take(R.call("C_bnmf_coactivity", ptr, R.nil(), R.integer([5]), R.nil(), R.nil(), R.real([1.0]), R.real([0.95]), R.logical([False]), R.integer(dims)))
    at = R.take(R.call("C_bnmf_coactivity_at", ptr, R.integer([13]), R.integer([5]), R.nil(), R.nil(), R.real([1.0]), R.real([0.95]), R.logical([False]),
                       R.integer(dims)))
    assert _same_bits(now["pair"], at["pair"])
    # refusals arrive as R errors with the library's message, the PROTECT stack empty
    with pytest.raises(RError, match="used has 3 entries"):
        R.call("C_bnmf_coactivity", ptr, R.integer([12]), R.integer([7]), R.logical([1, 1, 1]), R.nil(), R.real([1.0]), R.real([0.95]), R.logical([False]), R.integer(dims))
    with pytest.raises(RError, match="include has 2 flags for 9 tumours"):
        R.call("C_bnmf_coactivity", ptr, R.integer([12]), R.integer([7]), R.nil(), R.logical([1, 1]), R.real([1.0]), R.real([0.95]), R.logical([False]), R.integer(dims))
    with pytest.raises(RError, match="are kept"):
        R.call("C_bnmf_coactivity", ptr, R.integer([14]), R.integer([7]), R.nil(), R.nil(), R.real([1.0]), R.real([0.95]), R.logical([False]), R.integer(dims))
    with pytest.raises(RError, match="2 included tumours"):
        R.call("C_bnmf_coactivity", ptr, R.integer([12]), R.integer([3]), R.nil(), R.logical([1, 1, 0, 0, 0, 0, 0, 0, 0]), R.real([1.0]), R.real([0.95]),
               R.logical([False]), R.integer(dims))
    with pytest.raises(RError, match="min_load"):
        R.call("C_bnmf_coactivity", ptr, R.integer([12]), R.integer([3]), R.nil(), R.nil(), R.real([-1.0]), R.real([0.95]), R.logical([False]), R.integer(dims))
    with pytest.raises(RError, match="credible_interval"):
        R.call("C_bnmf_coactivity", ptr, R.integer([12]), R.integer([3]), R.nil(), R.nil(), R.real([1.0]), R.real([1.0]), R.logical([False]), R.integer(dims))
    assert R.L.rstub_protect_depth() == 0
    R.call("C_bnmf_destroy", ptr)
    R.release(ptr)
    e.close()
    assert R.L.rstub_violations() == v0
