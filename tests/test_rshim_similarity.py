"""The `.Call` routines of the similarity of tumours (C_bnmf_similarity / C_bnmf_similarity_at in r/bnmf_shim.c), compiled against the
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
    for name in ("C_bnmf_similarity", "C_bnmf_similarity_at"):
        m = re.search(r"^SEXP %s\(([^)]*)\)\s*\{" % name, src, re.M)
        assert m and len([p for p in m.group(1).split(",") if p.strip()]) == 9, name
        assert R.routines[name] == 9
    rsrc = open(os.path.join(ROOT, "r", "bayesNMF_hip.R")).read()
    assert '.Call("C_bnmf_similarity"' in rsrc and "get_similarity = function(include = NULL, query = NULL, top_k = 10, min_cosine = 0.9" in rsrc
    assert 'idx = "MAP_idx"' in rsrc[rsrc.index("get_similarity = function"):][:400]


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
    K, G, N, W = 12, 70, 3, 8
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
    inc = np.ones(G, dtype=np.int32)
    inc[[0, 64]] = 0
    dims = [K, G, N]

    def same(got, want, k, Q, tumour=True):
        for f in ("n_used", "n_included", "n_left_out", "top_k", "n_query"):
            assert got[f][0] == want[f], f
        for f in ("n_pairs", "n_similar_pairs", "n_isolated", "least_typical_at"):
            assert int(got[f][0]) == want[f], f
        for f in ("mean_similarity", "least_typical", "min_cosine"):
            assert _same_bits(got[f], np.array([want[f]])), f
        if k > 0:
            assert np.array_equal(np.asarray(got["neighbour_at"]).T.reshape(G, k), want["neighbour_at"])
            assert _same_bits(np.asarray(got["neighbour"]).T.reshape(3, G, k), want["neighbour"])
        else:
            assert got["neighbour_at"] is None and got["neighbour"] is None
        if Q > 0:
            assert _same_bits(np.asarray(got["dense"]).T.reshape(3, Q, G), want["dense"])
        else:
            assert got["dense"] is None
        if tumour:
            assert _same_bits(np.asarray(got["tumour"]).T, want["tumour"])
        else:
            assert got["tumour"] is None

    q = np.array([3, 69, 3], dtype=np.int32)
    want = e.similarity(7, include=inc, query=q, top_k=4, min_cosine=0.95, used=used, end_iter=12)
    got = R.take(R.call("C_bnmf_similarity", ptr, R.integer([12]), R.integer([7]), R.logical(used), R.logical(inc), R.integer(q), R.integer([4, 1]), R.real([0.95]),
                         R.integer(dims)))
    assert want["n_used"] == 5 and want["n_left_out"] == 2 and want["min_cosine"] == 0.95
    same(got, want, 4, 3)
    # used, include and query NULL, the current iteration
    lean = R.take(R.call("C_bnmf_similarity", ptr, R.integer([13]), R.integer([5]), R.nil(), R.nil(), R.nil(), R.integer([2, 1]), R.real([0.9]),
                         R.integer(dims)))
    same(lean, e.similarity(5, top_k=2), 2, 0)
    now = R.take(R.call("C_bnmf_similarity", ptr, R.nil(), R.integer([5]), R.nil(), R.nil(), R.nil(), R.integer([2, 1]), R.real([0.9]), R.integer(dims)))
    at = R.take(R.call("C_bnmf_similarity_at", ptr, R.integer([13]), R.integer([5]), R.nil(), R.nil(), R.nil(), R.integer([2, 1]), R.real([0.9]),
                       R.integer(dims)))
    assert _same_bits(now["tumour"], at["tumour"]) and _same_bits(now["neighbour"], at["neighbour"]) and _same_bits(now["tumour"], lean["tumour"])
    # the queries alone
    alone = R.take(R.call("C_bnmf_similarity", ptr, R.integer([12]), R.integer([7]), R.logical(used), R.logical(inc), R.integer(q), R.integer([0, 0]), R.real([0.95]),
                           R.integer(dims)))
    same(alone, e.similarity(7, include=inc, query=q, top_k=0, min_cosine=0.95, used=used, end_iter=12, tumour=False), 0, 3, tumour=False)
    assert int(alone["n_similar_pairs"][0]) == -1 and _same_bits(alone["dense"], got["dense"])
    # refusals arrive as R errors with the library's message, the PROTECT stack empty
    args = lambda **kw: [kw.get("end", R.integer([12])), R.integer([7]), kw.get("used", R.nil()), kw.get("include", R.nil()), kw.get("query", R.nil()),
                         R.integer([kw.get("k", 3), 1]), R.real([kw.get("mc", 0.9)]), R.integer(dims)]
    with pytest.raises(RError, match="used has 3 entries"):
        R.call("C_bnmf_similarity", ptr, *args(used=R.logical([1, 1, 1])))
    with pytest.raises(RError, match="include has 2 flags"):
        R.call("C_bnmf_similarity", ptr, *args(include=R.logical([1, 1])))
    with pytest.raises(RError, match="are kept"):
        R.call("C_bnmf_similarity", ptr, *args(end=R.integer([14])))
    with pytest.raises(RError, match="min_cosine"):
        R.call("C_bnmf_similarity", ptr, *args(mc=float("nan")))
    with pytest.raises(RError, match="top_k = 33"):
        R.call("C_bnmf_similarity_at", ptr, *args(k=33))
    with pytest.raises(RError, match=r"query\[0\] = 64"):
        R.call("C_bnmf_similarity_at", ptr, *args(include=R.logical(inc), query=R.integer([64])))
    assert R.L.rstub_protect_depth() == 0
    R.call("C_bnmf_destroy", ptr)
    R.release(ptr)
    e.close()
    assert R.L.rstub_violations() == v0
