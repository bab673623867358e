"""The `.Call` routines of the trade-offs between signatures (C_bnmf_tradeoff / C_bnmf_tradeoff_at in r/bnmf_shim.c), compiled against the
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
    for name in ("C_bnmf_tradeoff", "C_bnmf_tradeoff_at"):
        m = re.search(r"^SEXP %s\(([^)]*)\)\s*\{" % name, src, re.M)
        assert m and len([p for p in m.group(1).split(",") if p.strip()]) == 9, name
        assert R.routines[name] == 9
    rsrc = open(os.path.join(ROOT, "r", "bayesNMF_hip.R")).read()
    assert '.Call("C_bnmf_tradeoff"' in rsrc and "get_tradeoff = function(sets = NULL, query = NULL, include = NULL, relabel = TRUE, min_corr = 0.5" in rsrc
    assert 'idx = "MAP_idx"' in rsrc[rsrc.index("get_tradeoff = function"):][:300]


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
    perm = np.tile(np.arange(N, dtype=np.int32), (7, 1))
    perm[2] = [1, 0, 2]
    perm[5] = -1                                                              # an unmatched sample
    sets, q = np.array([0, -1, 0], dtype=np.int32), np.array([3, 69, 3], dtype=np.int32)

    def same(got, want, C, Q):
        for f in ("n_used", "n_matched", "n_unmatched", "n_included", "n_left_out", "n_sets", "n_query", "n_traded", "strongest_pair_at"):
            assert got[f][0] == want[f], f
        for f in ("strongest_pair", "mean_ratio", "min_corr"):
            assert _same_bits(got[f], np.array([want[f]])), f
        assert _same_bits(np.asarray(got["tumour"]).T, want["tumour"]) and np.array_equal(got["pair_at"], want["pair_at"])
        assert _same_bits(np.asarray(got["pair"]).T.reshape(5, N, N), want["pair"])
        if Q:
            assert _same_bits(np.asarray(got["dense"]).reshape(Q, 2, N, N), want["dense"])
        else:
            assert got["dense"] is None
        if C:
            assert _same_bits(np.asarray(got["setstat"]).reshape(4, C, G), want["setstat"])
        else:
            assert got["setstat"] is None

    opts = lambda mc=0.4, C=1: R.real([mc, C, G, N])  # noqa: E731
    pm = lambda: R.int_matrix(perm)  # noqa: E731
    want = e.tradeoff(7, include=inc, perm=perm, sets=sets, query=q, min_corr=0.4, used=used, end_iter=12)
    got = R.take(R.call("C_bnmf_tradeoff", ptr, R.integer([12]), R.integer([7]), R.logical(used), R.logical(inc), pm(), R.integer(sets), R.integer(q), opts()))
    assert want["n_used"] == 5 and want["n_unmatched"] == 1 and want["n_left_out"] == 2 and want["min_corr"] == 0.4 and want["n_query"] == 3
    same(got, want, 1, 3)
    # everything NULL, the current iteration
    lean = R.take(R.call("C_bnmf_tradeoff", ptr, R.integer([13]), R.integer([5]), R.nil(), R.nil(), R.nil(), R.nil(), R.nil(), opts(C=0)))
    same(lean, e.tradeoff(5, min_corr=0.4), 0, 0)
    now = R.take(R.call("C_bnmf_tradeoff", ptr, R.nil(), R.integer([5]), R.nil(), R.nil(), R.nil(), R.nil(), R.nil(), opts(C=0)))
    at = R.take(R.call("C_bnmf_tradeoff_at", ptr, R.integer([13]), R.integer([5]), R.nil(), R.nil(), R.nil(), R.nil(), R.nil(), opts(C=0)))
    assert _same_bits(now["tumour"], at["tumour"]) and _same_bits(now["pair"], at["pair"]) and _same_bits(now["tumour"], lean["tumour"])
    # refusals arrive as R errors with the library's message, the PROTECT stack empty
    args = lambda **kw: [kw.get("end", R.integer([12])), R.integer([7]), kw.get("used", R.nil()), kw.get("include", R.nil()), kw.get("perm", R.nil()),  # noqa: E731
                         kw.get("sets", R.nil()), kw.get("query", R.nil()), kw.get("opts", opts(C=0))]
    with pytest.raises(RError, match="used has 3 entries"):
        R.call("C_bnmf_tradeoff", ptr, *args(used=R.logical([1, 1, 1])))
    with pytest.raises(RError, match="include has 2 flags"):
        R.call("C_bnmf_tradeoff", ptr, *args(include=R.logical([1, 1])))
    with pytest.raises(RError, match="perm has 3 entries"):
        R.call("C_bnmf_tradeoff", ptr, *args(perm=R.integer([0, 1, 2])))
    with pytest.raises(RError, match="sets has 2 labels"):
        R.call("C_bnmf_tradeoff", ptr, *args(sets=R.integer([0, 0])))
    with pytest.raises(RError, match="opts has 2 entries"):
        R.call("C_bnmf_tradeoff", ptr, *args(opts=R.real([0.5, 0])))
    with pytest.raises(RError, match="are kept"):
        R.call("C_bnmf_tradeoff", ptr, *args(end=R.integer([14])))
    with pytest.raises(RError, match="min_corr"):
        R.call("C_bnmf_tradeoff", ptr, *args(opts=opts(mc=float("nan"), C=0)))
    with pytest.raises(RError, match="set 1 is empty"):
        R.call("C_bnmf_tradeoff_at", ptr, *args(sets=R.integer([0, 0, 2]), opts=opts(C=3)))
    assert R.L.rstub_protect_depth() == 0
    R.call("C_bnmf_destroy", ptr)
    R.release(ptr)
    e.close()
    assert R.L.rstub_violations() == v0
