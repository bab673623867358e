"""The `.Call` routines of the subtypes of tumours (C_bnmf_subtypes / C_bnmf_subtypes_at in r/bnmf_shim.c), compiled against the
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
    for name in ("C_bnmf_subtypes", "C_bnmf_subtypes_at"):
        m = re.search(r"^SEXP %s\(([^)]*)\)\s*\{" % name, src, re.M)
        assert m and len([p for p in m.group(1).split(",") if p.strip()]) == 9, name
        assert R.routines[name] == 9
    rsrc = open(os.path.join(ROOT, "r", "bayesNMF_hip.R")).read()
    assert '.Call("C_bnmf_subtypes"' in rsrc and "get_subtypes = function(n_subtypes = NULL, centres = NULL, seeds = NULL, include = NULL, query = NULL" in rsrc
    assert 'idx = "MAP_idx"' in rsrc[rsrc.index("get_subtypes = function"):][:500]


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
    Ecur = np.asarray(e.get("E"), dtype=np.float64)
    c0 = np.asfortranarray((Ecur / Ecur.sum(axis=0))[:, [3, 30, 60]])
    perm = np.tile(np.array([2, 0, 1], dtype=np.int32), (7, 1))
    perm[3] = -1                                                                 # an unmatched sample

    def same(got, want, Cn, Q, S, labels):
        for f in ("n_used", "n_matched", "n_unmatched", "n_included", "n_left_out", "C", "n_steps", "n_query", "n_not_converged", "n_certain", "n_never_assigned",
                  "smallest_subtype_at"):
            assert got[f][0] == want[f], f
        assert int(got["least_certain_at"][0]) == want["least_certain_at"]
        for f in ("mean_certainty", "least_certain", "smallest_subtype", "min_certainty"):
            assert _same_bits(got[f], np.array([want[f]])), f
        assert _same_bits(np.asarray(got["membership"]).T, want["membership"]) and np.array_equal(np.asarray(got["label"]).ravel(), want["label"])
        assert _same_bits(np.asarray(got["tumour"]).T, want["tumour"]) and _same_bits(np.asarray(got["size"]).T, want["size"])
        assert _same_bits(np.asarray(got["centre"]).T.reshape(4, Cn, N).transpose(0, 2, 1), want["centre"])
        assert _same_bits(np.asarray(got["series"]).T, want["series"])
        if Q > 0:
            assert _same_bits(np.asarray(got["together"]).T, want["together"])
        else:
            assert got["together"] is None
        if labels:
            assert np.array_equal(np.asarray(got["labels"]).T.reshape(S, G), want["labels"])
        else:
            assert got["labels"] is None

    q = np.array([3, 69, 3], dtype=np.int32)
    opts = lambda steps=20, mc=0.8, lab=1: R.real([steps, mc, lab, K, G, N])  # noqa: E731
    want = e.subtypes(7, c0, include=inc, perm=perm, n_steps=20, query=q, min_certainty=0.8, used=used, end_iter=12, labels=True)
    got = R.take(R.call("C_bnmf_subtypes", ptr, R.integer([12]), R.integer([7]), R.logical(used), R.logical(inc), R.int_matrix(perm), R.real_matrix(c0),
                        R.integer(q), opts()))
    assert want["n_used"] == 5 and want["n_unmatched"] == 1 and want["n_left_out"] == 2 and want["min_certainty"] == 0.8
    same(got, want, 3, 3, 5, True)
    # used, include, perm and query NULL, the current iteration
    lean = R.take(R.call("C_bnmf_subtypes", ptr, R.integer([13]), R.integer([5]), R.nil(), R.nil(), R.nil(), R.real_matrix(c0), R.nil(), opts(lab=0)))
    same(lean, e.subtypes(5, c0, n_steps=20, min_certainty=0.8), 3, 0, 5, False)
    now = R.take(R.call("C_bnmf_subtypes", ptr, R.nil(), R.integer([5]), R.nil(), R.nil(), R.nil(), R.real_matrix(c0), R.nil(), opts(lab=0)))
    at = R.take(R.call("C_bnmf_subtypes_at", ptr, R.integer([13]), R.integer([5]), R.nil(), R.nil(), R.nil(), R.real_matrix(c0), R.nil(), opts(lab=0)))
    assert _same_bits(now["tumour"], at["tumour"]) and _same_bits(now["centre"], at["centre"]) and _same_bits(now["tumour"], lean["tumour"])
    # refusals arrive as R errors with the library's message, the PROTECT stack empty
    args = lambda **kw: [kw.get("end", R.integer([12])), R.integer([7]), kw.get("used", R.nil()), kw.get("include", R.nil()), kw.get("perm", R.nil()),  # noqa: E731
                         kw.get("cen", R.real_matrix(c0)), kw.get("query", R.nil()), kw.get("opts", opts())]
    with pytest.raises(RError, match="used has 3 entries"):
        R.call("C_bnmf_subtypes", ptr, *args(used=R.logical([1, 1, 1])))
    with pytest.raises(RError, match="include has 2 flags"):
        R.call("C_bnmf_subtypes", ptr, *args(include=R.logical([1, 1])))
    with pytest.raises(RError, match="perm has 6 entries"):
        R.call("C_bnmf_subtypes", ptr, *args(perm=R.int_matrix(np.zeros((2, 3), dtype=np.int32))))
    with pytest.raises(RError, match="centres0 has 4 entries"):
        R.call("C_bnmf_subtypes", ptr, *args(cen=R.real([0.5, 0.5, 0.5, 0.5])))
    with pytest.raises(RError, match="opts has 2 entries"):
        R.call("C_bnmf_subtypes", ptr, *args(opts=R.real([20, 0.9])))
    with pytest.raises(RError, match="are kept"):
        R.call("C_bnmf_subtypes", ptr, *args(end=R.integer([14])))
    with pytest.raises(RError, match="min_certainty"):
        R.call("C_bnmf_subtypes", ptr, *args(opts=opts(mc=float("nan"))))
    with pytest.raises(RError, match="n_steps = 0"):
        R.call("C_bnmf_subtypes_at", ptr, *args(opts=opts(steps=0)))
    with pytest.raises(RError, match=r"query\[0\] = 64"):
        R.call("C_bnmf_subtypes_at", ptr, *args(include=R.logical(inc), query=R.integer([64])))
    assert R.L.rstub_protect_depth() == 0
    R.call("C_bnmf_destroy", ptr)
    R.release(ptr)
    e.close()
    assert R.L.rstub_violations() == v0
