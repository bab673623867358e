"""The `.Call` routines of the sparse per-tumour assignment (C_bnmf_prune / C_bnmf_prune_at in r/bnmf_shim.c), compiled against the
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
    for name in ("C_bnmf_prune", "C_bnmf_prune_at"):
        m = re.search(r"^SEXP %s\(([^)]*)\)\s*\{" % name, src, re.M)
        assert m and len([p for p in m.group(1).split(",") if p.strip()]) == 6, name
        assert R.routines[name] == 6
    rsrc = open(os.path.join(ROOT, "r", "bayesNMF_hip.R")).read()
    assert '.Call("C_bnmf_prune"' in rsrc and "get_sparse_assignment = function(max_loss = 0.01, n_steps = 20L, include = NULL" in rsrc
    assert 'idx = "MAP_idx"' in rsrc[rsrc.index("get_sparse_assignment = function"):][:300]


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
    M = M.copy()
    M[:, 5] = 0                                                               # an undefined tumour
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

    def same(got, want, S, exposures):
        for f in ("n_used", "n_included", "n_undefined", "n_single", "n_steps"):
            assert got[f][0] == want[f], f
        for f in ("trials", "max_change", "max_loss"):
            assert _same_bits(got[f], np.array([float(want[f])])), f
        assert _same_bits(np.asarray(got["load"]).T.reshape(4, G, N).transpose(0, 2, 1), want["load"]) and _same_bits(np.asarray(got["tumour"]).T, want["tumour"])
        assert _same_bits(np.asarray(got["series"]).T.reshape(2, S), want["series"]) and _same_bits(np.asarray(got["signature"]).T, want["signature"])
        if exposures:
            assert _same_bits(np.asarray(got["exposures"]).T.reshape(S, G, N).transpose(0, 2, 1), want["exposures"])
        else:
            assert got["exposures"] is None

    opts = lambda steps=5, loss=0.02, ex=1: R.real([steps, loss, ex, G, N])  # noqa: E731
    want = e.prune(7, include=inc, n_steps=5, max_loss=0.02, used=used, end_iter=12, exposures=True)
    got = R.take(R.call("C_bnmf_prune", ptr, R.integer([12]), R.integer([7]), R.logical(used), R.logical(inc), opts()))
    assert want["n_used"] == 5 and want["n_included"] == G - 2 and want["n_undefined"] == 1 and want["max_loss"] == 0.02 and want["trials"] > 0
    same(got, want, 5, True)
    # everything NULL, the current iteration
    lean = R.take(R.call("C_bnmf_prune", ptr, R.integer([13]), R.integer([5]), R.nil(), R.nil(), opts(ex=0)))
    same(lean, e.prune(5, n_steps=5, max_loss=0.02), 5, False)
    now = R.take(R.call("C_bnmf_prune", ptr, R.nil(), R.integer([5]), R.nil(), R.nil(), opts(ex=0)))
    at = R.take(R.call("C_bnmf_prune_at", ptr, R.integer([13]), R.integer([5]), R.nil(), R.nil(), opts(ex=0)))
    assert _same_bits(now["tumour"], at["tumour"]) and _same_bits(now["load"], at["load"]) and _same_bits(now["tumour"], lean["tumour"])
    # refusals arrive as R errors with the library's message, the PROTECT stack empty
    args = lambda **kw: [kw.get("end", R.integer([12])), R.integer([7]), kw.get("used", R.nil()), kw.get("include", R.nil()), kw.get("opts", opts(ex=0))]  # noqa: E731
    with pytest.raises(RError, match="used has 3 entries"):
        R.call("C_bnmf_prune", ptr, *args(used=R.logical([1, 1, 1])))
    with pytest.raises(RError, match="include has 2 flags"):
        R.call("C_bnmf_prune", ptr, *args(include=R.logical([1, 1])))
    with pytest.raises(RError, match="opts has 2 entries"):
        R.call("C_bnmf_prune", ptr, *args(opts=R.real([0.5, 0])))
    with pytest.raises(RError, match="are kept"):
        R.call("C_bnmf_prune", ptr, *args(end=R.integer([14])))
    with pytest.raises(RError, match="max_loss"):
        R.call("C_bnmf_prune", ptr, *args(opts=opts(loss=float("nan"), ex=0)))
    with pytest.raises(RError, match="n_steps"):
        R.call("C_bnmf_prune_at", ptr, *args(opts=opts(steps=0, ex=0)))
    assert R.L.rstub_protect_depth() == 0
    R.call("C_bnmf_destroy", ptr)
    R.release(ptr)
    e.close()
    assert R.L.rstub_violations() == v0
