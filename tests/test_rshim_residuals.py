"""The `.Call` routines of the residual structure (C_bnmf_residuals / C_bnmf_residuals_at in r/bnmf_shim.c), compiled against the
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
    for name in ("C_bnmf_residuals", "C_bnmf_residuals_at"):
        m = re.search(r"^SEXP %s\(([^)]*)\)\s*\{" % name, src, re.M)
        assert m and len([p for p in m.group(1).split(",") if p.strip()]) == 6, name
        assert R.routines[name] == 6
    rsrc = open(os.path.join(ROOT, "r", "bayesNMF_hip.R")).read()
    assert '.Call("C_bnmf_residuals"' in rsrc and "get_residuals = function(include = NULL, n_steps = 100, max_dispersion = 2.0, reference_P = NULL" in rsrc
    assert 'idx = "MAP_idx"' in rsrc[rsrc.index("get_residuals = function"):][:300]


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

    def same(got, want):
        for f in ("n_used", "n_flat", "n_included", "n_left_out", "n_steps", "n_biased", "n_overdispersed", "worst_type_at", "min_agreement_at"):
            assert got[f][0] == want[f], f
        for f in ("lambda", "share", "move", "mean_share", "min_agreement", "worst_type", "max_dispersion"):
            assert _same_bits(got[f], np.array([want[f]])), f
        for f in ("gram", "type", "component", "tumour", "series"):
            assert _same_bits(np.asarray(got[f]).T, want[f]), f

    opts = lambda steps=20, md=1.5: R.real([steps, md, K, G])  # noqa: E731
    want = e.residuals(7, include=inc, n_steps=20, max_dispersion=1.5, used=used, end_iter=12)
    got = R.take(R.call("C_bnmf_residuals", ptr, R.integer([12]), R.integer([7]), R.logical(used), R.logical(inc), opts()))
    assert want["n_used"] == 5 and want["n_left_out"] == 2 and want["max_dispersion"] == 1.5 and want["n_steps"] == 20
    same(got, want)
    # used and include NULL, the current iteration
    lean = R.take(R.call("C_bnmf_residuals", ptr, R.integer([13]), R.integer([5]), R.nil(), R.nil(), opts()))
    same(lean, e.residuals(5, n_steps=20, max_dispersion=1.5))
    now = R.take(R.call("C_bnmf_residuals", ptr, R.nil(), R.integer([5]), R.nil(), R.nil(), opts()))
    at = R.take(R.call("C_bnmf_residuals_at", ptr, R.integer([13]), R.integer([5]), R.nil(), R.nil(), opts()))
    assert _same_bits(now["tumour"], at["tumour"]) and _same_bits(now["gram"], at["gram"]) and _same_bits(now["tumour"], lean["tumour"])
    # refusals arrive as R errors with the library's message, the PROTECT stack empty
    args = lambda **kw: [kw.get("end", R.integer([12])), R.integer([7]), kw.get("used", R.nil()), kw.get("include", R.nil()), kw.get("opts", opts())]  # noqa: E731
    with pytest.raises(RError, match="used has 3 entries"):
        R.call("C_bnmf_residuals", ptr, *args(used=R.logical([1, 1, 1])))
    with pytest.raises(RError, match="include has 2 flags"):
        R.call("C_bnmf_residuals", ptr, *args(include=R.logical([1, 1])))
    with pytest.raises(RError, match="opts has 2 entries"):
        R.call("C_bnmf_residuals", ptr, *args(opts=R.real([20, 0.9])))
    with pytest.raises(RError, match="are kept"):
        R.call("C_bnmf_residuals", ptr, *args(end=R.integer([14])))
    with pytest.raises(RError, match="max_dispersion"):
        R.call("C_bnmf_residuals", ptr, *args(opts=opts(md=float("nan"))))
    with pytest.raises(RError, match="n_steps = 0"):
        R.call("C_bnmf_residuals_at", ptr, *args(opts=opts(steps=0)))
    assert R.L.rstub_protect_depth() == 0
    R.call("C_bnmf_destroy", ptr)
    R.release(ptr)
    e.close()
    assert R.L.rstub_violations() == v0
