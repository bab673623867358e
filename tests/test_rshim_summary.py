"""The `.Call` routines of the cohort summary of signatures (C_bnmf_summary / C_bnmf_summary_at in r/bnmf_shim.c), compiled against the
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
    for name in ("C_bnmf_summary", "C_bnmf_summary_at"):
        m = re.search(r"^SEXP %s\(([^)]*)\)\s*\{" % name, src, re.M)
        assert m and len([p for p in m.group(1).split(",") if p.strip()]) == 8, name
        assert R.routines[name] == 8
    rsrc = open(os.path.join(ROOT, "r", "bayesNMF_hip.R")).read()
    assert '.Call("C_bnmf_summary"' in rsrc and "get_summary = function(probs" in rsrc


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
    pm = np.tile(np.arange(N, dtype=np.int32), (7, 1))
    pm[2] = [1, 0, 2]
    pm[5] = -1
    probs = [0.0, 0.5, 0.9]

    def opts(ml, ci, series):
        return R.real([ml, ci, 1.0 if series else 0.0, G, N])

    def same(got, want, series):
        for k in ("n_used", "n_aligned", "n_included", "n_left_out", "n_levels", "n_blocks"):
            assert got[k][0] == want[k], k
        assert int(got["n_nonfinite"][0]) == want["n_nonfinite"]
        S, Q = want["n_used"], want["stat"].shape[0]
        for k in ("min_load", "credible_interval"):
            assert _same_bits(got[k], np.array([want[k]])), k
        assert got["stat"].shape == (N, 5 * Q)
        for q in range(Q):
            for i in range(5):
                assert _same_bits(got["stat"][:, 5 * q + i], want["stat"][q, i]), (q, i)
        if series:
            assert got["series"].shape == (N, Q * S)
            for q in range(Q):
                for s in range(S):
                    assert _same_bits(got["series"][:, S * q + s], want["series"][q, s])
        else:
            assert got["series"] is None

    want = e.summary(7, probs=probs, include=inc, perm=pm, used=used, end_iter=12, min_load=2.0, credible_interval=0.9, series=True)
    got = R.take(R.call("C_bnmf_summary", ptr, R.integer([12]), R.integer([7]), R.logical(used), R.logical(inc), R.int_matrix(pm), R.real(probs),
                        opts(2.0, 0.9, True)))
    assert want["n_used"] == 5 and want["n_aligned"] == 4 and want["n_included"] == 8 and want["n_left_out"] == 1 and want["n_levels"] == 3
    same(got, want, True)
    # used = NULL, include = NULL, perm = NULL, no series
    lean = R.take(R.call("C_bnmf_summary", ptr, R.integer([13]), R.integer([5]), R.nil(), R.nil(), R.nil(), R.real([0.5]), opts(1.0, 0.95, False)))
    same(lean, e.summary(5, probs=(0.5,)), False)
    now = R.take(R.call("C_bnmf_summary", ptr, R.nil(), R.integer([5]), R.nil(), R.nil(), R.nil(), R.real([0.5]), opts(1.0, 0.95, False)))
    at = R.take(R.call("C_bnmf_summary_at", ptr, R.integer([13]), R.integer([5]), R.nil(), R.nil(), R.nil(), R.real([0.5]), opts(1.0, 0.95, False)))
    assert _same_bits(now["stat"], at["stat"])
    # refusals arrive as R errors with the library's message, the PROTECT stack empty
    with pytest.raises(RError, match="used has 3 entries"):
        R.call("C_bnmf_summary", ptr, R.integer([12]), R.integer([7]), R.logical([1, 1, 1]), R.nil(), R.nil(), R.real([0.5]), opts(1.0, 0.95, False))
    with pytest.raises(RError, match="include has 2 flags for 9 tumours"):
        R.call("C_bnmf_summary", ptr, R.integer([12]), R.integer([7]), R.nil(), R.logical([1, 1]), R.nil(), R.real([0.5]), opts(1.0, 0.95, False))
    with pytest.raises(RError, match="perm has 6 entries"):
        R.call("C_bnmf_summary", ptr, R.integer([12]), R.integer([7]), R.nil(), R.nil(), R.int_matrix(pm[:2]), R.real([0.5]), opts(1.0, 0.95, False))
    with pytest.raises(RError, match="opts has 2 entries"):
        R.call("C_bnmf_summary", ptr, R.integer([12]), R.integer([7]), R.nil(), R.nil(), R.nil(), R.real([0.5]), R.real([1.0, 0.95]))
    with pytest.raises(RError, match="are kept"):
        R.call("C_bnmf_summary", ptr, R.integer([14]), R.integer([7]), R.nil(), R.nil(), R.nil(), R.real([0.5]), opts(1.0, 0.95, False))
    with pytest.raises(RError, match=r"probs\[1\]"):
        R.call("C_bnmf_summary", ptr, R.integer([12]), R.integer([3]), R.nil(), R.nil(), R.nil(), R.real([0.5, 0.5]), opts(1.0, 0.95, False))
    with pytest.raises(RError, match="L = 9"):
        R.call("C_bnmf_summary", ptr, R.integer([12]), R.integer([3]), R.nil(), R.nil(), R.nil(), R.real(np.linspace(0, 1, 9)), opts(1.0, 0.95, False))
    with pytest.raises(RError, match="min_load"):
        R.call("C_bnmf_summary", ptr, R.integer([12]), R.integer([3]), R.nil(), R.nil(), R.nil(), R.real([0.5]), opts(-1.0, 0.95, False))
    with pytest.raises(RError, match="credible_interval"):
        R.call("C_bnmf_summary", ptr, R.integer([12]), R.integer([3]), R.nil(), R.nil(), R.nil(), R.real([0.5]), opts(1.0, 1.0, False))
    assert R.L.rstub_protect_depth() == 0
    R.call("C_bnmf_destroy", ptr)
    R.release(ptr)
    e.close()
    assert R.L.rstub_violations() == v0
