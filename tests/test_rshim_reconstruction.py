"""The `.Call` routines of the reconstruction quality per tumour (C_bnmf_reconstruction / C_bnmf_reconstruction_at in r/bnmf_shim.c),
compiled against the stand-in R runtime of tests/r_stub/ and run: warning-free and registered with their parameter count (CPU); their
result is the ctypes binding's, bit for bit (GPU)."""
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
    for name in ("C_bnmf_reconstruction", "C_bnmf_reconstruction_at"):
        m = re.search(r"^SEXP %s\(([^)]*)\)\s*\{" % name, src, re.M)
        assert m and len([p for p in m.group(1).split(",") if p.strip()]) == 7, name
        assert R.routines[name] == 7
    rsrc = open(os.path.join(ROOT, "r", "bayesNMF_hip.R")).read()
    assert '.Call("C_bnmf_reconstruction"' in rsrc and "get_reconstruction = function(end_iter" in rsrc
    assert "min_cosine = 0.9, min_drop = 0.01" in rsrc and 'idx = "MAP_idx", min_cosine' in rsrc


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
    M = M.copy()
    M[:, 4] = 0                                                                 # an all-zero tumour: NaN rows, worst_at skips it
    ptr = R.call("C_bnmf_create", R.int_matrix(M), R.integer([K, G, N]), R.integer([0, 2, 0, 0, 0, 0, W]), R.real(np.ones(1)), R.real([9.0]),
                 R.integer([0]), R.integer([0]))
    for k, v in default_hyperprior_params("gamma", M, N).items():
        R.call("C_bnmf_set_array", ptr, R.integer([IDS[k[0].upper() + k[1:]]]), R.real([float(v)]))
    e = Engine(M, N, prior="gamma", seed=9, window=W, temperature=np.ones(1))   # the shim passes a schedule of one 1.0
    apply_hyperprior_params(e, "gamma", M, N)
    R.take(R.call("C_bnmf_init", ptr)); e.init()
    R.take(R.call("C_bnmf_run", ptr, R.integer([12]), R.logical([False]))); e.run(12)
    used = np.array([1, 0, 1, 1, 0, 1, 1], dtype=np.int32)
    dims = [K, G, N]

    def same(got, want):
        for k in ("n_used", "n_undefined"):
            assert got[k][0] == want[k], k
        for k in ("n_poor", "n_needed", "worst_at"):
            assert int(got[k][0]) == want[k], k
        for k in ("min_cosine", "min_drop", "worst_cosine"):
            assert _same_bits(got[k], np.array([want[k]])), k
        assert _same_bits(got["tumour"].T, want["tumour"]) and _same_bits(np.ravel(got["series"]), want["series"]) and _same_bits(got["signature"].T, want["signature"])
        assert _same_bits(got["drop"].T.reshape(4, G, N).transpose(0, 2, 1), want["drop"])

    want = e.reconstruction(7, used=used, end_iter=12, min_cosine=0.95, min_drop=0.02)
    got = R.take(R.call("C_bnmf_reconstruction", ptr, R.integer([12]), R.integer([7]), R.logical(used), R.real([0.95]), R.real([0.02]), R.integer(dims)))
    assert want["n_used"] == 5 and want["n_undefined"] == 1 and want["min_cosine"] == 0.95
    same(got, want)
    # used = NULL, the current iteration
    lean = R.take(R.call("C_bnmf_reconstruction", ptr, R.integer([13]), R.integer([5]), R.nil(), R.real([0.9]), R.real([0.01]), R.integer(dims)))
    same(lean, e.reconstruction(5))
    now = R.take(R.call("C_bnmf_reconstruction", ptr, R.nil(), R.integer([5]), R.nil(), R.real([0.9]), R.real([0.01]), R.integer(dims)))
    at = R.take(R.call("C_bnmf_reconstruction_at", ptr, R.integer([13]), R.integer([5]), R.nil(), R.real([0.9]), R.real([0.01]), R.integer(dims)))
    assert _same_bits(now["tumour"], at["tumour"]) and _same_bits(now["drop"], at["drop"]) and _same_bits(now["tumour"], lean["tumour"])
    # refusals arrive as R errors with the library's message, the PROTECT stack empty
    with pytest.raises(RError, match="used has 3 entries"):
        R.call("C_bnmf_reconstruction", ptr, R.integer([12]), R.integer([7]), R.logical([1, 1, 1]), R.real([0.9]), R.real([0.01]), R.integer(dims))
    with pytest.raises(RError, match="are kept"):
        R.call("C_bnmf_reconstruction", ptr, R.integer([14]), R.integer([7]), R.nil(), R.real([0.9]), R.real([0.01]), R.integer(dims))
    with pytest.raises(RError, match="min_drop"):
        R.call("C_bnmf_reconstruction", ptr, R.integer([12]), R.integer([7]), R.nil(), R.real([0.9]), R.real([float("nan")]), R.integer(dims))
    with pytest.raises(RError, match="1 used sample"):
        R.call("C_bnmf_reconstruction_at", ptr, R.integer([12]), R.integer([3]), R.logical([0, 1, 0]), R.real([0.9]), R.real([0.01]), R.integer(dims))
    assert R.L.rstub_protect_depth() == 0
    R.call("C_bnmf_destroy", ptr)
    R.release(ptr)
    e.close()
    assert R.L.rstub_violations() == v0
