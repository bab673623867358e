"""The `.Call` routine of WAIC (C_bnmf_waic in r/bnmf_shim.c), compiled against the stand-in R runtime of tests/r_stub/ and run:
warning-free and registered with its parameter count (CPU); its result is the ctypes binding's, bit for bit (GPU)."""
import os
import re

import numpy as np
import pytest

from rshim import RShim, RError, ROOT, syntax_check


@pytest.fixture(scope="module")
def R():
    if not os.path.exists(os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")):
        pytest.skip("libbnmf.so not built")
    return RShim()


def test_shim_compiles_without_warnings():
    p = syntax_check()
    assert p.returncode == 0 and p.stderr == "", p.stderr


def test_routine_is_registered_with_its_parameter_count(R):
    src = open(os.path.join(ROOT, "r", "bnmf_shim.c")).read()
    m = re.search(r"^SEXP C_bnmf_waic\(([^)]*)\)\s*\{", src, re.M)
    assert m and len([p for p in m.group(1).split(",") if p.strip()]) == 7
    assert R.routines["C_bnmf_waic"] == 7 and R.routines["C_bnmf_waic_at"] == 7
    rsrc = open(os.path.join(ROOT, "r", "bayesNMF_hip.R")).read()
    assert '.Call("C_bnmf_waic"' in rsrc and "get_WAIC = function(" in rsrc


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.gpu
def test_shim_result_is_the_ctypes_result(R):
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import IDS
    from bayesnmf_amd.setup import synth_counts, default_hyperprior_params, apply_hyperprior_params
    v0 = R.L.rstub_violations()
    K, G, N, W = 96, 7, 5, 16
    M, _, _ = synth_counts(K, G, 3, 7, mean_total=1500)
    ptr = R.call("C_bnmf_create", R.int_matrix(M), R.integer([K, G, N]), R.integer([0, 2, 0, 0, 0, 0, W]), R.real(np.ones(1)), R.real([9.0]),
                 R.integer([0]), R.integer([0]))
    for k, v in default_hyperprior_params("gamma", M, N).items():
        R.call("C_bnmf_set_array", ptr, R.integer([IDS[k[0].upper() + k[1:]]]), R.real([float(v)]))
    e = Engine(M, N, prior="gamma", seed=9, window=W, temperature=np.ones(1))   # the shim passes a schedule of one 1.0
    apply_hyperprior_params(e, "gamma", M, N)
    R.take(R.call("C_bnmf_init", ptr)); e.init()
    R.take(R.call("C_bnmf_run", ptr, R.integer([39]), R.logical([False]))); e.run(39)
    used = np.array([1, 1, 0, 1, 1, 1, 0, 0, 1, 1, 1, 1], dtype=np.int32)
    dims = [K, G, N]
    want = e.waic(12, used=used, end_iter=38, pointwise=True)
    got = R.take(R.call("C_bnmf_waic", ptr, R.integer([38]), R.integer([12]), R.logical(used), R.logical([True]), R.logical([True]), R.integer(dims)))
    for k in ("lppd", "p_waic", "elpd_waic", "waic", "se_elpd", "mean_loglik"):
        assert _bits(got[k][0]) == _bits(want[k]), k
    assert got["n_used"][0] == want["n_used"] == 9 and got["n_high_var"][0] == want["n_high_var"]
    assert got["col"].shape == (G, 3)
    for j, k in enumerate(("lppd_col", "p_waic_col", "mean_loglik_col")):
        assert np.array_equal(_bits(got["col"][:, j]), _bits(want[k])), k
    assert np.array_equal(_bits(got["lppd_cell"]), _bits(want["lppd_cell"])) and np.array_equal(_bits(got["p_waic_cell"]), _bits(want["p_waic_cell"]))
    # used = NULL, nothing pointwise: the info fields alone
    lean = R.take(R.call("C_bnmf_waic", ptr, R.integer([40]), R.integer([10]), R.nil(), R.logical([False]), R.logical([False]), R.integer(dims)))
    assert lean["col"] is None and lean["lppd_cell"] is None and lean["p_waic_cell"] is None
    assert _bits(lean["elpd_waic"][0]) == _bits(e.waic(10)["elpd_waic"])
    now = R.take(R.call("C_bnmf_waic", ptr, R.nil(), R.integer([10]), R.nil(), R.logical([False]), R.logical([False]), R.integer(dims)))
    at = R.take(R.call("C_bnmf_waic_at", ptr, R.integer([40]), R.integer([10]), R.nil(), R.logical([False]), R.logical([False]), R.integer(dims)))
    assert _bits(now["elpd_waic"][0]) == _bits(at["elpd_waic"][0]) == _bits(lean["elpd_waic"][0])
    # refusals arrive as R errors with the library's message, the PROTECT stack empty
    with pytest.raises(RError, match="used has 3 entries"):
        R.call("C_bnmf_waic", ptr, R.integer([38]), R.integer([12]), R.logical([1, 1, 1]), R.logical([False]), R.logical([False]), R.integer(dims))
    with pytest.raises(RError, match="are kept"):
        R.call("C_bnmf_waic", ptr, R.integer([41]), R.integer([12]), R.nil(), R.logical([False]), R.logical([False]), R.integer(dims))
    with pytest.raises(RError, match="at least 2"):
        R.call("C_bnmf_waic", ptr, R.integer([38]), R.integer([3]), R.logical([0, 1, 0]), R.logical([False]), R.logical([False]), R.integer(dims))
    assert R.L.rstub_protect_depth() == 0
    R.call("C_bnmf_destroy", ptr)
    R.release(ptr)
    e.close()
    assert R.L.rstub_violations() == v0
