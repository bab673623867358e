"""The `.Call` routines of the mixing diagnostics (C_bnmf_mixing / C_bnmf_mixing_at in r/bnmf_shim.c), compiled against the stand-in R
runtime of tests/r_stub/ and run: warning-free and registered with their parameter count (CPU); their result is the ctypes binding's,
bit for bit, and the refusals surface through Rf_error (GPU)."""
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


def test_routines_are_registered_with_their_parameter_count(R):
    src = open(os.path.join(ROOT, "r", "bnmf_shim.c")).read()
    for name in ("C_bnmf_mixing", "C_bnmf_mixing_at"):
        m = re.search(r"^SEXP %s\(([^)]*)\)\s*\{" % name, src, re.M)
        assert m and len([p for p in m.group(1).split(",") if p.strip()]) == 7
        assert R.routines[name] == 7
    rsrc = open(os.path.join(ROOT, "r", "bayesNMF_hip.R")).read()
    assert '.Call("C_bnmf_mixing"' in rsrc and "get_mixing = function(" in rsrc


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.gpu
def test_shim_result_is_the_ctypes_result(R):
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import IDS, MIX_ROWS
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
    keep = np.array([1, 0, 1, 1, 1], dtype=np.int32)
    dims = [K, G, N]
    want = e.mixing(12, used=used, end_iter=38, keep=keep)
    got = R.take(R.call("C_bnmf_mixing", ptr, R.integer([38]), R.integer([12]), R.logical(used), R.logical(keep), R.logical([True]), R.integer(dims)))
    assert got["n_used"][0] == want["n_used"] == 9 and got["n_half"][0] == want["n_half"] == 4
    for k in ("n_const", "n_ran_out", "n_low_ess", "n_high_rhat"):
        assert got[k][0] == want[k], k
    for k in ("min_ess_P", "min_ess_E", "max_rhat_P", "max_rhat_E"):
        assert _bits(got[k][0]) == _bits(want[k]), k
        assert got[k + "_at"][0] == want[k + "_at"] + 1, k                      # 1-based positions
    assert got["P"].shape == (K * N, 11) and got["E"].shape == (N * G, 11)
    for j, k in enumerate(MIX_ROWS):
        assert np.array_equal(_bits(got["P"][:, j]), _bits(want[k + "_P"].ravel(order="F"))), k
        assert np.array_equal(_bits(got["E"][:, j]), _bits(want[k + "_E"].ravel(order="F"))), k
    # used = keep = NULL, no arrays: the summary alone
    lean = R.take(R.call("C_bnmf_mixing", ptr, R.integer([40]), R.integer([10]), R.nil(), R.nil(), R.logical([False]), R.integer(dims)))
    assert lean["P"] is None and lean["E"] is None
    assert _bits(lean["min_ess_E"][0]) == _bits(e.mixing(10, arrays=False)["min_ess_E"])
    now = R.take(R.call("C_bnmf_mixing", ptr, R.nil(), R.integer([10]), R.nil(), R.nil(), R.logical([False]), R.integer(dims)))
    at = R.take(R.call("C_bnmf_mixing_at", ptr, R.integer([40]), R.integer([10]), R.nil(), R.nil(), R.logical([False]), R.integer(dims)))
    assert _bits(now["min_ess_E"][0]) == _bits(at["min_ess_E"][0]) == _bits(lean["min_ess_E"][0])
    # refusals arrive as R errors with the library's message, the PROTECT stack empty
    with pytest.raises(RError, match="used has 3 entries"):
        R.call("C_bnmf_mixing", ptr, R.integer([38]), R.integer([12]), R.logical([1, 1, 1]), R.nil(), R.logical([False]), R.integer(dims))
    with pytest.raises(RError, match="keep has 2 entries"):
        R.call("C_bnmf_mixing", ptr, R.integer([38]), R.integer([12]), R.nil(), R.logical([1, 1]), R.logical([False]), R.integer(dims))
    with pytest.raises(RError, match="are kept"):
        R.call("C_bnmf_mixing", ptr, R.integer([41]), R.integer([12]), R.nil(), R.nil(), R.logical([False]), R.integer(dims))
    with pytest.raises(RError, match="at least 4"):
        R.call("C_bnmf_mixing_at", ptr, R.integer([38]), R.integer([5]), R.logical([0, 1, 0, 1, 1]), R.nil(), R.logical([False]), R.integer(dims))
    assert R.L.rstub_protect_depth() == 0
    R.call("C_bnmf_destroy", ptr)
    R.release(ptr)
    e.close()
    assert R.L.rstub_violations() == v0
