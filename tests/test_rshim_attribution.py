"""The `.Call` routines of the signature attribution (C_bnmf_attribution / C_bnmf_attribution_at in r/bnmf_shim.c), compiled against the
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
    for name in ("C_bnmf_attribution", "C_bnmf_attribution_at"):
        m = re.search(r"^SEXP %s\(([^)]*)\)\s*\{" % name, src, re.M)
        assert m and len([p for p in m.group(1).split(",") if p.strip()]) == 7, name
        assert R.routines[name] == 7
    rsrc = open(os.path.join(ROOT, "r", "bayesNMF_hip.R")).read()
    assert '.Call("C_bnmf_attribution"' in rsrc and "get_attribution = function(" in rsrc


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


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
    dims = [K, G, N]

    def same(got, want, prob):
        assert got["n_used"][0] == want["n_used"] and got["n_present"][0] == want["n_present"]
        assert _bits(got["total"][0]) == _bits(want["total"]) and got["min_load"][0] == want["min_load"]
        S = want["n_used"]
        assert got["load"].shape == (N * G, 4) and got["series"].shape == (N, S)
        for i in range(4):
            assert np.array_equal(_bits(got["load"][:, i].reshape((N, G), order="F")), _bits(want["load"][i])), i
        assert np.array_equal(_bits(got["series"].T), _bits(want["series"]))
        if prob:
            assert got["prob"].shape == (K * N, G)
            assert np.array_equal(_bits(got["prob"].reshape((K, N, G), order="F")), _bits(want["prob"]))
        else:
            assert got["prob"] is None

    want = e.attribution(7, used=used, end_iter=12, min_load=2.0, prob=True)
    got = R.take(R.call("C_bnmf_attribution", ptr, R.integer([12]), R.integer([7]), R.logical(used), R.real([2.0]), R.logical([True]), R.integer(dims)))
    assert want["n_used"] == 5
    same(got, want, True)
    # used = NULL, no prob
    lean = R.take(R.call("C_bnmf_attribution", ptr, R.integer([13]), R.integer([5]), R.nil(), R.real([1.0]), R.logical([False]), R.integer(dims)))
    same(lean, e.attribution(5), False)
    now = R.take(R.call("C_bnmf_attribution", ptr, R.nil(), R.integer([5]), R.nil(), R.real([1.0]), R.logical([False]), R.integer(dims)))
    at = R.take(R.call("C_bnmf_attribution_at", ptr, R.integer([13]), R.integer([5]), R.nil(), R.real([1.0]), R.logical([False]), R.integer(dims)))
    assert np.array_equal(_bits(now["load"]), _bits(at["load"])) and np.array_equal(_bits(now["load"]), _bits(lean["load"]))
    # refusals arrive as R errors with the library's message, the PROTECT stack empty
    with pytest.raises(RError, match="used has 3 entries"):
        R.call("C_bnmf_attribution", ptr, R.integer([12]), R.integer([7]), R.logical([1, 1, 1]), R.real([1.0]), R.logical([False]), R.integer(dims))
    with pytest.raises(RError, match="are kept"):
        R.call("C_bnmf_attribution", ptr, R.integer([14]), R.integer([7]), R.nil(), R.real([1.0]), R.logical([False]), R.integer(dims))
    with pytest.raises(RError, match="at least 2"):
        R.call("C_bnmf_attribution", ptr, R.integer([12]), R.integer([3]), R.logical([0, 1, 0]), R.real([1.0]), R.logical([False]), R.integer(dims))
    with pytest.raises(RError, match="min_load"):
        R.call("C_bnmf_attribution", ptr, R.integer([12]), R.integer([3]), R.nil(), R.real([-1.0]), R.logical([False]), R.integer(dims))
    assert R.L.rstub_protect_depth() == 0
    R.call("C_bnmf_destroy", ptr)
    R.release(ptr)
    e.close()
    assert R.L.rstub_violations() == v0
