"""The `.Call` routines of the label-switching correction (C_bnmf_relabel / C_bnmf_relabel_at in r/bnmf_shim.c), compiled against the
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
    for name in ("C_bnmf_relabel", "C_bnmf_relabel_at"):
        m = re.search(r"^SEXP %s\(([^)]*)\)\s*\{" % name, src, re.M)
        assert m and len([p for p in m.group(1).split(",") if p.strip()]) == 8, name
        assert R.routines[name] == 8
    rsrc = open(os.path.join(ROOT, "r", "bayesNMF_hip.R")).read()
    assert '.Call("C_bnmf_relabel"' in rsrc and "get_relabelling = function(" in rsrc


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
    piv = np.asfortranarray(e.get("P")[:, [2, 0, 1]])                           # a pivot that moves every label

    def same(got, want, aligned):
        for k in ("n_used", "n_aligned", "n_unmatched", "rounds", "converged", "n_switched", "n_changed_last"):
            assert got[k][0] == want[k], k
        assert _bits(got["mean_cosine"][0]) == _bits(want["mean_cosine"]) and _bits(got["min_cosine"][0]) == _bits(want["min_cosine"])
        assert got["min_cosine_at"][0] == want["min_cosine_at"] + 1
        S = want["n_used"]
        assert got["perm"].shape == (N, S) and got["cosine"].shape == (N, S) and got["confusion"].shape == (N, N)
        assert np.array_equal(got["perm"].T, want["perm"] + 1)
        assert np.array_equal(_bits(got["cosine"].T), _bits(want["cosine"]))
        assert np.array_equal(got["confusion"], want["confusion"].astype(float))
        assert got["P"].shape == (K * N, 2) and got["E"].shape == (N * G, 2)
        for i, nm in enumerate(("mean", "var")):
            assert np.array_equal(_bits(got["P"][:, i].reshape((K, N), order="F")), _bits(want["P_" + nm])), nm
            assert np.array_equal(_bits(got["E"][:, i].reshape((N, G), order="F")), _bits(want["E_" + nm])), nm
        if aligned:
            assert got["aligned_P"].shape == (K * N, S) and got["aligned_E"].shape == (N * G, S)
            assert np.array_equal(_bits(got["aligned_P"].T.reshape((S, N, K)).transpose(0, 2, 1)), _bits(want["aligned_P"]))
            assert np.array_equal(_bits(got["aligned_E"].T.reshape((S, G, N)).transpose(0, 2, 1)), _bits(want["aligned_E"]))
        else:
            assert got["aligned_P"] is None and got["aligned_E"] is None

    want = e.relabel(7, used=used, end_iter=12, pivot_P=piv, max_rounds=10, aligned=True)
    got = R.take(R.call("C_bnmf_relabel", ptr, R.integer([12]), R.integer([7]), R.logical(used), R.real_matrix(piv), R.integer([10]), R.logical([True]),
                        R.integer(dims)))
    assert want["n_used"] == 5 and want["n_switched"] == 5
    same(got, want, True)
    # used = NULL, pivot = NULL, one round, no aligned samples
    lean = R.take(R.call("C_bnmf_relabel", ptr, R.integer([13]), R.integer([5]), R.nil(), R.nil(), R.integer([1]), R.logical([False]), R.integer(dims)))
    same(lean, e.relabel(5, max_rounds=1), False)
    now = R.take(R.call("C_bnmf_relabel", ptr, R.nil(), R.integer([5]), R.nil(), R.nil(), R.integer([1]), R.logical([False]), R.integer(dims)))
    at = R.take(R.call("C_bnmf_relabel_at", ptr, R.integer([13]), R.integer([5]), R.nil(), R.nil(), R.integer([1]), R.logical([False]), R.integer(dims)))
    assert np.array_equal(_bits(now["E"]), _bits(at["E"])) and np.array_equal(_bits(now["E"]), _bits(lean["E"]))
    # refusals arrive as R errors with the library's message, the PROTECT stack empty
    with pytest.raises(RError, match="used has 3 entries"):
        R.call("C_bnmf_relabel", ptr, R.integer([12]), R.integer([7]), R.logical([1, 1, 1]), R.nil(), R.integer([10]), R.logical([False]), R.integer(dims))
    with pytest.raises(RError, match="pivot_P has 6 entries"):
        R.call("C_bnmf_relabel", ptr, R.integer([12]), R.integer([7]), R.nil(), R.real(np.ones(6)), R.integer([10]), R.logical([False]), R.integer(dims))
    with pytest.raises(RError, match="are kept"):
        R.call("C_bnmf_relabel", ptr, R.integer([14]), R.integer([7]), R.nil(), R.nil(), R.integer([10]), R.logical([False]), R.integer(dims))
    with pytest.raises(RError, match="at least 2"):
        R.call("C_bnmf_relabel", ptr, R.integer([12]), R.integer([3]), R.logical([0, 1, 0]), R.nil(), R.integer([10]), R.logical([False]), R.integer(dims))
    with pytest.raises(RError, match="max_rounds"):
        R.call("C_bnmf_relabel", ptr, R.integer([12]), R.integer([3]), R.nil(), R.nil(), R.integer([0]), R.logical([False]), R.integer(dims))
    assert R.L.rstub_protect_depth() == 0
    R.call("C_bnmf_destroy", ptr)
    R.release(ptr)
    e.close()
    assert R.L.rstub_violations() == v0
