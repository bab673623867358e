"""The `.Call` routines of the decomposition into a reference catalogue (C_bnmf_decompose / C_bnmf_decompose_at in r/bnmf_shim.c), compiled
against the stand-in R runtime of tests/r_stub/ and run: warning-free and registered with their parameter count (CPU); their result is
the ctypes binding's, bit for bit (GPU)."""
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
    for name in ("C_bnmf_decompose", "C_bnmf_decompose_at"):
        m = re.search(r"^SEXP %s\(([^)]*)\)\s*\{" % name, src, re.M)
        assert m and len([p for p in m.group(1).split(",") if p.strip()]) == 9, name
        assert R.routines[name] == 9
    rsrc = open(os.path.join(ROOT, "r", "bayesNMF_hip.R")).read()
    assert '.Call("C_bnmf_decompose"' in rsrc and "get_decomposition = function(" in rsrc


def _bits(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = np.uint64(0x7FF8000000000000)      # a NaN is a NaN (the cosine of a factor that is not kept)
    return b


@pytest.mark.gpu
def test_shim_result_is_the_ctypes_result(R):
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import IDS
    from bayesnmf_amd.setup import synth_counts, default_hyperprior_params, apply_hyperprior_params
    v0 = R.L.rstub_violations()
    K, G, N, W, NR = 70, 9, 3, 8, 6
    M, _, _ = synth_counts(K, G, 3, 7, mean_total=1500)
    cat = np.asfortranarray(np.random.default_rng(5).gamma(0.4, 1.0, size=(K, NR)))
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

    def same(got, want, weights):
        S = want["n_used"]
        assert got["n_used"][0] == S and got["n_steps"][0] == want["n_steps"] and got["R"][0] == NR and got["n_present"][0] == want["n_present"]
        assert got["min_cosine_at"][0] == want["min_cosine_at"] and got["min_share"][0] == want["min_share"]
        for k in ("max_rel_change", "min_cosine"):
            assert _bits(got[k][0]) == _bits(want[k]), k
        assert got["weight"].shape == (NR * N, 4) and got["fit"].shape == (N, 3) and got["nactive"].shape == (N, S) and got["included"].shape == (N,)
        for i in range(4):
            assert np.array_equal(_bits(got["weight"][:, i].reshape((NR, N), order="F")), _bits(want["weight"][i])), i
        assert np.array_equal(_bits(got["fit"].T), _bits(want["fit"])) and np.array_equal(got["nactive"].T, want["nactive"])
        assert np.array_equal(got["included"], want["included"])
        if weights:
            assert got["weights"].shape == (NR * N, S)
            for s in range(S):
                assert np.array_equal(_bits(got["weights"][:, s].reshape((NR, N), order="F")), _bits(want["weights"][s])), s
        else:
            assert got["weights"] is None

    def call(end, n, u, ref, keep, steps, ms, ws):
        return R.call("C_bnmf_decompose", ptr, R.nil() if end is None else R.integer([end]), R.integer([n]), R.nil() if u is None else R.logical(u),
                      R.real_matrix(ref), R.nil() if keep is None else R.logical(keep), R.real([ms]), R.integer([steps, int(ws)]), R.integer(dims))

    want = e.decompose(7, cat, used=used, end_iter=12, keep=[1, 0, 1], n_steps=20, min_share=0.1, weights=True)
    assert want["n_used"] == 5 and np.isnan(want["cosine"][1]) and want["included"].tolist() == [5, 0, 5]
    same(R.take(call(12, 7, used, cat, [1, 0, 1], 20, 0.1, True)), want, True)
    # used = NULL, keep = NULL, no weights; end_iter = NULL is the current iteration
    lean = R.take(call(13, 5, None, cat, None, 20, 0.05, False))
    same(lean, e.decompose(5, cat, n_steps=20), False)
    now = R.take(call(None, 5, None, cat, None, 20, 0.05, False))
    at = R.take(R.call("C_bnmf_decompose_at", ptr, R.integer([13]), R.integer([5]), R.nil(), R.real_matrix(cat), R.nil(), R.real([0.05]), R.integer([20, 0]),
                       R.integer(dims)))
    assert np.array_equal(_bits(now["weight"]), _bits(lean["weight"])) and np.array_equal(_bits(now["fit"]), _bits(lean["fit"]))
    assert np.array_equal(_bits(at["weight"]), _bits(lean["weight"])) and np.array_equal(_bits(at["fit"]), _bits(lean["fit"]))
    # refusals arrive as R errors with the library's message, the PROTECT stack empty
    with pytest.raises(RError, match="used has 3 entries"):
        call(12, 7, [1, 1, 1], cat, None, 20, 0.05, False)
    with pytest.raises(RError, match="keep has 2 entries"):
        call(12, 7, None, cat, [1, 1], 20, 0.05, False)
    with pytest.raises(RError, match="not a multiple of K"):
        R.call("C_bnmf_decompose", ptr, R.integer([12]), R.integer([7]), R.nil(), R.real(np.ones(K + 1)), R.nil(), R.real([0.05]), R.integer([20, 0]),
               R.integer(dims))
    with pytest.raises(RError, match="are kept"):
        call(14, 7, None, cat, None, 20, 0.05, False)
    with pytest.raises(RError, match="at least 2"):
        call(12, 3, [0, 1, 0], cat, None, 20, 0.05, False)
    with pytest.raises(RError, match="n_steps"):
        call(12, 3, None, cat, None, 0, 0.05, False)
    with pytest.raises(RError, match="min_share"):
        call(12, 3, None, cat, None, 20, 1.0, False)
    cb = cat.copy(order="F"); cb[2, 3] = -1.0
    with pytest.raises(RError, match=r"reference_P\[2, 3\]"):
        call(12, 3, None, cb, None, 20, 0.05, False)
    assert R.L.rstub_protect_depth() == 0
    R.call("C_bnmf_destroy", ptr)
    R.release(ptr)
    e.close()
    assert R.L.rstub_violations() == v0
