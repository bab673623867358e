"""The `.Call` routines of the silhouette stability (C_bnmf_stability / C_bnmf_stability_at in r/bnmf_shim.c), compiled against the
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
    for name in ("C_bnmf_stability", "C_bnmf_stability_at"):
        m = re.search(r"^SEXP %s\(([^)]*)\)\s*\{" % name, src, re.M)
        assert m and len([p for p in m.group(1).split(",") if p.strip()]) == 8, name
        assert R.routines[name] == 8
    rsrc = open(os.path.join(ROOT, "r", "bayesNMF_hip.R")).read()
    assert '.Call("C_bnmf_stability"' in rsrc and "get_stability = function(end_iter" in rsrc
    # get_relabelling's perm is N x S: the method transposes it (the GPU test below walks the same steps on the shim's result)
    assert "perm <- t(matrix(as.integer(perm), nrow = N))" in rsrc


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
    lab = np.stack([np.random.default_rng(s).permutation(N) for s in range(7)]).astype(np.int32)
    lab[3, 1] = -1
    ex = np.asfortranarray(np.random.default_rng(4).gamma(0.5, 1.0, size=(K, 5)))
    el = np.array([0, 2, 2, 1, 0], dtype=np.int32)
    dims = [K, G, N]

    def same(got, want):
        for k in ("n_used", "n_points", "n_extra", "n_left_out", "n_clusters", "min_stability_at"):
            assert got[k][0] == want[k], k
        assert int(got["n_negative"][0]) == want["n_negative"]
        for k in ("mean_silhouette", "min_stability"):
            assert _same_bits(got[k], np.array([want[k]])), k
        assert _same_bits(got["point"].T, want["point"]) and _same_bits(got["factor"].T, want["factor"]) and _same_bits(got["between"].T, want["between"])
        assert _same_bits(got["medoid"], want["medoid"]) and np.array_equal(np.asarray(got["medoid_at"]).astype(np.int64), want["medoid_at"])

    want = e.stability(7, labels=lab, used=used, end_iter=12, extra_P=ex, extra_label=el)
    got = R.take(R.call("C_bnmf_stability", ptr, R.integer([12]), R.integer([7]), R.logical(used), R.int_matrix(lab), R.real_matrix(ex), R.integer(el),
                        R.integer(dims)))
    assert want["n_used"] == 5 and want["n_extra"] == 5 and want["n_left_out"] == 1
    same(got, want)
    # used = NULL, labels = NULL, no extras
    lean = R.take(R.call("C_bnmf_stability", ptr, R.integer([13]), R.integer([5]), R.nil(), R.nil(), R.nil(), R.nil(), R.integer(dims)))
    same(lean, e.stability(5))
    now = R.take(R.call("C_bnmf_stability", ptr, R.nil(), R.integer([5]), R.nil(), R.nil(), R.nil(), R.nil(), R.integer(dims)))
    at = R.take(R.call("C_bnmf_stability_at", ptr, R.integer([13]), R.integer([5]), R.nil(), R.nil(), R.nil(), R.nil(), R.integer(dims)))
    assert _same_bits(now["point"], at["point"])
    # the steps of the R method get_stability(relabel = TRUE), S = 5 used samples of N = 3 factors: C_bnmf_relabel's perm is N x S
    # (1-based, NA = unmatched); t(matrix(as.integer(perm), nrow = N)) is S x N and goes into the used rows of an n_samples x N matrix
    piv = np.asfortranarray(e.get("P")[:, [2, 0, 1]])
    rl = R.take(R.call("C_bnmf_relabel", ptr, R.integer([12]), R.integer([7]), R.logical(used), R.real_matrix(piv), R.integer([10]), R.logical([False]),
                       R.integer(dims)))
    S = int(used.sum())
    assert rl["perm"].shape == (N, S) and S != N
    flat = rl["perm"].ravel(order="F")                                          # as.integer(perm)
    perm = flat.reshape((N, S), order="F").T                                    # t(matrix(., nrow = N))
    rlab = np.full((7, N), -1, dtype=np.int32)
    rlab[used == 1] = np.where(perm == np.iinfo(np.int32).min, -1, perm - 1)    # ifelse(is.na(perm), -1L, perm - 1L)
    wperm = e.relabel(7, used=used, end_iter=12, pivot_P=piv)["perm"]
    wlab = np.full((7, N), -1, dtype=np.int32)
    wlab[used == 1] = wperm
    assert np.array_equal(rlab, wlab) and (wperm != np.arange(N)).any()
    same(R.take(R.call("C_bnmf_stability", ptr, R.integer([12]), R.integer([7]), R.logical(used), R.int_matrix(rlab), R.nil(), R.nil(), R.integer(dims))),
         e.stability(7, labels=wlab, used=used, end_iter=12))
    # refusals arrive as R errors with the library's message, the PROTECT stack empty
    with pytest.raises(RError, match="used has 3 entries"):
        R.call("C_bnmf_stability", ptr, R.integer([12]), R.integer([7]), R.logical([1, 1, 1]), R.nil(), R.nil(), R.nil(), R.integer(dims))
    with pytest.raises(RError, match="labels has 3 entries"):
        R.call("C_bnmf_stability", ptr, R.integer([12]), R.integer([7]), R.nil(), R.integer([0, 1, 2]), R.nil(), R.nil(), R.integer(dims))
    with pytest.raises(RError, match="one label per extra column"):
        R.call("C_bnmf_stability", ptr, R.integer([12]), R.integer([7]), R.nil(), R.nil(), R.real_matrix(ex), R.integer([0, 1]), R.integer(dims))
    with pytest.raises(RError, match="are kept"):
        R.call("C_bnmf_stability", ptr, R.integer([14]), R.integer([7]), R.nil(), R.nil(), R.nil(), R.nil(), R.integer(dims))
    bad = lab.copy(); bad[2, 0] = 7
    with pytest.raises(RError, match=r"labels\[2\]\[0\] = 7"):
        R.call("C_bnmf_stability", ptr, R.integer([12]), R.integer([7]), R.nil(), R.int_matrix(bad), R.nil(), R.nil(), R.integer(dims))
    assert R.L.rstub_protect_depth() == 0
    R.call("C_bnmf_destroy", ptr)
    R.release(ptr)
    e.close()
    assert R.L.rstub_violations() == v0
