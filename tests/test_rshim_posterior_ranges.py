"""The `.Call` routines of posterior inference on any recorded range and of the label-switching trace (C_bnmf_map_at,
C_bnmf_assign_at, C_bnmf_label_switching in r/bnmf_shim.c), compiled against the stand-in R runtime of tests/r_stub/ and run:
registered with their parameter counts and called by the R class (CPU); the same bits as the ctypes binding (GPU)."""
import os
import re

import numpy as np
import pytest

from rshim import RShim, ROOT

GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def R():
    if not os.path.exists(os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")):
        pytest.skip("libbnmf.so not built")
    return RShim()


def test_new_routines_are_registered_and_called_by_the_R_class(R):
    assert R.routines["C_bnmf_map_at"] == 5 and R.routines["C_bnmf_assign_at"] == 9 and R.routines["C_bnmf_label_switching"] == 4
    rsrc = open(os.path.join(ROOT, "r", "bayesNMF_hip.R")).read()
    called = set(re.findall(r'\.Call\("(C_bnmf_\w+)"', rsrc))
    assert {"C_bnmf_map_at", "C_bnmf_assign_at", "C_bnmf_label_switching"} <= called
    assert re.search(r"get_MAP = function\(end_iter = self\$state\$iter, n_samples = ", rsrc)
    assert "label_switching_df = function(reference_P, idx = \"all\")" in rsrc


def _create_args(R, M, N, window, seed, learning_rank=0, temperature=None):
    K, G = M.shape
    return (R.int_matrix(M), R.integer([K, G, N]), R.integer([0, 2, 0, learning_rank, 0, 0, window]),
            R.real(np.ones(1) if temperature is None else temperature), R.real([float(seed)]), R.integer([0]), R.integer([0]))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.gpu
def test_shim_ranges_and_label_switching_bit_identical_to_the_ctypes_binding(R):
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import IDS
    from bayesnmf_amd.setup import synth_counts, default_hyperprior_params, apply_hyperprior_params
    v0 = R.L.rstub_violations()
    K, G, N, W = 96, 30, 6, 200
    M, _, _ = synth_counts(K, G, 3, 7, mean_total=1500)
    temp = np.concatenate([np.zeros(3), 10.0 ** np.linspace(-6, 0, 40), np.ones(300)])
    ptr = R.call("C_bnmf_create", *_create_args(R, M, N, W, 9, learning_rank=1, temperature=temp))
    for k, v in default_hyperprior_params("gamma", M, N).items():
        R.call("C_bnmf_set_array", ptr, R.integer([IDS[k[0].upper() + k[1:]]]), R.real([float(v)]))
    e = Engine(M, N, prior="gamma", learning_rank=True, seed=9, window=W, temperature=temp)
    apply_hyperprior_params(e, "gamma", M, N)
    assert np.array_equal(_bits(R.take(R.call("C_bnmf_init", ptr))), _bits(e.init()))
    assert np.array_equal(_bits(R.take(R.call("C_bnmf_run", ptr, R.integer([150]), R.logical([False]))).T), _bits(e.run(150)))
    dims = [K, G, N]

    for ci in (0.9, 0.0):
        mp = R.take(R.call("C_bnmf_map_at", ptr, R.integer([100]), R.integer([40]), R.real([ci]), R.integer(dims)))
        ref = e.map(40, ci if ci > 0 else None, end_iter=100)
        assert list(mp) == ["P", "E", "A", "top_A", "P_lower", "P_upper", "E_lower", "E_upper", "used", "n_used", "n_patterns", "top_counts", "rmse", "kl"]
        for k in ("P", "E", "A", "P_lower", "P_upper", "E_lower", "E_upper"):
            assert (mp[k] is None) if ref[k] is None else np.array_equal(_bits(mp[k]), _bits(ref[k])), k
        assert mp["used"].dtype == bool and np.array_equal(mp["used"], ref["used"])
        assert mp["n_used"][0] == ref["n_used"] and mp["rmse"][0] == ref["rmse"] and mp["kl"][0] == ref["kl"]
        assert np.array_equal(mp["top_A"][:len(ref["top_A"])], ref["top_A"])

    cosmic = np.load(os.path.join(GOLD, "cosmic_v3.3.1_sbs.npz"))["P"]
    m = e.map(40, None, end_iter=100)
    keep = (m["A"].ravel() == 1).astype(np.int32)
    asg = R.take(R.call("C_bnmf_assign_at", ptr, R.integer([100]), R.integer([40]), R.logical(m["used"].astype(np.int32)), R.real_matrix(cosmic),
                        R.logical(keep), R.real_matrix(m["P"]), R.real([0.9]), R.integer(dims)))
    ra = e.assign(40, cosmic, used=m["used"].astype(np.int32), keep=keep, MAP_P=m["P"], credible_interval=0.9, end_iter=100)
    assert np.array_equal(_bits(asg["votes"]), _bits(ra["votes"]))
    assert np.array_equal(asg["assigned"], np.where(ra["assigned"] < 0, np.iinfo(np.int32).min, ra["assigned"] + 1))
    for a, b in (("MAP_cosine", "MAP_cosine"), ("lower", "lower_cosine"), ("upper", "upper_cosine")):
        assert np.array_equal(_bits(asg[a]), _bits(ra[b])), a

    iters = np.arange(2, 152, dtype=np.int32)
    for refP in (cosmic, m["P"][:, :3]):                                 # N <= R, and N > R ("None" = NA_integer_)
        ls = R.take(R.call("C_bnmf_label_switching", ptr, R.integer(iters), R.real_matrix(refP), R.integer(dims)))
        rl = e.label_switching(iters, refP)
        assert list(ls) == ["assigned", "cosine", "included"]
        assert ls["assigned"].shape == (N, len(iters))                   # one column per iteration
        assert np.array_equal(ls["assigned"].T, np.where(rl["assigned"] < 0, np.iinfo(np.int32).min, rl["assigned"] + 1))
        assert np.array_equal(_bits(ls["cosine"].T), _bits(rl["cosine"]))
        assert ls["included"].dtype == bool and np.array_equal(ls["included"].T, rl["included"])
    with pytest.raises(Exception, match="kept"):
        R.call("C_bnmf_label_switching", ptr, R.integer([1, 500]), R.real_matrix(cosmic), R.integer(dims))
    R.call("C_bnmf_destroy", ptr, keep_args=True)
    R.release(ptr); R.gc(); e.close()
    assert R.L.rstub_violations() == v0
