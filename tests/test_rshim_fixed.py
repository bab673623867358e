"""The `.Call` routines of fixed columns of P (C_bnmf_set_fixed, C_bnmf_get_fixed in r/bnmf_shim.c), compiled against the stand-in R
runtime of tests/r_stub/: registered, bad arguments refused through Rf_error before the handle is touched (CPU); a fixed chain driven
through the shim gives the bits of the ctypes route (GPU)."""
import os

import numpy as np
import pytest

from rshim import RShim, RError, ROOT


@pytest.fixture(scope="module")
def R():
    if not os.path.exists(os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")):
        pytest.skip("libbnmf.so not built")
    return RShim()


def test_routines_are_registered(R):
    assert R.routines["C_bnmf_set_fixed"] == 3 and R.routines["C_bnmf_get_fixed"] == 3


def test_bad_arguments_are_R_errors(R):
    NA = np.iinfo(np.int32).min
    with pytest.raises(RError, match="holds NA .entry 2."):
        R.call("C_bnmf_set_fixed", R.nil(), R.integer([0]), R.integer([1, NA, 0]))
    with pytest.raises(RError, match="id must be one integer"):
        R.call("C_bnmf_set_fixed", R.nil(), R.integer([0, 1]), R.integer([1, 0]))
    with pytest.raises(RError, match="is not a number of columns"):
        R.call("C_bnmf_get_fixed", R.nil(), R.integer([0]), R.real([-1.0]))
    with pytest.raises(RError, match="is not a number of columns"):
        R.call("C_bnmf_get_fixed", R.nil(), R.integer([0]), R.real([float("nan")]))
    with pytest.raises(RError, match="one number each"):
        R.call("C_bnmf_get_fixed", R.nil(), R.integer([0]), R.real([3.0, 4.0]))
    assert R.L.rstub_protect_depth() == 0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.gpu
def test_shim_route_gives_the_bits_of_the_ctypes_route(R):
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import IDS
    from bayesnmf_amd.setup import synth_counts, default_hyperprior_params, apply_hyperprior_params
    v0 = R.L.rstub_violations()
    K, G, N, W = 96, 40, 5, 30
    M, _, _ = synth_counts(K, G, 3, 7, mean_total=1500)
    P0 = np.asfortranarray(np.random.default_rng(3).gamma(1.0, 0.05, size=(K, N)))
    mask = np.array([1, 0, 1, 1, 0], dtype=np.int32)
    ptr = R.call("C_bnmf_create", R.int_matrix(M), R.integer([K, G, N]), R.integer([0, 2, 0, 0, 0, 0, W]), R.real(np.ones(1)), R.real([9.0]),
                 R.integer([0]), R.integer([0]))
    for k, v in default_hyperprior_params("gamma", M, N).items():
        R.call("C_bnmf_set_array", ptr, R.integer([IDS[k[0].upper() + k[1:]]]), R.real([float(v)]))
    R.call("C_bnmf_set_array", ptr, R.integer([IDS["P"]]), R.real(P0.ravel(order="F")))
    with pytest.raises(RError, match="out of scope"):
        R.call("C_bnmf_set_fixed", ptr, R.integer([IDS["E"]]), R.integer(mask))
    with pytest.raises(RError, match="neither 0 nor 1"):
        R.call("C_bnmf_set_fixed", ptr, R.integer([IDS["P"]]), R.integer([1, 0, 3, 0, 0]))
    R.call("C_bnmf_set_fixed", ptr, R.integer([IDS["P"]]), R.integer(mask))
    assert np.array_equal(R.take(R.call("C_bnmf_get_fixed", ptr, R.integer([IDS["P"]]), R.real([float(N)]))), mask)
    e = Engine(M, N, prior="gamma", seed=9, window=W, temperature=np.ones(1))
    apply_hyperprior_params(e, "gamma", M, N)
    e.set("P", P0); e.set_fixed("P", mask)
    r1 = R.take(R.call("C_bnmf_init", ptr))
    assert np.array_equal(_bits(r1), _bits(e.init()))
    a = R.take(R.call("C_bnmf_run", ptr, R.integer([30]), R.logical([False]))).T
    assert np.array_equal(_bits(a), _bits(e.run(30)))
    for nm in ("P", "E", "Alpha_p", "Beta_e"):
        n = int(np.prod(e.get(nm).shape))
        got = R.take(R.call("C_bnmf_get_array", ptr, R.integer([IDS[nm]]), R.real([float(n)])))
        assert np.array_equal(_bits(got), _bits(e.get(nm).ravel(order="F"))), nm
    assert np.array_equal(_bits(e.get("P")[:, [0, 2, 3]]), _bits(P0[:, [0, 2, 3]]))
    with pytest.raises(RError, match="initialised, loaded or run"):
        R.call("C_bnmf_set_fixed", ptr, R.integer([IDS["P"]]), R.integer(mask))
    R.call("C_bnmf_destroy", ptr)
    R.release(ptr)
    e.close()
    assert R.L.rstub_violations() == v0
