"""Real-valued data for the Normal likelihood (bnmf_create_f64) — what can be checked without a GPU: the entry point and its R
binding exist, every refusal of bad data comes from the host before any device call, and the Python layers hand Normal data on
as float64, untouched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rshim import RShim, RError, RViolation, ROOT

EINVAL, ENODEVICE = -1, -4


def _lib():
    from bayesnmf_amd.engine import lib
    return lib()


def _cfg(K, G, N, likelihood, prior):
    from bayesnmf_amd.engine import BnmfConfig, LIKELIHOOD, PRIOR
    return BnmfConfig(K, G, N, LIKELIHOOD[likelihood], PRIOR[prior], 0, 0, 0, 0, 0, 1, 0, 0, None, 0)


def _create_f64(M, N=2, likelihood="normal", prior="exponential"):
    """rc and message of bnmf_create_f64; a handle it made (a GPU is visible) is destroyed again"""
    L = _lib()
    M = np.asfortranarray(M, dtype=np.float64)
    cfg = _cfg(M.shape[0], M.shape[1], N, likelihood, prior)
    h = C.c_void_p()
    rc = L.bnmf_create_f64(C.byref(cfg), M.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h))
    msg = L.bnmf_last_error().decode()
    if rc == 0:
        L.bnmf_destroy(h)
    return rc, msg


def _no_device():
    from bayesnmf_amd.engine import device_count
    return device_count() == 0


def test_library_exports_the_real_valued_entry_point():
    from bayesnmf_amd import engine
    assert "bnmf_create_f64" in engine.ABI_SYMBOLS
    assert hasattr(_lib(), "bnmf_create_f64")
    hdr = open(os.path.join(ROOT, "include", "bnmf.h")).read()
    assert re.search(r"^int bnmf_create_f64\(const bnmf_config\* cfg, const double\* M_colmajor, bnmf_handle\*\* out\);", hdr, re.M)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_normal_refuses_non_finite_values_naming_the_cell(bad):
    M = np.random.default_rng(0).normal(0.5, 1.0, size=(6, 5))
    M[4, 3] = bad
    rc, msg = _create_f64(M)
    assert rc == EINVAL, msg
    assert "M[4, 3]" in msg and "not finite" in msg
    M[1, 0] = np.nan                                   # the FIRST bad cell in column-major order is named
    rc, msg = _create_f64(M)
    assert rc == EINVAL and "M[1, 0]" in msg


@pytest.mark.parametrize("bad,what", [(2.5, "non-integer"), (-1.0, "non-integer"), (-0.25, "non-integer"), (2.0 ** 31, "non-integer"),
                                      (np.nan, "non-integer"), (np.inf, "non-integer")])
def test_poisson_refuses_what_is_not_a_count(bad, what):
    M = np.random.default_rng(1).poisson(4.0, size=(6, 5)).astype(np.float64)
    M[2, 4] = bad
    rc, msg = _create_f64(M, prior="gamma", likelihood="poisson")
    assert rc == EINVAL, msg
    assert what in msg and "M[2, 4]" in msg


def test_refusals_of_data_come_before_the_device():
    """Valid data go on to the device checks (no GPU: BNMF_ENODEVICE; a GPU: a handle); bad data never get there."""
    rng = np.random.default_rng(2)
    real = rng.normal(0.2, 1.5, size=(8, 7))
    assert (real < 0).any() and (real != np.floor(real)).any()
    counts = rng.poisson(3.0, size=(8, 7)).astype(np.float64)
    counts[0, 0] = 2.0 ** 31 - 1                       # the largest count still converts
    expect = ENODEVICE if _no_device() else 0
    assert _create_f64(real)[0] == expect              # negative and fractional values are Normal data
    assert _create_f64(counts, likelihood="poisson", prior="gamma")[0] == expect
    assert _create_f64(real, likelihood="poisson", prior="gamma")[0] == EINVAL
    # the arguments bnmf_create refuses, refused alike
    assert _create_f64(real, N=0)[0] == EINVAL
    assert _create_f64(real, N=1025)[0] == EINVAL
    L = _lib()
    cfg = _cfg(8, 7, 2, "normal", "exponential")
    assert L.bnmf_create_f64(C.byref(cfg), None, C.byref(C.c_void_p())) == EINVAL


def test_bnmf_create_keeps_its_order_of_refusals():
    """bnmf_create (int32) answers as before: BNMF_ENODEVICE without a GPU, else BNMF_EINVAL for a negative count, whatever the
    likelihood."""
    from bayesnmf_amd.engine import BnmfConfig, LIKELIHOOD, PRIOR
    L = _lib()
    M = np.asfortranarray(-np.ones((4, 3), dtype=np.int32))
    for lk, pr in (("poisson", "gamma"), ("normal", "exponential")):
        cfg = BnmfConfig(4, 3, 2, LIKELIHOOD[lk], PRIOR[pr], 0, 0, 0, 0, 0, 1, 0, 0, None, 0)
        rc = L.bnmf_create(C.byref(cfg), M.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(C.c_void_p()))
        assert rc == (ENODEVICE if _no_device() else EINVAL), lk
        if rc == EINVAL:
            assert "negative count" in L.bnmf_last_error().decode()


def test_engine_sends_normal_data_as_float64():
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import BnmfError
    M = np.random.default_rng(3).normal(0.0, 1.0, size=(5, 4))
    M[0, 0] = np.nan
    with pytest.raises(BnmfError) as ei:                 # the NaN reached the library: the data were not cast to int32
        Engine(M, 2, likelihood="normal", prior="exponential")
    assert ei.value.code == EINVAL and "M[0, 0]" in str(ei.value)


class _Sent(Exception):
    pass


def _spy(seen):
    def factory(M, N, **kw):
        seen.append((M, N, kw))
        raise _Sent()
    return factory


def test_sampler_hands_normal_data_on_unchanged(tmp_path):
    """bayesNMF_sampler with likelihood = "normal" gives the engine the real data, float64, bit for bit (it used to get
    int32(trunc(x)))."""
    from bayesnmf_amd.sampler import bayesNMF_sampler
    rng = np.random.default_rng(4)
    x_real = rng.normal(0.3, 1.2, size=(12, 9))
    assert (x_real < 0).any()
    seen = []
    with pytest.raises(_Sent):
        bayesNMF_sampler(x_real, 3, likelihood="normal", prior="exponential", output_dir=str(tmp_path / "n"), engine_factory=_spy(seen))
    M = seen[0][0]
    assert M.dtype == np.float64 and M.shape == x_real.shape
    assert np.array_equal(M.view(np.uint64), x_real.view(np.uint64))
    # Poisson keeps its counts as int32
    counts = rng.poisson(3.0, size=(12, 9))
    with pytest.raises(_Sent):
        bayesNMF_sampler(counts, 3, likelihood="poisson", prior="gamma", MH=False, output_dir=str(tmp_path / "p"), engine_factory=_spy(seen))
    assert seen[1][0].dtype == np.int32 and np.array_equal(seen[1][0], counts)


def test_multichain_hands_normal_data_on_unchanged(tmp_path):
    from bayesnmf_amd.multichain import run_chains
    x_real = np.random.default_rng(5).normal(0.1, 1.0, size=(6, 5))
    seen = []
    with pytest.raises(_Sent):
        run_chains(x_real, 2, n_chains=2, devices=[0], likelihood="normal", prior="truncnormal", output_dir=str(tmp_path / "mc"),
                   engine_factory=_spy(seen))
    assert seen and all(s[0].dtype == np.float64 and np.array_equal(s[0], x_real) for s in seen)


# ---- the R binding, through the stand-in R runtime
@pytest.fixture(scope="module")
def R():
    _lib()                                              # (raises when libbnmf.so has not been built)
    return RShim()


def _args(R, data, likelihood, prior, N=2):
    K, G = data.shape
    mat = R.real_matrix(data) if data.dtype == np.float64 else R.int_matrix(data)
    return (mat, R.integer([K, G, N]), R.integer([likelihood, prior, 0, 0, 0, 0, 0]), R.real(np.ones(1)), R.real([11.0]),
            R.integer([0]), R.integer([0]))


def test_shim_registers_the_real_valued_create(R):
    assert R.routines["C_bnmf_create_f64"] == 7
    assert R.routines["C_bnmf_create"] == 7
    rsrc = open(os.path.join(ROOT, "r", "bayesNMF_hip.R")).read()
    assert '.Call("C_bnmf_create_f64", self$data' in rsrc
    assert 'storage.mode(self$data) <- "double"' in rsrc


def test_shim_reads_a_real_matrix(R):
    """C_bnmf_create_f64 takes a REALSXP: the library sees its values (its refusal names the cell), and an integer matrix is an
    API violation the stand-in names rather than a silent reinterpretation."""
    x = np.random.default_rng(6).normal(0.0, 1.0, size=(5, 4))
    x[3, 2] = np.inf
    with pytest.raises(RError, match=r"M\[3, 2\]"):
        R.call("C_bnmf_create_f64", *_args(R, x, 1, 1))
    y = np.full((5, 4), 2.5)
    with pytest.raises(RError, match="non-integer count"):
        R.call("C_bnmf_create_f64", *_args(R, y, 0, 2))
    with pytest.raises(RViolation, match=r"REAL\(\) applied to a integer"):
        R.call("C_bnmf_create_f64", *_args(R, np.ones((5, 4), dtype=np.int32), 1, 1))
    ok = np.random.default_rng(7).normal(0.0, 1.0, size=(5, 4))
    if _no_device():
        with pytest.raises(RError, match="(?i)device|gpu|hip"):
            R.call("C_bnmf_create_f64", *_args(R, ok, 1, 1))
    else:
        ptr = R.call("C_bnmf_create_f64", *_args(R, ok, 1, 1))
        R.call("C_bnmf_destroy", ptr, keep_args=True)
        R.release(ptr)
    R.gc()
    assert R.L.rstub_live_objects() == 0
