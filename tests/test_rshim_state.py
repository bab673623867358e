"""The `.Call` routines of a chain's state in a file (C_bnmf_save_state, C_bnmf_load_state, C_bnmf_state_info in r/bnmf_shim.c),
compiled against the stand-in R runtime of tests/r_stub/ and run: registered, refusing a bad path through Rf_error (CPU); the file the
shim writes is the file ctypes writes, and a handle loaded through the shim continues bit for bit (GPU)."""
import ctypes as C
import os

import numpy as np
import pytest

from rshim import RShim, RError, ROOT


@pytest.fixture(scope="module")
def R():
    if not os.path.exists(os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")):
        pytest.skip("libbnmf.so not built")
    r = RShim()
    r.L.Rf_mkString.restype, r.L.Rf_mkString.argtypes = C.c_void_p, [C.c_char_p]
    return r


def _str(R, s):
    return R.L.Rf_mkString(os.fsencode(s))


def test_routines_are_registered(R):
    assert R.routines["C_bnmf_save_state"] == 3 and R.routines["C_bnmf_load_state"] == 2 and R.routines["C_bnmf_state_info"] == 1


def test_bad_path_is_an_R_error(R, tmp_path):
    with pytest.raises(RError, match="bnmf_state_info: cannot open"):
        R.call("C_bnmf_state_info", _str(R, str(tmp_path / "none.bin")))
    (tmp_path / "junk.bin").write_bytes(b"not a state file" * 20)
    with pytest.raises(RError, match="bad magic"):
        R.call("C_bnmf_state_info", _str(R, str(tmp_path / "junk.bin")))
    assert R.L.rstub_protect_depth() == 0


def _create_args(R, M, N, window, seed):
    K, G = M.shape
    return (R.int_matrix(M), R.integer([K, G, N]), R.integer([0, 2, 0, 0, 0, 0, window]), R.real(np.ones(1)), R.real([float(seed)]),
            R.integer([0]), R.integer([0]))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.gpu
def test_shim_file_is_the_ctypes_file_and_a_shim_load_continues(R, tmp_path):
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import IDS, state_info
    from bayesnmf_amd.setup import synth_counts, default_hyperprior_params, apply_hyperprior_params
    v0 = R.L.rstub_violations()
    K, G, N, W = 96, 40, 5, 30
    M, _, _ = synth_counts(K, G, 3, 7, mean_total=1500)
    ptr = R.call("C_bnmf_create", *_create_args(R, M, N, W, 9))
    for k, v in default_hyperprior_params("gamma", M, N).items():
        R.call("C_bnmf_set_array", ptr, R.integer([IDS[k[0].upper() + k[1:]]]), R.real([float(v)]))
    e = Engine(M, N, prior="gamma", seed=9, window=W, temperature=np.ones(1))   # the shim passes a schedule of one 1.0
    apply_hyperprior_params(e, "gamma", M, N)
    R.take(R.call("C_bnmf_init", ptr)); e.init()
    R.take(R.call("C_bnmf_run", ptr, R.integer([45]), R.logical([False]))); e.run(45)
    ps, pc = str(tmp_path / "shim.bin"), str(tmp_path / "ctypes.bin")
    nbytes = R.take(R.call("C_bnmf_save_state", ptr, _str(R, ps), R.integer([0])))
    e.save_state(pc)
    assert open(ps, "rb").read() == open(pc, "rb").read() and nbytes[0] == os.path.getsize(ps)
    info = R.take(R.call("C_bnmf_state_info", _str(R, ps)))
    assert list(info["dims"]) == [K, G, N] and info["last_iter"][0] == 46 and info["n_records"][0] == 1
    assert state_info(ps)["last_iter"] == 46
    # a fresh handle through the shim loads the ctypes file and continues as the ctypes engine
    p2 = R.call("C_bnmf_create", *_create_args(R, M, N, W, 9))
    assert R.take(R.call("C_bnmf_load_state", p2, _str(R, pc)))[0] == 46
    with pytest.raises(RError, match="already run"):
        R.call("C_bnmf_load_state", p2, _str(R, pc))
    a = R.take(R.call("C_bnmf_run", p2, R.integer([25]), R.logical([False]))).T
    assert np.array_equal(_bits(a), _bits(e.run(25)))
    for nm in ("P", "E", "Alpha_e"):
        n = int(np.prod(e.get(nm).shape))
        got = R.take(R.call("C_bnmf_get_array", p2, R.integer([IDS[nm]]), R.real([float(n)])))
        assert np.array_equal(_bits(got), _bits(e.get(nm).ravel(order="F"))), nm
    for p in (ptr, p2):
        R.call("C_bnmf_destroy", p)
        R.release(p)
    e.close()
    assert R.L.rstub_violations() == v0
