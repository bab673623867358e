"""Host side of a chain's state in a file (bnmf_save_state / bnmf_load_state / bnmf_state_info): the symbols are declared and
exported, bnmf_state_info refuses what is not a state file without a device, load_sampler says what is missing, the R class calls the
three routines.  No GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bnmf_save_state", "bnmf_load_state", "bnmf_state_info")


def test_new_symbols_are_declared_exported_and_bound():
    from bayesnmf_amd import engine
    hdr = open(os.path.join(ROOT, "include", "bnmf.h")).read()
    for name in NEW:
        assert re.search(r"^int\s+%s\(" % name, hdr, re.M), name
        assert name in engine.ABI_SYMBOLS
        assert hasattr(engine.lib(), name)                   # exported by libbnmf.so
    assert engine.lib().bnmf_version() == 100                # the file format has a version of its own
    assert callable(engine.state_info) and hasattr(engine.Engine, "save_state") and hasattr(engine.Engine, "load_state")


@pytest.mark.parametrize("what", ["missing", "empty", "random", "header_only"])
def test_state_info_refuses_what_is_not_a_state_file(tmp_path, what):
    from bayesnmf_amd.engine import BnmfError, state_info
    p = tmp_path / "f.bin"
    if what == "empty":
        p.write_bytes(b"")
    elif what == "random":
        p.write_bytes(np.random.default_rng(1).integers(0, 256, 4096, dtype=np.uint8).tobytes())
    elif what == "header_only":
        p.write_bytes(b"BNMFSTAT" + bytes(200))
    with pytest.raises(BnmfError) as ei:
        state_info(str(p))
    assert ei.value.code == -1                               # BNMF_EINVAL
    msg = str(ei.value)
    assert "bnmf_state_info" in msg and str(p) in msg
    assert {"missing": "cannot open", "empty": "shorter than its header", "random": "bad magic", "header_only": "version"}[what] in msg


def test_load_sampler_without_engine_state_is_a_clear_error(tmp_path):
    from bayesnmf_amd.sampler import load_sampler
    (tmp_path / "sampler.pkl").write_bytes(b"")
    with pytest.raises(FileNotFoundError, match="engine_state.bin.*save_engine_state=True"):
        load_sampler(str(tmp_path))


def test_sampler_refuses_save_engine_state_with_an_engine_that_cannot_save(tmp_path):
    from bayesnmf_amd.sampler import bayesNMF_sampler

    class NoSave:                                            # an engine_factory's engine without save_state
        def __init__(self, M, N, **kw):
            pass

        def set(self, name, value):
            pass

        def close(self):
            pass
    M = np.ones((4, 5), dtype=np.int32)
    with pytest.raises(ValueError, match="save_engine_state"):
        bayesNMF_sampler(M, 2, prior="gamma", output_dir=str(tmp_path / "x"), engine_factory=NoSave, save_engine_state=True)


def test_R_class_calls_the_three_routines():
    rsrc = open(os.path.join(ROOT, "r", "bayesNMF_hip.R")).read()
    called = set(re.findall(r'\.Call\("(C_bnmf_\w+)"', rsrc))
    assert {"C_bnmf_save_state", "C_bnmf_load_state", "C_bnmf_state_info"} <= called
    assert "load_bayesNMF_hip <- function(output_dir, device = 0L)" in rsrc
    assert "super$save_object()" in rsrc and "save_engine_state = FALSE" in rsrc
