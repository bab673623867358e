"""CPU test: the planner still yields the geometries the fixed instantiations of k_zalloc_sort are built for (csrc/zalloc_sort.h ZSFix10k,
ZSFix2k; chosen in csrc/api.hip build_zsort).  A planner change that moves KP, GBc, the item format or the quads per item of the headline
shapes would route them to the dynamic form without any test failing: this one does."""
import ctypes as C

import numpy as np
import pytest

K, N, N_CU = 96, 20, 256
DATA_SEED = 20250218                       # bench.py: the headline's data; configuration 2 is seed + 2 (bench.py secondary_configs)
SWITCHES = ("BNMF_ZSORT", "BNMF_ZSSPREAD", "BNMF_ZSLDS", "BNMF_ZSW", "BNMF_ZSQMAX", "BNMF_ZSIT16", "BNMF_ZSPK", "BNMF_ZSFIXED")
# (KP, GBc, it16, qmax) of ZSFix10k and ZSFix2k
FIXED = {10000: (97, 40, 1, 64), 2000: (97, 8, 0, 16)}


def plan_desc(M, n_cu=N_CU, save_Z=False, n=N):
    """desc of bnmf_test_zsort_plan: ok, KP, GBc, blocks, W, qmax, it16, pk, shared, blocks without an own column, ..., threshold blocks"""
    from bayesnmf_amd.engine import lib
    L = lib()
    L.bnmf_test_zsort_plan.argtypes = [C.c_int] * 5 + [C.c_void_p, C.POINTER(C.c_longlong)] + [C.c_void_p] * 5
    M = np.asfortranarray(M, dtype=np.int32)
    d = (C.c_longlong * 14)()
    assert L.bnmf_test_zsort_plan(M.shape[0], M.shape[1], n, int(save_Z), n_cu, M.ctypes.data, d, None, None, None, None, None) == 0
    return [int(x) for x in d]


def takes_fixed_form(d, K_=K, N_=N):
    """what zsort_fixed_form (csrc/zalloc_sort.h) decides from a plan"""
    ok, KP, GBc, _, W, qmax, it16, pk, shared = d[:9]
    return bool(ok and pk and not shared and W == 14 and d[13] == 4 and K_ == K and N_ == N and (KP, GBc, it16, qmax) in FIXED.values())


@pytest.mark.parametrize("G,seed", [(10000, DATA_SEED), (2000, DATA_SEED + 2), (2000, DATA_SEED)])
def test_planner_yields_the_instantiated_geometry(G, seed, monkeypatch):
    from bayesnmf_amd.setup import synth_counts
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    M, _, _ = synth_counts(K, G, 8, seed)
    d = plan_desc(M)
    assert d[0] == 1, "the sorted schedule declined the shape"
    assert (d[1], d[2], d[6], d[5]) == FIXED[G], "(KP, GBc, it16, qmax)"
    assert d[3] == N_CU and d[4] == 14 and d[7] == 1 and d[8] == 0 and d[13] == 4, "256 blocks of 14 waves, packed tables, no shared column, four threshold blocks"
    assert takes_fixed_form(d)


def test_switch_is_not_a_planner_input(monkeypatch):
    """BNMF_ZSFIXED chooses between two instantiations of one kernel over the SAME schedule: the plan does not depend on it"""
    from bayesnmf_amd.setup import synth_counts
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    M, _, _ = synth_counts(K, 2000, 8, DATA_SEED + 2)
    d1 = plan_desc(M)
    monkeypatch.setenv("BNMF_ZSFIXED", "0")
    assert plan_desc(M) == d1
