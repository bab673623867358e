"""The Poisson sampler of the stream spec on the device (probe 8 of bnmf_test_sampler) and the posterior predictive checks of a
recorded range (bnmf_ppc / bnmf_ppc_at, csrc/ppc.h) against their restatement in Python floats (tests/ppc_ref.py, written from
DESIGN.md 4 and 14): every output bit for bit, no tolerance; then the equivalences and the refusals.

Every chain keeps a window of 8 samples and runs to iteration 13 (the rank-learning one to iteration 10, whose range then holds
iteration 3, where the tempered rank sweep excluded every factor), so the kept range wraps the ring of 9 slots.  The shapes are the smallest that
reach each path of the tiling: a partial row wave and a partial column group (70 x 9), two row chunks with the second nearly empty
(130 x 17), N = 20 (96 x 8), and N = 151, where the stage exceeds the LDS and the lanes read through the caches."""
import ctypes as C

import numpy as np
import pytest

import ppc_ref as R

pytestmark = pytest.mark.gpu

W, T_END = 8, 13
KEYS = {"key_1_0": (1, 0), "key_wide": (0x9E3779B97F4A7C15, 0x80000001)}      # tests/test_gpu_keys.py's
INFO = ("p_T1", "p_T2", "mean_T1_obs", "mean_T1_rep", "mean_T2_obs", "mean_T2_rep")
CELLS = ("mean_cell", "var_cell", "p_less_cell", "p_equal_cell", "pit")

# name: K, G, N, likelihood, prior, learning_rank, (end_iter, n_samples, used or None), key
CASES = {
    "p70_gaps": (70, 9, 3, "poisson", "gamma", False, (12, 7, [1, 0, 1, 1, 0, 1, 1]), "key_1_0"),       # wraps the ring; gaps in used
    "p130": (130, 17, 4, "poisson", "gamma", False, (13, 4, None), "key_wide"),                          # two row chunks
    "p96_sbfi": (96, 8, 20, "poisson", "gamma", True, (8, 6, None), "key_1_0"),                          # samples with A[n] = 0; one with A = 0
    "p_unstaged": (5, 3, 151, "poisson", "gamma", False, (13, 2, None), "key_1_0"),                      # the stage exceeds 160 KB
    "n70_real": (70, 9, 3, "normal", "exponential", False, (12, 7, [1, 1, 0, 1, 0, 1, 1]), "key_wide"),  # real-valued data
    "n130_int": (130, 17, 4, "normal", "truncnormal", False, (13, 3, None), "key_1_0"),                  # whole-number data
}


def _t_end(case):
    return 10 if case == "p96_sbfi" else T_END


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _data(case):
    K, G, N, lk, *_ = CASES[case]
    rng = np.random.default_rng(K * 1000 + G)
    M = rng.poisson(rng.gamma(0.6, 25.0, size=(K, G))).astype(np.int32)      # cell means on both sides of 10
    M[:, G // 2] = 0
    M[K // 3, :] = 0
    M[1, 1] = 1500
    if case == "n70_real":
        return np.asfortranarray(M * 0.37 + rng.normal(0.0, 0.5, size=(K, G)))
    return np.asfortranarray(M)


def _temps():
    return np.concatenate([np.zeros(3), 10.0 ** np.linspace(-6, 0, 60), np.ones(100)])


def _create(case):
    from bayesnmf_amd import Engine
    K, G, N, lk, prior, lr, _, key = CASES[case]
    seed, chain = KEYS[key]
    M = _data(case)
    return Engine(M, N, likelihood=lk, prior=prior, learning_rank=lr, seed=seed, chain_id=chain, window=W, temperature=_temps() if lr else None), M


def _fresh(case):
    from bayesnmf_amd.setup import apply_hyperprior_params
    e, M = _create(case)
    apply_hyperprior_params(e, CASES[case][4], M, CASES[case][2])
    row1 = e.init()
    return e, M, row1


def _reference(e, case, M, end, n, used):
    """ppc_ref on the samples bnmf_window returns for the range"""
    K, G, N, lk, _, _, _, key = CASES[case]
    first = end - n + 1
    back = e.iter - first + 1
    sel = np.arange(n) if used is None else np.where(np.asarray(used) == 1)[0]
    win = {nm: np.stack([e.window(nm, back)[i] for i in sel]) for nm in ("P", "E", "A") + (("sigmasq",) if lk == "normal" else ())}
    sig = win["sigmasq"].reshape(len(sel), G) if lk == "normal" else None
    seed, chain = KEYS[key]
    return R.ppc_reference(win["P"], win["E"], win["A"].reshape(len(sel), N), sig, M, lk, first + sel, seed, chain)


_RUNS = {}


def _run(case):
    """the chain at its last iteration, its metric rows, the device's checks of the case's range and the reference: made once per case"""
    if case in _RUNS:
        return _RUNS[case]
    e, M, row1 = _fresh(case)
    rows = np.vstack([row1[None, :], e.run(_t_end(case) - 1)])
    assert e.iter == _t_end(case)
    end, n, used = CASES[case][6]
    used = None if used is None else np.array(used, dtype=np.int32)
    dev = e.ppc(n, used=used, end_iter=end, pointwise=True)
    ref = _reference(e, case, M, end, n, used)
    _RUNS[case] = dict(e=e, M=M, rows=rows, end=end, n=n, used=used, dev=dev, ref=ref)
    return _RUNS[case]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for r in _RUNS.values():
        r["e"].close()
    _RUNS.clear()


def _same(a, b, pointwise=True):
    for k in INFO:
        assert _bits(a[k]) == _bits(b[k]), (k, a[k], b[k])
    assert a["n_used"] == b["n_used"] and a["n_tail_cells"] == b["n_tail_cells"]
    for k in ("col", "series") + (CELLS if pointwise else ()):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


@pytest.mark.parametrize("key", list(KEYS))
def test_probe_8_is_the_restated_sampler(key, oracle_lib):
    from bayesnmf_amd import engine as E
    seed, chain = KEYS[key]
    edge = [1e-6, 0.5, np.nextafter(10.0, 0.0), 10.0, np.nextafter(10.0, 20.0), 50.0, 1e3, 1e6, 1.6e7, 2.0 ** 24]
    lam = np.concatenate([edge, np.geomspace(1e-6, 2.0 ** 24, 190)])          # 200 values that straddle every branch
    lam3 = np.tile(lam, 3)                                                     # every value on three elements
    bad = 0
    for elem0, it in ((0, 1), (0x80000005, 0x90000000)):
        got = E.test_sampler("rpois", a=lam3, seed=seed, chain=chain, var=R.V_YREP, elem0=elem0, it=it)
        want, att = R.rpois_vec(lam3, seed=seed, chain=chain, var=R.V_YREP, elem0=elem0, it=it)
        ne = _bits(got) != _bits(want)
        print(f"rpois[{key}] elem0={elem0:#x} it={it:#x}: {int(ne.sum())} of {lam3.size} differ; attempts up to {att.max()}, "
              f"{int((att[lam3 >= 10.0] > 1).sum())} draws of the rejection branch took more than one")
        for i in np.where(ne)[0][:5]:
            print(f"    lam {lam3[i]!r}: device {got[i]!r} restatement {want[i]!r}")
        bad += int(ne.sum())
        assert (got >= 0).all() and (got == np.floor(got)).all()
    assert bad == 0


@pytest.mark.parametrize("case", list(CASES))
def test_every_output_is_the_restatement_bit_for_bit(case, oracle_lib):
    r = _run(case)
    K, G, N, lk, *_ = CASES[case]
    dev, ref = r["dev"], r["ref"]
    if lk == "poisson":
        lam = ref["lam"]
        print(f"ppc[{case}] lam: {int((lam < 10.0).sum())} below 10, {int((lam >= 10.0).sum())} from 10 on, {int((lam == 1e-6).sum())} clipped at 1e-6; "
              f"attempts up to {ref['attempts'].max()}")
        if case != "p_unstaged":
            assert (lam < 10.0).any() and (lam >= 10.0).any(), "the cell means do not fall on both sides of the sampler's threshold"
    if case == "p96_sbfi":
        A = np.stack(r["e"].window("A", _t_end(case) - (r["end"] - r["n"] + 1) + 1))[:r["n"]].reshape(r["n"], N)
        assert (A == 0).any(), "no used sample excludes a factor"
        assert (ref["lam"] == 1e-6).all(axis=0).any(), "no column and sample with every lam at the clip"
    bad = []
    for k in ("series", "col") + CELLS:
        ne = _bits(dev[k]) != _bits(ref[k])
        if ne.any():
            i = tuple(np.argwhere(ne)[0])
            print(f"ppc[{case}] {k}: {int(ne.sum())} of {ne.size} differ, first at {i}: device {np.asarray(dev[k])[i]!r} restatement {np.asarray(ref[k])[i]!r}")
            bad.append(k)
    for k in INFO + ("n_used", "n_tail_cells"):
        if not (dev[k] == ref[k]):
            print(f"ppc[{case}] {k}: device {dev[k]!r} restatement {ref[k]!r}")
            bad.append(k)
    print(f"ppc[{case}] S {dev['n_used']} p_T1 {dev['p_T1']:.2f} p_T2 {dev['p_T2']:.2f} tail cells {dev['n_tail_cells']} of {K * G}")
    assert not bad, bad


@pytest.mark.parametrize("case", ["p70_gaps", "p96_sbfi", "n70_real"])
def test_equivalent_calls_give_the_same_bits(case):
    r = _run(case)
    e, n, end, used = r["e"], r["n"], r["end"], r["used"]
    _same(r["dev"], e.ppc(n, used=used, end_iter=end, pointwise=True))                        # a second call
    _same(r["dev"], e.ppc(n, used=used, end_iter=end, pointwise=False), False)                # cell = NULL
    _same(e.ppc(5, pointwise=True), e.ppc(5, end_iter=e.iter, pointwise=True))                # bnmf_ppc is bnmf_ppc_at(iter)
    _same(e.ppc(5, pointwise=True), e.ppc(5, used=np.ones(5, dtype=np.int32), pointwise=True))   # NULL is all ones
    # col, cell and series all NULL: the info fields alone
    from bayesnmf_amd.engine import lib, BnmfPpcInfo
    info = BnmfPpcInfo()
    u = None if used is None else used.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib().bnmf_ppc_at(e._h, end, n, u, None, None, None, C.byref(info)) == 0
    for k in INFO + ("n_used", "n_tail_cells"):
        assert getattr(info, k) == r["dev"][k], k


@pytest.mark.parametrize("case", ["p70_gaps", "n70_real"])
def test_overlapping_ranges_share_the_replicates_of_their_iterations(case):
    """iterations 8..10 belong to the ranges 6..10 and 8..12: the same whole-matrix T of the data and of the replicate, per sample"""
    e = _run(case)["e"]
    a, b = e.ppc(5, end_iter=10), e.ppc(5, end_iter=12)
    assert np.array_equal(_bits(a["series"][:, 2:]), _bits(b["series"][:, :3]))
    assert not np.array_equal(_bits(a["series"][1, :2]), _bits(b["series"][1, 3:]))           # (other iterations, other replicates)
    # ... and one iteration, asked for with another used[]: the cell statistics of the pair (10, 12) from either range
    u1, u2 = np.array([0, 0, 0, 0, 1, 0, 1], dtype=np.int32), np.array([1, 0, 1], dtype=np.int32)
    _same(e.ppc(7, used=u1, end_iter=12, pointwise=True), e.ppc(3, used=u2, end_iter=12, pointwise=True))


@pytest.mark.parametrize("case", ["p70_gaps", "n130_int"])
def test_a_reopened_chain_gives_the_same_bits(case, tmp_path):
    r = _run(case)
    path = str(tmp_path / "state.bin")
    r["e"].save_state(path)
    c, _ = _create(case)
    assert c.load_state(path) == T_END
    _same(r["dev"], c.ppc(r["n"], used=r["used"], end_iter=r["end"], pointwise=True))
    c.close()


def test_refusals():
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import lib, BnmfPpcInfo, BnmfError
    from bayesnmf_amd.setup import apply_hyperprior_params
    r = _run("p70_gaps")
    e, M, L = r["e"], r["M"], lib()
    info = BnmfPpcInfo()
    ip = C.POINTER(C.c_int32)

    def err():
        msg = L.bnmf_last_error().decode()
        assert msg
        return msg
    assert L.bnmf_ppc(e._h, 5, None, None, None, None, None) == -1 and "null" in err()                     # BNMF_EINVAL
    assert L.bnmf_ppc_at(e._h, e.iter, 5, None, None, None, None, None) == -1 and "null" in err()
    u = np.ones(5, dtype=np.int32); u[3] = 2
    assert L.bnmf_ppc(e._h, 5, u.ctypes.data_as(ip), None, None, None, C.byref(info)) == -1 and "used[3] = 2" in err()
    u[3] = -1
    assert L.bnmf_ppc_at(e._h, e.iter, 5, u.ctypes.data_as(ip), None, None, None, C.byref(info)) == -1 and "used[3] = -1" in err()
    u = np.zeros(5, dtype=np.int32); u[3] = 1
    assert L.bnmf_ppc(e._h, 5, u.ctypes.data_as(ip), None, None, None, C.byref(info)) == -2 and "1 used sample" in err()   # BNMF_ESIZE
    assert L.bnmf_ppc(e._h, 1, None, None, None, None, C.byref(info)) == -2 and err()
    # the range rule of bnmf_map_at: iterations [max(1, iter - window + 1), iter]
    assert L.bnmf_ppc_at(e._h, e.iter + 1, 5, None, None, None, None, C.byref(info)) == -2 and "are kept" in err()
    assert L.bnmf_ppc_at(e._h, e.iter, W + 1, None, None, None, None, C.byref(info)) == -2 and "are kept" in err()
    assert L.bnmf_ppc_at(e._h, e.iter - W + 1, 3, None, None, None, None, C.byref(info)) == -2 and "are kept" in err()
    assert L.bnmf_ppc(e._h, W + 1, None, None, None, None, C.byref(info)) == -2 and err()
    with pytest.raises(BnmfError, match="used has 3 entries"):
        e.ppc(5, used=[1, 1, 1])
    # window = 0: BNMF_ESTATE
    z = Engine(M, 3, prior="gamma", seed=4, window=0)
    apply_hyperprior_params(z, "gamma", M, 3)
    z.init(); z.run(5)
    assert L.bnmf_ppc(z._h, 3, None, None, None, None, C.byref(info)) == -7 and "window = 0" in err()
    assert L.bnmf_ppc_at(z._h, z.iter, 3, None, None, None, None, C.byref(info)) == -7 and "window = 0" in err()
    z.close()
    assert L.bnmf_version() == 100
    # the handle is usable afterwards: the same bits as before the refusals
    _same(r["dev"], e.ppc(r["n"], used=r["used"], end_iter=r["end"], pointwise=True))


@pytest.mark.parametrize("case", ["p70_gaps", "p96_sbfi", "n70_real"])
def test_the_call_is_read_only_for_the_chain(case):
    """a chain that calls ppc mid-run continues with the bits of a twin that never did"""
    r = _run(case)
    b, _, row1 = _fresh(case)
    rows_b = np.vstack([row1[None, :], b.run(_t_end(case) - 1)])
    assert np.array_equal(_bits(rows_b), _bits(r["rows"]))
    more_a, more_b = r["e"].run(6), b.run(6)                                      # a called ppc at its last iteration, b never did
    assert np.array_equal(_bits(more_a), _bits(more_b))
    names = ("P", "E", "A") + (("sigmasq",) if CASES[case][3] == "normal" else ())
    for nm in names:
        assert np.array_equal(_bits(r["e"].get(nm)), _bits(b.get(nm))), nm
    b.close()
    _RUNS.pop(case)["e"].close()                                                  # (this case's chain has moved on)
