"""Signature attribution of a recorded range on the device (bnmf_attribution / bnmf_attribution_at, csrc/attribution.h) against its
numerical spec restated in numpy float64 (tests/attribution_ref.py, written from DESIGN.md 15): every output of every case bit for
bit, no tolerance — the operations are multiply, add, IEEE division and compare only; then the equivalences and the refusals.

Every case keeps window = 16 samples and runs to iteration 40, so the kept range wraps the ring; the range is the 12 samples that end
2 iterations before `iter`, with a `used` mask that has gaps (tests/test_gpu_waic.py's).  The shapes are the smallest that reach each
path of the tiling: K < 64 and a lone last column; a last pass of 32 rows; a second chunk of rows (scratch write, then add); N = 20, not
a multiple of the factor tile of 8; N = 151, where the stage exceeds the LDS and the lanes read through the caches; real-valued data
with negative cells; rings recorded by the MH sweep.

The rank-learning chain (seed 14; temperature 1 for 20 iterations, then 0 for 3 and a ramp from 1e-6) was rehearsed on the CPU
oracle: its A is all zero at iteration 31, a used sample, so every cell of that sample has c == 0, and every other used sample
excludes between 6 and 13 of the 20 factors."""
import ctypes as C

import numpy as np
import pytest

import attribution_ref as R

pytestmark = pytest.mark.gpu

W, T_END, N_RANGE = 16, 40, 12
USED = np.array([1, 1, 0, 1, 1, 1, 0, 0, 1, 1, 1, 1], dtype=np.int32)
ARRAYS = ("load", "series", "prob")
INFO = ("n_used", "n_present", "min_load", "total")

# name: K, G, N, likelihood, prior, MH, learning_rank, seed
CASES = {
    "pg_k8": (8, 7, 3, "poisson", "gamma", False, False, 4),              # K < 64; odd G: a lone last column
    "pg_k96": (96, 6, 5, "poisson", "gamma", False, False, 4),            # a last pass of 32 rows
    "pg_k130": (130, 5, 2, "poisson", "gamma", False, False, 4),          # a second chunk of rows: scratch write, then add
    "sbfi": (96, 8, 20, "poisson", "gamma", False, True, 14),             # three factor tiles, the last of 4; samples with A[n] = 0, one with A = 0
    "unstaged": (5, 3, 151, "poisson", "gamma", False, False, 4),         # the stage exceeds 160 KB
    "normal": (12, 10, 3, "normal", "exponential", False, False, 4),      # real-valued data, negative cells
    "ptn_mh": (96, 6, 5, "poisson", "truncnormal", True, False, 4),       # rings recorded by the MH sweep
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _data(case):
    from bayesnmf_amd.setup import synth_counts
    K, G, N, lk, *_ = CASES[case]
    if lk == "normal":
        rng = np.random.default_rng(11)
        return np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, 3)) @ rng.gamma(0.5, 1.0, size=(3, G)) + rng.normal(0.0, 0.5, size=(K, G)))   # small means: some cells below 0
    M, _, _ = synth_counts(K, G, min(3, N), 21, mean_total=1500)
    return M


def _temps():
    return np.concatenate([np.ones(20), np.zeros(3), 10.0 ** np.linspace(-6, 0, 60), np.ones(100)])


def _create(case):
    from bayesnmf_amd import Engine
    K, G, N, lk, prior, MH, lr, seed = CASES[case]
    M = _data(case)
    return Engine(M, N, likelihood=lk, prior=prior, MH=MH, learning_rank=lr, seed=seed, window=W, temperature=_temps() if lr else None), M


def _fresh(case):
    from bayesnmf_amd.setup import apply_hyperprior_params
    e, M = _create(case)
    apply_hyperprior_params(e, CASES[case][4], M, CASES[case][2])
    row1 = e.init()
    return e, M, row1


_RUNS = {}


def _run(case):
    """the chain at iteration 40, its metric rows, the device's attribution of the range and the restatement: made once per case"""
    if case in _RUNS:
        return _RUNS[case]
    K, G, N, lk, prior, MH, lr, _ = CASES[case]
    e, M, row1 = _fresh(case)
    rows = np.vstack([row1[None, :], e.run(T_END - 1, converged=MH)])
    assert e.iter == T_END
    end = T_END - 2
    first = end - N_RANGE + 1
    back = T_END - first + 1
    sel = np.where(USED == 1)[0]
    win = {nm: np.stack([e.window(nm, back)[i] for i in sel]) for nm in ("P", "E", "A")}
    samples = (win["P"], win["E"], win["A"].reshape(len(sel), N))
    ref = R.attribution_reference(*samples, M, lk, min_load=1.0)
    dev = e.attribution(N_RANGE, used=USED, end_iter=end, prob=True)
    _RUNS[case] = dict(e=e, M=M, rows=rows, end=end, first=first, samples=samples, ref=ref, dev=dev)
    return _RUNS[case]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for r in _RUNS.values():
        r["e"].close()
    _RUNS.clear()


def _differences(tag, a, b, prob=True):
    """the names of the outputs of a that are not b's, bit for bit (printed with the first place they differ)"""
    bad = []
    for k in ARRAYS if prob else ARRAYS[:2]:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape:
            print(f"attribution[{tag}] {k}: shapes {x.shape} and {y.shape}")
            bad.append(k)
            continue
        ne = _bits(x) != _bits(y)
        if ne.any():
            i = tuple(np.argwhere(ne)[0])
            print(f"attribution[{tag}] {k}: {int(ne.sum())} of {ne.size} differ, first at {i}: {x[i]!r} against {y[i]!r}")
            bad.append(k)
    for k in INFO:
        if _bits(float(a[k])) != _bits(float(b[k])):
            print(f"attribution[{tag}] {k}: {a[k]!r} against {b[k]!r}")
            bad.append(k)
    return bad


def _same(a, b, prob=True):
    assert not _differences("equivalence", a, b, prob)


@pytest.mark.parametrize("case", list(CASES))
def test_every_output_is_the_restatement_bit_for_bit(case, oracle_lib):
    r = _run(case)
    K, G, N, lk, *_ = CASES[case]
    dev, ref = r["dev"], r["ref"]
    A = r["samples"][2]
    print(f"attribution[{case}] S {dev['n_used']} total {dev['total']!r} (sum of the data {float(np.sum(r['M']))!r}) present {dev['n_present']} of {N * G}; "
          f"samples that exclude a factor {int((A == 0).any(axis=1).sum())}, cells with c == 0 {int((ref['c'] == 0).sum())}")
    if case == "sbfi":
        assert (A == 0).any(), "no used sample excludes a factor"
        assert (ref["c"] == 0).any(), "no (k, g, s) with c == 0"
    if case == "normal":
        assert (np.asarray(r["M"]) < 0).any(), "no negative cell"
    assert dev["n_used"] == int(USED.sum()) and dev["prob"].shape == (K, N, G) and dev["load"].shape == (4, N, G) and dev["series"].shape == (dev["n_used"], N)
    bad = _differences(case, dev, ref)
    # without prob: the kernel that keeps no per-cell sums, against the restatement too
    bad += _differences(case + ", no prob", r["e"].attribution(N_RANGE, used=USED, end_iter=r["end"], prob=False), ref, prob=False)
    assert not bad, bad


@pytest.mark.parametrize("case", ["pg_k130", "sbfi", "normal"])
def test_equivalent_calls_give_the_same_bits(case, monkeypatch):
    r = _run(case)
    e, end = r["e"], r["end"]
    _same(r["dev"], e.attribution(N_RANGE, used=USED, end_iter=end, prob=True))                     # a second call
    _same(r["dev"], e.attribution(N_RANGE, used=USED, end_iter=end, prob=False), False)             # prob = NULL
    _same(e.attribution(10, prob=True), e.attribution(10, end_iter=e.iter, prob=True))              # bnmf_attribution is bnmf_attribution_at(iter)
    _same(e.attribution(10, prob=True), e.attribution(10, used=np.ones(10, dtype=np.int32), prob=True))   # NULL is all ones
    _same(e.attribution(N_RANGE, end_iter=end, prob=True), e.attribution(N_RANGE, used=np.ones(N_RANGE, dtype=np.int32), end_iter=end, prob=True))
    for batch in ("1", "5"):                                                                         # 9 samples in 9 and in 2 batches
        monkeypatch.setenv("BNMF_ATTR_BATCH", batch)
        _same(r["dev"], e.attribution(N_RANGE, used=USED, end_iter=end, prob=True))
        _same(r["dev"], e.attribution(N_RANGE, used=USED, end_iter=end, prob=False), False)
    monkeypatch.delenv("BNMF_ATTR_BATCH")
    # load, prob and series all NULL: the info fields alone
    from bayesnmf_amd.engine import lib, BnmfAttrInfo
    info = BnmfAttrInfo()
    assert lib().bnmf_attribution_at(e._h, end, N_RANGE, USED.ctypes.data_as(C.POINTER(C.c_int32)), 1.0, None, None, None, C.byref(info)) == 0
    for k in INFO:
        assert getattr(info, k) == r["dev"][k], k
    # another min_load moves row 3 and n_present alone
    hi = e.attribution(N_RANGE, used=USED, end_iter=end, min_load=50.0)
    assert np.array_equal(_bits(hi["load"][:3]), _bits(r["dev"]["load"][:3])) and np.array_equal(_bits(hi["series"]), _bits(r["dev"]["series"]))
    a = R.attribution_reference(*r["samples"], r["M"], CASES[case][3], min_load=50.0, prob=False)
    assert np.array_equal(_bits(hi["p_present"]), _bits(a["p_present"])) and hi["n_present"] == a["n_present"] and hi["min_load"] == 50.0


@pytest.mark.parametrize("case", ["pg_k96", "normal"])
def test_a_reopened_chain_gives_the_same_bits(case, tmp_path):
    r = _run(case)
    path = str(tmp_path / "state.bin")
    r["e"].save_state(path)
    c, _ = _create(case)
    assert c.load_state(path) == T_END
    _same(r["dev"], c.attribution(N_RANGE, used=USED, end_iter=r["end"], prob=True))
    c.close()


def test_refusals():
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import lib, BnmfAttrInfo, BnmfError
    from bayesnmf_amd.setup import apply_hyperprior_params
    r = _run("pg_k8")
    e, M, L = r["e"], r["M"], lib()
    info = BnmfAttrInfo()
    ip = C.POINTER(C.c_int32)

    def err():
        msg = L.bnmf_last_error().decode()
        assert msg
        return msg
    assert L.bnmf_attribution(e._h, 10, None, 1.0, None, None, None, None) == -1 and "null" in err()                     # BNMF_EINVAL
    assert L.bnmf_attribution_at(e._h, e.iter, 10, None, 1.0, None, None, None, None) == -1 and "null" in err()
    u = np.ones(10, dtype=np.int32); u[6] = 2
    assert L.bnmf_attribution(e._h, 10, u.ctypes.data_as(ip), 1.0, None, None, None, C.byref(info)) == -1 and "used[6] = 2" in err()
    u[6] = -1
    assert L.bnmf_attribution_at(e._h, e.iter, 10, u.ctypes.data_as(ip), 1.0, None, None, None, C.byref(info)) == -1 and "used[6] = -1" in err()
    for bad in (float("nan"), float("inf"), -float("inf"), -0.5):
        assert L.bnmf_attribution(e._h, 10, None, bad, None, None, None, C.byref(info)) == -1 and "min_load" in err()
        assert L.bnmf_attribution_at(e._h, e.iter, 10, None, bad, None, None, None, C.byref(info)) == -1 and "min_load" in err()
    u = np.zeros(10, dtype=np.int32); u[3] = 1
    assert L.bnmf_attribution(e._h, 10, u.ctypes.data_as(ip), 1.0, None, None, None, C.byref(info)) == -2 and "1 used sample" in err()   # BNMF_ESIZE
    assert L.bnmf_attribution(e._h, 1, None, 1.0, None, None, None, C.byref(info)) == -2 and err()
    # the range rule of bnmf_waic_at: iterations [max(1, iter - window + 1), iter]
    assert L.bnmf_attribution_at(e._h, e.iter + 1, 5, None, 1.0, None, None, None, C.byref(info)) == -2 and "are kept" in err()
    assert L.bnmf_attribution_at(e._h, e.iter, W + 1, None, 1.0, None, None, None, C.byref(info)) == -2 and "are kept" in err()
    assert L.bnmf_attribution_at(e._h, e.iter - W + 1, 3, None, 1.0, None, None, None, C.byref(info)) == -2 and "are kept" in err()
    assert L.bnmf_attribution(e._h, W + 1, None, 1.0, None, None, None, C.byref(info)) == -2 and err()
    with pytest.raises(BnmfError, match="used has 3 entries"):
        e.attribution(10, used=[1, 1, 1])
    # window = 0: BNMF_ESTATE
    z = Engine(M, 3, prior="gamma", seed=4, window=0)
    apply_hyperprior_params(z, "gamma", M, 3)
    z.init(); z.run(5)
    assert L.bnmf_attribution(z._h, 3, None, 1.0, None, None, None, C.byref(info)) == -7 and "window = 0" in err()
    assert L.bnmf_attribution_at(z._h, z.iter, 3, None, 1.0, None, None, None, C.byref(info)) == -7 and "window = 0" in err()
    z.close()
    assert L.bnmf_version() == 100
    assert L.bnmf_attribution(e._h, 10, None, 0.0, None, None, None, C.byref(info)) == 0          # min_load = 0 is allowed: every load counts
    assert info.n_present == CASES["pg_k8"][2] * CASES["pg_k8"][1]
    # the handle is usable afterwards: the same bits as before the refusals
    _same(r["dev"], e.attribution(N_RANGE, used=USED, end_iter=r["end"], prob=True))


@pytest.mark.parametrize("case", ["pg_k96", "ptn_mh", "sbfi"])
def test_the_call_is_read_only_for_the_chain(case):
    """a chain that calls attribution mid-run continues with the bits of a twin that never did"""
    r = _run(case)
    MH = CASES[case][5]
    b, _, row1 = _fresh(case)
    rows_b = np.vstack([row1[None, :], b.run(T_END - 1, converged=MH)])
    assert np.array_equal(_bits(rows_b), _bits(r["rows"]))
    more_a, more_b = r["e"].run(10, converged=MH), b.run(10, converged=MH)       # a called attribution at iteration 40, b never did
    assert np.array_equal(_bits(more_a), _bits(more_b))
    for nm in ("P", "E", "A"):
        assert np.array_equal(_bits(r["e"].get(nm)), _bits(b.get(nm))), nm
    b.close()
    _RUNS.pop(case)["e"].close()                                                 # (this case's chain has moved on)
