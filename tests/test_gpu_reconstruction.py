"""Reconstruction quality per tumour over a recorded range on the device (bnmf_reconstruction / bnmf_reconstruction_at,
csrc/reconstruction.h) against the numerical spec restated in numpy float64 (tests/reconstruction_ref.py, written from DESIGN.md 23):
every output and every info field of every case bit for bit, NaN compared as NaN, no tolerance — the operations are + - * /, sqrt,
|.|, comparisons and integer counts only; then the equivalences and the refusals.

Every case keeps window = 16 samples and runs to iteration 40, so the kept range wraps the ring; the range is the 12 samples that end
2 iterations before `iter`, with a `used` mask that has gaps (tests/test_gpu_contrast.py's recipe).  The shapes are the smallest that
reach each path: G = 70 (not a multiple of 64) and G = 264 (two workgroups) with K = 8; K = 96 with N = 3 / 5, 12, 20 and 30 for the
register forms of 8, 16, 24 and 32 factors and N = 40 for the tiled form (5 tiles), each with x staged in the LDS and read through the caches; the rank-learning chain of
test_gpu_attribution (samples with A[n] = 0, one with A all zero: the drop of an excluded factor is exactly +0.0 and cos exactly 0.0,
no NaN); a data matrix with one all-zero column; real-valued data with negative cells; rings recorded by the MH sweep.

Permuting the tumours permutes `tumour` and `drop`: the rings cannot be written from outside and a chain on permuted data draws other
samples, so on the device this is held through the restatement (every tumour's bits are the restatement's wherever it sits: lanes,
waves and workgroups differ between G = 70 and G = 264), and the restatement's own invariance is pinned in
tests/test_reconstruction_host.py."""
import ctypes as C

import numpy as np
import pytest

import reconstruction_ref as R

pytestmark = pytest.mark.gpu

W, T_END, N_RANGE = 16, 40, 12
USED = np.array([1, 1, 0, 1, 1, 1, 0, 0, 1, 1, 1, 1], dtype=np.int32)
ARRAYS = ("tumour", "drop", "series", "signature")
INFO = ("n_used", "n_undefined", "n_poor", "n_needed", "min_cosine", "min_drop", "worst_cosine", "worst_at")
MIN_COS, MIN_DROP = 0.9, 0.01

# name: K, G, N, likelihood, prior, MH, learning_rank, seed
CASES = {
    "g70": (8, 70, 3, "poisson", "gamma", False, False, 4),                # the register form of 8
    "g264": (8, 264, 3, "poisson", "gamma", False, False, 4),              # two workgroups
    "k96n5": (96, 70, 5, "poisson", "gamma", False, False, 4),
    "n12": (96, 70, 12, "poisson", "gamma", False, False, 4),              # the register form of 16
    "n20": (96, 70, 20, "poisson", "gamma", False, False, 4),              # ... of 24
    "n30": (96, 70, 30, "poisson", "gamma", False, False, 4),              # ... of 32
    "n40": (96, 70, 40, "poisson", "gamma", False, False, 4),              # past the register forms: the tiled form, 5 tiles
    "sbfi": (96, 8, 20, "poisson", "gamma", False, True, 14),              # samples with A[n] = 0, one with A = 0
    "zerocol": (8, 70, 3, "poisson", "gamma", False, False, 5),            # one all-zero tumour
    "normal": (12, 10, 3, "normal", "exponential", False, False, 4),       # real-valued data, negative cells
    "ptn_mh": (96, 6, 5, "poisson", "truncnormal", True, False, 4),        # rings recorded by the MH sweep
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
    if case == "zerocol":
        M = M.copy()
        M[:, 37] = 0
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
    """the chain at iteration 40, its metric rows, the used samples of the range, the device's result and the restatement: once per case"""
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
    ref = R.reconstruction_reference(*samples, M, min_cosine=MIN_COS, min_drop=MIN_DROP)
    dev = e.reconstruction(N_RANGE, used=USED, end_iter=end, min_cosine=MIN_COS, min_drop=MIN_DROP)
    _RUNS[case] = dict(e=e, M=M, rows=rows, end=end, samples=samples, ref=ref, dev=dev)
    return _RUNS[case]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for r in _RUNS.values():
        r["e"].close()
    _RUNS.clear()


def _differences(tag, a, b, arrays=ARRAYS):
    """the names of the outputs of a that are not b's, bit for bit with NaN equal to NaN (printed with the first place they differ)"""
    bad = []
    for k in arrays:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape:
            print(f"reconstruction[{tag}] {k}: shapes {x.shape} and {y.shape}")
            bad.append(k)
            continue
        nx, ny = np.isnan(x), np.isnan(y)
        ne = (nx != ny) | (~nx & ~ny & (_bits(x).reshape(x.shape) != _bits(y).reshape(y.shape)))
        if ne.any():
            i = tuple(np.argwhere(ne)[0])
            print(f"reconstruction[{tag}] {k}: {int(ne.sum())} of {ne.size} differ, first at {i}: {x[i]!r} against {y[i]!r}")
            bad.append(k)
    for k in INFO:
        fa, fb = float(a[k]), float(b[k])
        if not ((np.isnan(fa) and np.isnan(fb)) or _bits(fa) == _bits(fb)):
            print(f"reconstruction[{tag}] {k}: {a[k]!r} against {b[k]!r}")
            bad.append(k)
    return bad


def _same(a, b, arrays=ARRAYS):
    assert not _differences("equivalence", a, b, arrays)


@pytest.mark.parametrize("case", list(CASES))
def test_every_output_is_the_restatement_bit_for_bit(case, monkeypatch):
    r = _run(case)
    K, G, N, lk, *_ = CASES[case]
    dev, ref, e = r["dev"], r["ref"], r["e"]
    A = r["samples"][2]
    S = int(USED.sum())
    print(f"reconstruction[{case}] S {dev['n_used']} undefined {dev['n_undefined']} poor {dev['n_poor']} needed {dev['n_needed']} worst {dev['worst_cosine']!r} at "
          f"{dev['worst_at']}; samples that exclude a factor {int((A == 0).any(axis=1).sum())}, series {dev['series'].round(4).tolist()}")
    assert dev["n_used"] == S and dev["tumour"].shape == (6, G) and dev["drop"].shape == (4, N, G) and dev["series"].shape == (S,) and dev["signature"].shape == (3, N)
    kw = dict(used=USED, end_iter=r["end"], min_cosine=MIN_COS, min_drop=MIN_DROP)
    bad = _differences(case, dev, ref)
    if case == "sbfi":
        assert (A == 0).any() and (A == 0).all(axis=1).any(), "no used sample without a factor"
        s0 = int(np.where((A == 0).all(axis=1))[0][0])
        assert (ref["cos"][s0] == 0).all() and not np.isnan(dev["tumour"]).any() and not np.isnan(dev["drop"]).any() and not np.isnan(dev["series"]).any()
        assert dev["series"][s0] == 0.0 and (dev["tumour"][2] == 0.0).all()                       # the sample with no factor: cos exactly 0.0
        never = (A == 0).all(axis=0)
        assert (ref["drops"][A == 0] == 0).all() and not np.signbit(ref["drops"][A == 0]).any()
        if never.any():
            assert (dev["drop"][0][never] == 0).all() and not np.signbit(dev["drop"][0][never]).any() and (dev["drop"][1][never] == 0).all()
    if case == "zerocol":
        assert dev["n_undefined"] == 1 and np.isnan(dev["tumour"][[0, 1, 2, 5], 37]).all() and np.isnan(dev["drop"][:, :, 37]).all()
        assert int(np.isnan(dev["tumour"]).sum()) == 4 and int(np.isnan(dev["drop"]).sum()) == 4 * N and dev["worst_at"] != 37
    if case == "normal":
        assert (np.asarray(r["M"]) < 0).any(), "no negative cell"
    # the other form of the kernel, x read through the caches instead of staged in the LDS, and other batch sizes: the same bits
    for name, val in (("BNMF_REC_FORM", "1"), ("BNMF_REC_STAGE", "0"), ("BNMF_REC_BATCH", "1"), ("BNMF_REC_BATCH", "5")):
        monkeypatch.setenv(name, val)
        bad += _differences(f"{case}, {name}={val}", e.reconstruction(N_RANGE, **kw), ref)
        monkeypatch.delenv(name)
    monkeypatch.setenv("BNMF_REC_FORM", "1")
    monkeypatch.setenv("BNMF_REC_STAGE", "0")
    monkeypatch.setenv("BNMF_REC_BATCH", "4")
    bad += _differences(f"{case}, tiled, unstaged, batches of 4", e.reconstruction(N_RANGE, **kw), ref)
    for name in ("BNMF_REC_FORM", "BNMF_REC_STAGE", "BNMF_REC_BATCH"):
        monkeypatch.delenv(name)
    # other thresholds: every count 1, every count 0
    for mc, md in ((-2.0, -2.0), (2.0, 2.0)):
        d = e.reconstruction(N_RANGE, used=USED, end_iter=r["end"], min_cosine=mc, min_drop=md)
        bad += _differences(f"{case}, min_cosine {mc:g}, min_drop {md:g}", d, R.reconstruction_reference(*r["samples"], r["M"], min_cosine=mc, min_drop=md))
        live = ~np.isnan(d["tumour"][0])
        assert (d["tumour"][5][live] == (1.0 if mc < 0 else 0.0)).all() and d["n_needed"] == (N * int(live.sum()) if md < 0 else 0)
    assert not bad, bad


@pytest.mark.parametrize("case", ["g264", "sbfi", "normal"])
def test_equivalent_calls_give_the_same_bits(case):
    r = _run(case)
    e, end = r["e"], r["end"]
    kw = dict(min_cosine=MIN_COS, min_drop=MIN_DROP)
    _same(r["dev"], e.reconstruction(N_RANGE, used=USED, end_iter=end, **kw))                       # a second call
    _same(e.reconstruction(10, **kw), e.reconstruction(10, end_iter=e.iter, **kw))                  # bnmf_reconstruction is bnmf_reconstruction_at(iter)
    _same(e.reconstruction(10, **kw), e.reconstruction_at(e.iter, 10, used=np.ones(10, dtype=np.int32), **kw))   # NULL is all ones
    # each output NULL in turn, then all of them: the others and the info fields are the same
    from bayesnmf_amd.engine import lib, BnmfReconstructionInfo
    L, dp, ip = lib(), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    K, G, N = CASES[case][:3]
    S = int(USED.sum())
    for skip in ARRAYS + ("all",):
        bufs = dict(tumour=np.full((6, G), -7.0), drop=np.full((4, G, N), -7.0), series=np.full(S, -7.0), signature=np.full((3, N), -7.0))
        ptr = {k: (None if skip in (k, "all") else v.ctypes.data_as(dp)) for k, v in bufs.items()}
        info = BnmfReconstructionInfo()
        assert L.bnmf_reconstruction_at(e._h, end, N_RANGE, USED.ctypes.data_as(ip), MIN_COS, MIN_DROP, ptr["tumour"], ptr["drop"], ptr["series"], ptr["signature"],
                                        C.byref(info)) == 0
        got = dict(tumour=bufs["tumour"], drop=bufs["drop"].transpose(0, 2, 1), series=bufs["series"], signature=bufs["signature"],
                   **{k: getattr(info, k) for k in INFO})
        for k in ARRAYS:
            if skip in (k, "all"):
                assert (bufs[k] == -7).all(), k                                                       # (not written)
        _same(got, r["dev"], tuple(k for k in ARRAYS if skip not in (k, "all")))


@pytest.mark.parametrize("case", ["k96n5", "normal"])
def test_a_reopened_chain_gives_the_same_bits(case, tmp_path):
    r = _run(case)
    path = str(tmp_path / "state.bin")
    r["e"].save_state(path)
    c, _ = _create(case)
    assert c.load_state(path) == T_END
    _same(r["dev"], c.reconstruction(N_RANGE, used=USED, end_iter=r["end"], min_cosine=MIN_COS, min_drop=MIN_DROP))
    c.close()


def test_refusals():
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import lib, BnmfReconstructionInfo, BnmfError
    from bayesnmf_amd.setup import apply_hyperprior_params
    r = _run("g70")
    e, M, L = r["e"], r["M"], lib()
    info = BnmfReconstructionInfo()
    ip = C.POINTER(C.c_int32)

    def err():
        msg = L.bnmf_last_error().decode()
        assert msg
        return msg

    def call(n=10, used=None, mc=0.9, md=0.01, inf=info, at=None, h=None):
        u = None if used is None else used.ctypes.data_as(ip)
        i = None if inf is None else C.byref(inf)
        h = e._h if h is None else h
        if at is None:
            return L.bnmf_reconstruction(h, n, u, mc, md, None, None, None, None, i)
        return L.bnmf_reconstruction_at(h, at, n, u, mc, md, None, None, None, None, i)

    for at in (None, e.iter):
        assert call(inf=None, at=at) == -1 and "null" in err()                                       # BNMF_EINVAL
        u = np.ones(10, dtype=np.int32); u[6] = 2
        assert call(used=u, at=at) == -1 and "used[6] = 2" in err()
        u[6] = -1
        assert call(used=u, at=at) == -1 and "used[6] = -1" in err()
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert call(mc=bad, at=at) == -1 and "min_cosine" in err()
            assert call(md=bad, at=at) == -1 and "min_drop" in err()
        u = np.zeros(10, dtype=np.int32); u[3] = 1
        assert call(used=u, at=at) == -2 and "1 used sample" in err()                                # BNMF_ESIZE
    assert call(n=1) == -2 and err()
    assert call(n=W + 1) == -2 and err()
    # the range rule of bnmf_attribution_at: iterations [max(1, iter - window + 1), iter]
    assert call(n=5, at=e.iter + 1) == -2 and "are kept" in err()
    assert call(n=W + 1, at=e.iter) == -2 and "are kept" in err()
    assert call(n=3, at=e.iter - W + 1) == -2 and "are kept" in err()
    with pytest.raises(BnmfError, match="used has 3 entries"):
        e.reconstruction(10, used=[1, 1, 1])
    # window = 0: BNMF_ESTATE
    z = Engine(M, 3, prior="gamma", seed=4, window=0)
    apply_hyperprior_params(z, "gamma", M, 3)
    z.init(); z.run(5)
    assert call(n=3, h=z._h) == -7 and "window = 0" in err()
    assert call(n=3, at=z.iter, h=z._h) == -7 and "window = 0" in err()
    z.close()
    assert L.bnmf_version() == 100
    assert call(mc=-1.0, md=0.0) == 0 and info.n_used == 10 and info.n_poor == 0                     # any finite threshold is allowed
    # the handle is usable afterwards: the same bits as before the refusals
    _same(r["dev"], e.reconstruction(N_RANGE, used=USED, end_iter=r["end"], min_cosine=MIN_COS, min_drop=MIN_DROP))


@pytest.mark.parametrize("case", ["g70", "ptn_mh", "sbfi"])
def test_the_call_is_read_only_for_the_chain(case):
    """a chain that calls reconstruction mid-run continues with the bits of a twin that never did"""
    r = _run(case)
    MH = CASES[case][5]
    b, _, row1 = _fresh(case)
    rows_b = np.vstack([row1[None, :], b.run(T_END - 1, converged=MH)])
    assert np.array_equal(_bits(rows_b), _bits(r["rows"]))
    more_a, more_b = r["e"].run(10, converged=MH), b.run(10, converged=MH)       # a called reconstruction at iteration 40, b never did
    assert np.array_equal(_bits(more_a), _bits(more_b))
    for nm in ("P", "E", "A"):
        assert np.array_equal(_bits(r["e"].get(nm)), _bits(b.get(nm))), nm
    b.close()
    _RUNS.pop(case)["e"].close()                                                  # (this chain has moved on)
