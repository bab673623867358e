"""Decomposition of the recorded signatures into a reference catalogue on the device (bnmf_decompose / bnmf_decompose_at,
csrc/decompose.h) against the numerical spec restated in numpy float64 (tests/decompose_ref.py, written from DESIGN.md 18): every
output and every info field of every case bit for bit, no tolerance — the operations are multiply, add, IEEE division, square root
and compare only; then the equivalences and the refusals.

Every case keeps window = 16 samples and runs to iteration 40, so the kept range wraps the ring; the range is the 12 samples that end
2 iterations before `iter`, with a `used` mask that has gaps (tests/test_gpu_project.py's); n_steps = 25 (and 25 more after the
pruning), min_share = 0.05.  The shapes are the smallest that reach each path: w and g in registers (R = 4, a tile of 8 with 4 idle
places); the 79 COSMIC columns with w and g in LDS columns (the catalogue fits beside them when staging is asked for); the rank-learning chain of
tests/test_gpu_attribution.py (several factors excluded per sample, and one used sample with A = 0); R = 128 with K = 130, where the
catalogue does not fit beside the columns; R = 33, one reference past the register form, with N = 40 so that 9 samples are 360
problems in 6 waves; rings recorded by the MH sweep; a Normal-likelihood chain (only P and A are read).

NaN: IEEE 754 leaves the sign and payload of a generated NaN to the implementation, so a NaN is compared as "a NaN" (one canonical
pattern); every other value by its 64 bits."""
import ctypes as C
import os

import numpy as np
import pytest

import decompose_ref as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, T_END, N_RANGE, STEPS, MIN_SHARE = 16, 40, 12, 25, 0.05
USED = np.array([1, 1, 0, 1, 1, 1, 0, 0, 1, 1, 1, 1], dtype=np.int32)
ARRAYS = ("weight", "fit", "nactive", "included", "weights")
INFO = ("n_used", "n_steps", "R", "n_present", "min_share", "max_rel_change", "min_cosine", "min_cosine_at")

# name: K, G, N, likelihood, prior, MH, learning_rank, seed, R (0 = the COSMIC fixture's 79 columns)
CASES = {
    "reg": (8, 7, 3, "poisson", "gamma", False, False, 4, 4),                # w, g in registers; one partial wave
    "cosmic": (96, 6, 5, "poisson", "gamma", False, False, 4, 0),            # LDS columns; the catalogue fits beside them
    "sbfi": (96, 8, 20, "poisson", "gamma", False, True, 14, 0),             # samples with A[n] = 0, one with A = 0
    "max_r": (130, 5, 2, "poisson", "gamma", False, False, 4, 128),          # the largest R; the catalogue is never staged
    "lds33": (12, 5, 40, "poisson", "gamma", False, False, 4, 33),           # one reference past the register form; 6 waves
    "ptn_mh": (96, 6, 5, "poisson", "truncnormal", True, False, 4, 6),       # rings recorded by the MH sweep
    "normal": (24, 6, 3, "normal", "exponential", False, False, 4, 5),       # the Normal likelihood
}


def _bits(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = np.uint64(0x7FF8000000000000)
    return b


def _catalogue(K, R):
    if R == 0:
        return np.asfortranarray(np.load(os.path.join(ROOT, "tests", "golden", "cosmic_v3.3.1_sbs.npz"))["P"], dtype=np.float64)
    ref = np.random.default_rng(100 + R).gamma(0.4, 1.0, size=(K, R))
    ref[0, :] = 0.0                                                  # a row of zeros
    ref[:, R - 1] *= 1000.0                                          # a column on another scale: normalised away
    return np.asfortranarray(ref)


def _temps():
    return np.concatenate([np.ones(20), np.zeros(3), 10.0 ** np.linspace(-6, 0, 60), np.ones(100)])


def _fresh(case):
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    K, G, N, lik, prior, MH, lr, seed, _ = CASES[case]
    M, _, _ = synth_counts(K, G, min(3, N), 21, mean_total=1500)
    data = np.asfortranarray(M, dtype=np.float64) if lik == "normal" else M
    e = Engine(data, N, likelihood=lik, prior=prior, MH=MH, learning_rank=lr, seed=seed, window=W, temperature=_temps() if lr else None)
    apply_hyperprior_params(e, prior, M, N)
    row1 = e.init()
    return e, row1


_RUNS = {}


def _run(case):
    """the chain at iteration 40, its metric rows, the device's decomposition and the restatement: made once per case"""
    if case in _RUNS:
        return _RUNS[case]
    K, G, N, lik, prior, MH, lr, _, R = CASES[case]
    e, row1 = _fresh(case)
    rows = np.vstack([row1[None, :], e.run(T_END - 1, converged=MH)])
    assert e.iter == T_END
    end = T_END - 2
    back = T_END - (end - N_RANGE + 1) + 1
    sel = np.where(USED == 1)[0]
    win = {nm: np.stack([e.window(nm, back)[i] for i in sel]) for nm in ("P", "A")}
    samples = (win["P"], win["A"].reshape(len(sel), N))
    cat = _catalogue(K, R)
    ref = D.decompose_reference(*samples, cat, STEPS, min_share=MIN_SHARE)
    dev = e.decompose(N_RANGE, cat, used=USED, end_iter=end, n_steps=STEPS, min_share=MIN_SHARE, weights=True)
    _RUNS[case] = dict(e=e, rows=rows, end=end, samples=samples, cat=cat, ref=ref, dev=dev)
    return _RUNS[case]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for r in _RUNS.values():
        r["e"].close()
    _RUNS.clear()


def _differences(tag, a, b, arrays=ARRAYS, info=INFO):
    """the names of the outputs of a that are not b's, bit for bit (printed with the first place they differ)"""
    bad = []
    for k in arrays:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape:
            print(f"decompose[{tag}] {k}: shapes {x.shape} and {y.shape}")
            bad.append(k)
            continue
        ne = _bits(x) != _bits(y)
        if ne.any():
            i = tuple(np.argwhere(ne)[0])
            print(f"decompose[{tag}] {k}: {int(ne.sum())} of {ne.size} differ, first at {i}: {x[i]!r} against {y[i]!r}")
            bad.append(k)
    for k in info:
        if _bits(float(a[k])) != _bits(float(b[k])):
            print(f"decompose[{tag}] {k}: {a[k]!r} against {b[k]!r}")
            bad.append(k)
    return bad


def _same(a, b, arrays=ARRAYS, info=INFO):
    assert not _differences("equivalence", a, b, arrays, info)


@pytest.mark.parametrize("case", list(CASES))
def test_every_output_is_the_restatement_bit_for_bit(case):
    r = _run(case)
    K, G, N = CASES[case][:3]
    dev, ref = r["dev"], r["ref"]
    R = r["cat"].shape[1]
    part = ref["part"]
    print(f"decompose[{case}] S {dev['n_used']} R {R} present {dev['n_present']} of {R * N}; max_rel_change {dev['max_rel_change']!r} "
          f"min_cosine {dev['min_cosine']!r} at {dev['min_cosine_at']}; nactive {int(dev['nactive'].min())}..{int(dev['nactive'].max())}; "
          f"factors taking part per sample {part.sum(axis=1).tolist()}")
    if case == "sbfi":
        assert (part.sum(axis=1) == 0).any(), "no used sample with A = 0"
        assert ((part.sum(axis=1) > 0) & (part.sum(axis=1) < N)).any(), "no used sample excludes only some factors"
        s0 = int(np.where(part.sum(axis=1) == 0)[0][0])
        assert (dev["weights"][s0] == 0).all() and (dev["nactive"][s0] == 0).all() and np.isnan(dev["cosine"]).all()
        assert (dev["included"] < dev["n_used"]).all()
    else:
        assert part.all() and (dev["included"] == dev["n_used"]).all()
    assert dev["n_used"] == int(USED.sum()) and dev["R"] == R and dev["weight"].shape == (4, R, N) and dev["fit"].shape == (3, N)
    assert dev["nactive"].shape == (dev["n_used"], N) and dev["included"].shape == (N,) and dev["weights"].shape == (dev["n_used"], R, N)
    bad = _differences(case, dev, ref)
    assert not bad, bad
    # the pruning did something, and what it dropped is +0.0
    assert (dev["nactive"][part] >= 1).all() and (dev["nactive"] <= R).all()
    assert ((dev["weights"] != 0).sum(axis=1) <= dev["nactive"]).all()
    assert not np.signbit(dev["weights"]).any()


@pytest.mark.parametrize("case", ["reg", "cosmic", "sbfi", "lds33", "max_r"])
def test_equivalent_calls_give_the_same_bits(case, monkeypatch):
    r = _run(case)
    e, end, cat = r["e"], r["end"], r["cat"]
    N, R = CASES[case][2], cat.shape[1]
    kw = dict(used=USED, end_iter=end, n_steps=STEPS, min_share=MIN_SHARE, weights=True)
    _same(r["dev"], e.decompose(N_RANGE, cat, **kw))                                                  # a second call
    _same(e.decompose(10, cat, n_steps=3, weights=True), e.decompose(10, cat, end_iter=e.iter, n_steps=3, weights=True))   # bnmf_decompose is bnmf_decompose_at(iter)
    _same(e.decompose(10, cat, n_steps=3), e.decompose(10, cat, used=np.ones(10, dtype=np.int32), keep=np.ones(N, dtype=np.int32), n_steps=3), ARRAYS[:4])   # NULL is all ones
    for batch in ("1", "5"):                                                                          # 9 samples in 9 and in 2 batches
        monkeypatch.setenv("BNMF_DEC_BATCH", batch)
        _same(r["dev"], e.decompose(N_RANGE, cat, **kw))
    monkeypatch.delenv("BNMF_DEC_BATCH")
    for stage in ("0", "1"):                                                                          # the catalogue through the caches, staged in the LDS
        monkeypatch.setenv("BNMF_DEC_STAGE", stage)
        _same(r["dev"], e.decompose(N_RANGE, cat, **kw))
    monkeypatch.delenv("BNMF_DEC_STAGE")
    # a keep[] subset: the kept factors keep their bits, the others are as a factor that takes no part
    keep = (np.arange(N) % 3 != 1).astype(np.int32)
    k = e.decompose(N_RANGE, cat, keep=keep, **kw)
    on, off = keep == 1, keep == 0
    assert np.array_equal(_bits(k["weights"][:, :, on]), _bits(r["dev"]["weights"][:, :, on])) and np.array_equal(_bits(k["weight"][:, :, on]), _bits(r["dev"]["weight"][:, :, on]))
    assert np.array_equal(_bits(k["fit"][:, on]), _bits(r["dev"]["fit"][:, on])) and np.array_equal(k["nactive"][:, on], r["dev"]["nactive"][:, on])
    assert np.array_equal(k["included"][on], r["dev"]["included"][on])
    assert (k["weights"][:, :, off] == 0).all() and (k["weight"][:, :, off] == 0).all() and (k["nactive"][:, off] == 0).all() and (k["included"][off] == 0).all()
    assert np.isnan(k["cosine"][off]).all() and (k["fit"][1:, off] == 0).all()
    # min_share = 0: no pruning, one stage
    z = e.decompose(N_RANGE, cat, used=USED, end_iter=end, n_steps=STEPS, min_share=0.0, weights=True)
    took = z["nactive"] > 0
    assert (z["nactive"][took] == R).all() and z["min_share"] == 0.0 and np.array_equal(took, r["dev"]["nactive"] > 0)
    assert np.array_equal(z["p_present"], (z["weights"] >= 0.0).mean(axis=0)) and z["n_present"] == R * N
    if case in ("reg", "lds33"):
        assert not _differences(case + " min_share 0", z, D.decompose_reference(*r["samples"], cat, STEPS, min_share=0.0))
    # each output NULL in turn, and all of them: the others and the info fields keep their bits
    from bayesnmf_amd.engine import lib, BnmfDecomposeInfo
    S = r["dev"]["n_used"]
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    flat = np.ascontiguousarray(cat.ravel(order="F"))
    for null in ([0], [1], [2], [3], [4], [0, 1, 2, 3, 4]):
        bufs = [np.empty((4, R * N)), np.empty((3, N)), np.empty((S, N), dtype=np.int32), np.empty(N, dtype=np.int32), np.empty((S, R * N))]
        ptrs = [None if i in null else b.ctypes.data_as(ip if b.dtype == np.int32 else dp) for i, b in enumerate(bufs)]
        info = BnmfDecomposeInfo()
        assert lib().bnmf_decompose_at(e._h, end, N_RANGE, USED.ctypes.data_as(ip), flat.ctypes.data_as(dp), R, None, STEPS, MIN_SHARE, *ptrs, C.byref(info)) == 0
        for k_ in INFO:
            assert _bits(float(getattr(info, k_))) == _bits(float(r["dev"][k_])), k_
        got = dict(weight=np.stack([row.reshape((R, N), order="F") for row in bufs[0]]), fit=bufs[1], nactive=bufs[2], included=bufs[3],
                   weights=np.stack([row.reshape((R, N), order="F") for row in bufs[4]]))
        _same(got, r["dev"], [a for i, a in enumerate(ARRAYS) if i not in null], ())


def test_identical_samples_have_variance_zero():
    """every column of P fixed: all samples share one P, so every sample's weights are the same bits and the variance row is 0.0"""
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    K, G, N, R = 24, 6, 3, 5
    M, _, _ = synth_counts(K, G, N, 21, mean_total=1500)
    e = Engine(M, N, likelihood="poisson", prior="gamma", seed=4, window=W)
    apply_hyperprior_params(e, "gamma", M, N)
    e.set("P", np.asfortranarray(np.random.default_rng(3).gamma(1.0, 1.0, size=(K, N))))
    e.set_fixed("P", np.ones(N, dtype=np.int32))
    e.init(); e.run(9)
    r = e.decompose(8, _catalogue(K, R), n_steps=STEPS, weights=True)
    assert (r["weights"][0] > 0).any()
    for s in range(1, 8):
        assert np.array_equal(_bits(r["weights"][s]), _bits(r["weights"][0])), s
    assert np.array_equal(_bits(r["weight_var"]), _bits(np.zeros((R, N)))) and np.array_equal(_bits(r["weight_mean"]), _bits(r["weights"][0]))
    e.close()


def test_refusals():
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import lib, BnmfDecomposeInfo, BnmfError
    from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
    r = _run("reg")
    e, L, cat = r["e"], lib(), r["cat"]
    K, R = cat.shape
    N = CASES["reg"][2]
    info = BnmfDecomposeInfo()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    cp = cat.ctypes.data_as(dp)

    def err():
        msg = L.bnmf_last_error().decode()
        assert msg
        return msg

    def call(h=None, last_n=10, used=None, ref=cp, nref=R, keep=None, steps=5, min_share=0.05, inf=info, at=None):
        h = e._h if h is None else h
        tail = (used, ref, nref, keep, steps, min_share, None, None, None, None, None, None if inf is None else C.byref(inf))
        return L.bnmf_decompose(h, last_n, *tail) if at is None else L.bnmf_decompose_at(h, at, last_n, *tail)
    for at in (None, e.iter):
        assert call(inf=None, at=at) == -1 and "null" in err()                                       # BNMF_EINVAL
        assert call(ref=None, at=at) == -1 and "null" in err()
        u = np.ones(10, dtype=np.int32); u[6] = 2
        assert call(used=u.ctypes.data_as(ip), at=at) == -1 and "used[6] = 2" in err()
        kp = np.ones(N, dtype=np.int32); kp[1] = -1
        assert call(keep=kp.ctypes.data_as(ip), at=at) == -1 and "keep[1] = -1" in err()
        for bad in (0, -1, 129):
            assert call(nref=bad, at=at) == -1 and f"R = {bad}" in err() and "BNMF_DEC_MAX_R = 128" in err()
        for bad in (0, -3, 100001):
            assert call(steps=bad, at=at) == -1 and f"n_steps = {bad}" in err()
        for bad in (float("nan"), float("inf"), -float("inf"), -0.5, 1.0, 1.5):
            assert call(min_share=bad, at=at) == -1 and "min_share" in err()
        for bad in (float("nan"), float("inf"), -1.0):
            cb = cat.copy(order="F"); cb[3, 2] = bad; cb[5, 3] = bad
            assert call(ref=cb.ctypes.data_as(dp), at=at) == -1 and "reference_P[3, 2]" in err()
        cb = cat.copy(order="F"); cb[:, 1] = 0.0
        assert call(ref=cb.ctypes.data_as(dp), at=at) == -1 and "column 1" in err() and "all zero" in err()
        u = np.zeros(10, dtype=np.int32); u[3] = 1
        assert call(used=u.ctypes.data_as(ip), at=at) == -2 and "1 used sample" in err()             # BNMF_ESIZE
        assert call(last_n=1, at=at) == -2 and err()
        # precedence: a bad argument before the number of used samples
        assert call(used=u.ctypes.data_as(ip), steps=0, at=at) == -1 and "n_steps" in err()
    # the range rule of bnmf_map_at: iterations [max(1, iter - window + 1), iter]
    assert call(last_n=5, at=e.iter + 1) == -2 and "are kept" in err()
    assert call(last_n=W + 1, at=e.iter) == -2 and "are kept" in err()
    assert call(last_n=3, at=e.iter - W + 1) == -2 and "are kept" in err()
    assert call(last_n=W + 1) == -2 and err()
    with pytest.raises(BnmfError, match="used has 3 entries"):
        e.decompose(10, cat, used=[1, 1, 1])
    with pytest.raises(BnmfError, match="keep has 2 entries"):
        e.decompose(10, cat, keep=[1, 1])
    with pytest.raises(BnmfError, match="rows are needed"):
        e.decompose(10, cat[:-1])
    M, _, _ = synth_counts(K, 7, 3, 21, mean_total=1500)
    # window = 0: BNMF_ESTATE
    z = Engine(M, 3, prior="gamma", seed=4, window=0)
    apply_hyperprior_params(z, "gamma", M, 3)
    z.init(); z.run(5)
    assert call(h=z._h, last_n=3) == -7 and "window = 0" in err()
    assert call(h=z._h, last_n=3, at=z.iter) == -7 and "window = 0" in err()
    z.close()
    assert L.bnmf_version() == 100
    # the handle is usable afterwards: the same bits as before the refusals
    _same(r["dev"], e.decompose(N_RANGE, cat, used=USED, end_iter=r["end"], n_steps=STEPS, min_share=MIN_SHARE, weights=True))


@pytest.mark.parametrize("case", ["cosmic", "ptn_mh", "sbfi"])
def test_the_call_is_read_only_for_the_chain(case):
    """a chain that calls decompose mid-run continues with the bits of a twin that never did"""
    r = _run(case)
    MH = CASES[case][5]
    b, row1 = _fresh(case)
    rows_b = np.vstack([row1[None, :], b.run(T_END - 1, converged=MH)])
    assert np.array_equal(_bits(rows_b), _bits(r["rows"]))
    more_a, more_b = r["e"].run(10, converged=MH), b.run(10, converged=MH)       # a called decompose at iteration 40, b never did
    assert np.array_equal(_bits(more_a), _bits(more_b))
    for nm in ("P", "E", "A"):
        assert np.array_equal(_bits(r["e"].get(nm)), _bits(b.get(nm))), nm
    b.close()
    _RUNS.pop(case)["e"].close()                                                 # (this case's chain has moved on)
