"""Similarity of tumours over a recorded range on the device (bnmf_similarity / bnmf_similarity_at, csrc/similarity.h) against the
numerical spec restated in numpy float64 (tests/similarity_ref.py, written from DESIGN.md 24): every output and every info field of
every case bit for bit, NaN compared as NaN, no tolerance — the operations are + - * /, sqrt, comparisons and whole numbers only; then
the equivalences and the refusals.

Every case keeps window = 16 samples and runs to iteration 40, so the kept range wraps the ring; the range is the 12 samples that end 2
iterations before `iter`, with a `used` mask that has gaps (tests/test_gpu_contrast.py's recipe).  K = 8 throughout (K enters through
the column sums of P only).  The shapes are the smallest that reach each path of the kernel, whose tile is 64 x 64 pairs and whose
staged chunk is 32 factors: G = 2 and 3, G = 63, 64 and 65 (one below, at and one above the tile edge), G = 150 (two tiles and a ragged
rest; also in bands of 1, 50 and 64 rows: 150, 3 and 3 bands), N = 1, 2 and 5, and N = 40 (two chunks of factors).  Chains: rank
learning (samples with A[n] = 0, one with A all zero: cosines exactly +0.0), real-valued Normal data, a refit with every column of P
held fixed.

The rings cannot be written from outside, so a tumour with an all-zero profile in one sample only and a NaN load cannot be planted on
the device: those conventions are pinned on the restatement (tests/test_similarity_host.py) and held on the device through it, where a
chain produces them (the rank-learning chain's sample without any factor)."""
import ctypes as C

import numpy as np
import pytest

import similarity_ref as R

pytestmark = pytest.mark.gpu

W, T_END, N_RANGE = 16, 40, 12
USED = np.array([1, 1, 0, 1, 1, 1, 0, 0, 1, 1, 1, 1], dtype=np.int32)
ARRAYS = ("neighbour_at", "neighbour", "dense", "tumour")
INFO = ("n_used", "n_included", "n_left_out", "top_k", "n_query", "n_pairs", "n_similar_pairs", "n_isolated", "least_typical_at", "mean_similarity",
        "least_typical", "min_cosine")
MIN_COS, TOP_K = 0.9, 5

# name: K, G, N, likelihood, prior, learning_rank, fixed_P, seed
CASES = {
    "g2": (8, 2, 2, "poisson", "gamma", False, False, 4),
    "g3": (8, 3, 1, "poisson", "gamma", False, False, 4),
    "g63": (8, 63, 5, "poisson", "gamma", False, False, 4),
    "g64": (8, 64, 5, "poisson", "gamma", False, False, 4),
    "g65": (8, 65, 5, "poisson", "gamma", False, False, 4),
    "g150": (8, 150, 5, "poisson", "gamma", False, False, 4),              # two tiles and a ragged rest
    "n40": (8, 20, 40, "poisson", "gamma", False, False, 4),               # two staged chunks of factors
    "sbfi": (96, 8, 20, "poisson", "gamma", True, False, 14),              # samples with A[n] = 0, one with A = 0
    "normal": (12, 10, 3, "normal", "exponential", False, False, 4),       # real-valued data
    "refit": (8, 30, 3, "poisson", "gamma", False, True, 4),               # every column of P held fixed
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _data(case):
    from bayesnmf_amd.setup import synth_counts
    K, G, N, lk, *_ = CASES[case]
    if lk == "normal":
        rng = np.random.default_rng(11)
        return np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, 3)) @ rng.gamma(0.5, 1.0, size=(3, G)) + rng.normal(0.0, 0.5, size=(K, G)))
    M, _, _ = synth_counts(K, G, min(3, N), 21, mean_total=1500)
    return M


def _temps():
    return np.concatenate([np.ones(20), np.zeros(3), 10.0 ** np.linspace(-6, 0, 60), np.ones(100)])


_RUNS = {}


def _run(case):
    """the chain at iteration 40, the used samples of the range and their loads' restatement inputs: once per case"""
    if case in _RUNS:
        return _RUNS[case]
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import apply_hyperprior_params
    K, G, N, lk, prior, lr, fixed, seed = CASES[case]
    M = _data(case)
    e = Engine(M, N, likelihood=lk, prior=prior, learning_rank=lr, seed=seed, window=W, temperature=_temps() if lr else None)
    apply_hyperprior_params(e, prior, M, N)
    if fixed:
        rng = np.random.default_rng(3)
        P0 = rng.gamma(0.5, 1.0, size=(K, N))
        e.set("P", np.asfortranarray(P0 / P0.sum(axis=0)))
        e.set_fixed("P", np.ones(N, dtype=np.int32))
    e.init()
    e.run(T_END - 1)
    assert e.iter == T_END
    end = T_END - 2
    back = T_END - (end - N_RANGE + 1) + 1
    sel = np.where(USED == 1)[0]
    win = {nm: np.stack([e.window(nm, back)[i] for i in sel]) for nm in ("P", "E", "A")}
    samples = (win["P"], win["E"], win["A"].reshape(len(sel), N))
    _RUNS[case] = dict(e=e, end=end, samples=samples, G=G, N=N)
    return _RUNS[case]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for r in _RUNS.values():
        r["e"].close()
    _RUNS.clear()


def _differences(tag, a, b, arrays=ARRAYS, info=INFO):
    """the names of the outputs of a that are not b's, bit for bit with NaN equal to NaN (printed with the first place they differ)"""
    bad = []
    for k in arrays:
        if k not in a and k not in b:
            continue
        if (k in a) != (k in b):
            if np.asarray(a[k] if k in a else b[k]).size == 0:                                                # (top_k = 0 or no query: the binding leaves it out)
                continue
            print(f"similarity[{tag}] {k}: only one side has it")
            bad.append(k)
            continue
        x, y = np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)
        if x.shape != y.shape:
            print(f"similarity[{tag}] {k}: shapes {x.shape} and {y.shape}")
            bad.append(k)
            continue
        nx, ny = np.isnan(x), np.isnan(y)
        ne = (nx != ny) | (~nx & ~ny & (_bits(x).reshape(x.shape) != _bits(y).reshape(y.shape)))
        if ne.any():
            i = tuple(np.argwhere(ne)[0])
            print(f"similarity[{tag}] {k}: {int(ne.sum())} of {ne.size} differ, first at {i}: {x[i]!r} against {y[i]!r}")
            bad.append(k)
    for k in info:
        fa, fb = float(a[k]), float(b[k])
        if not ((np.isnan(fa) and np.isnan(fb)) or _bits(fa) == _bits(fb)):
            print(f"similarity[{tag}] {k}: {a[k]!r} against {b[k]!r}")
            bad.append(k)
    return bad


def _queries(G):
    return np.array(sorted({0, G - 1, G // 2, min(64, G - 1)}) + [0], dtype=np.int32)        # the ends, a tile edge, one named twice


@pytest.mark.parametrize("case", list(CASES))
def test_every_output_is_the_restatement_bit_for_bit(case, monkeypatch):
    r = _run(case)
    e, G, N = r["e"], r["G"], r["N"]
    q = _queries(G)
    kw = dict(used=USED, end_iter=r["end"], min_cosine=MIN_COS)
    ref = R.similarity_reference(*r["samples"], query=q, top_k=TOP_K, min_cosine=MIN_COS)
    dev = e.similarity(N_RANGE, query=q, top_k=TOP_K, **kw)
    A = r["samples"][2]
    print(f"similarity[{case}] S {dev['n_used']} m {dev['n_included']} pairs {dev['n_pairs']} similar {dev['n_similar_pairs']} isolated {dev['n_isolated']} mean "
          f"{dev['mean_similarity']!r} least typical {dev['least_typical']!r} at {dev['least_typical_at']}; samples that exclude a factor "
          f"{int((A == 0).any(axis=1).sum())}")
    assert dev["neighbour_at"].shape == (G, TOP_K) and dev["neighbour"].shape == (3, G, TOP_K) and dev["dense"].shape == (3, len(q), G) and dev["tumour"].shape == (3, G)
    bad = _differences(case, dev, ref)
    if case == "sbfi":
        assert (A == 0).any() and (A == 0).all(axis=1).any(), "no used sample without a factor"
        s0 = int(np.where((A == 0).all(axis=1))[0][0])
        assert (ref["c"][s0] == 0.0).all() and not np.signbit(ref["c"][s0]).any()              # the sample with no factor: every cosine exactly +0.0
        assert not np.isnan(dev["tumour"]).any() and (dev["dense"][2][~np.isnan(dev["dense"][2])] < 1.0).all()
    # bands of rows through the scratch: the same bits
    for band in ("1", "50", "64"):
        monkeypatch.setenv("BNMF_SIM_BAND", band)
        bad += _differences(f"{case}, bands of {band}", e.similarity(N_RANGE, query=q, top_k=TOP_K, **kw), ref)
        monkeypatch.delenv("BNMF_SIM_BAND")
    # top_k 0, 1, m - 1 and 32
    for k in sorted({0, 1, min(G - 1, 32), 32}):
        bad += _differences(f"{case}, top_k {k}", e.similarity(N_RANGE, top_k=k, **kw), R.similarity_reference(*r["samples"], top_k=k, min_cosine=MIN_COS))
    # the queries alone are the same rows, also in bands, and say that the pass over all pairs did not run
    alone_ref = R.similarity_reference(*r["samples"], query=q, top_k=0, min_cosine=MIN_COS, tumour=False)
    assert not _differences("restatement, the queries alone", alone_ref, ref, arrays=("dense",), info=())
    for band in (None, "2"):
        if band:
            monkeypatch.setenv("BNMF_SIM_BAND", band)
        alone = e.similarity(N_RANGE, query=q, top_k=0, tumour=False, **kw)
        if band:
            monkeypatch.delenv("BNMF_SIM_BAND")
        assert "tumour" not in alone and "neighbour" not in alone and alone["n_similar_pairs"] == -1 and alone["least_typical_at"] == -1
        bad += _differences(f"{case}, the queries alone, band {band}", alone, alone_ref)
    # other thresholds: every pair similar, no pair similar
    for mc in (-2.0, 2.0):
        d = e.similarity(N_RANGE, top_k=2, used=USED, end_iter=r["end"], min_cosine=mc)
        bad += _differences(f"{case}, min_cosine {mc:g}", d, R.similarity_reference(*r["samples"], top_k=2, min_cosine=mc))
        assert d["n_similar_pairs"] == (G * (G - 1) // 2 if mc < 0 else 0) and d["n_isolated"] == (0 if mc < 0 else G)
    assert not bad, bad


@pytest.mark.parametrize("case", ["g65", "g150", "sbfi"])
def test_include_leaves_tumours_out(case):
    """the first, the last and a tile-edge tumour left out: the restatement's bits, which are those of the cohort without them
    (tests/test_similarity_host.py)"""
    r = _run(case)
    e, G = r["e"], r["G"]
    inc = np.ones(G, dtype=np.int32)
    inc[[0, G - 1, min(63, G - 2)]] = 0
    q = np.array([1, G - 3], dtype=np.int32)
    dev = e.similarity(N_RANGE, include=inc, query=q, top_k=TOP_K, used=USED, end_iter=r["end"], min_cosine=MIN_COS)
    assert dev["n_left_out"] == 3 and np.isnan(dev["tumour"][:, inc == 0]).all() and (dev["neighbour_at"][inc == 0] == -1).all()
    assert not (np.isin(dev["neighbour_at"], np.where(inc == 0)[0])).any() and np.isnan(dev["dense"][:, :, inc == 0]).all()
    assert not _differences(case, dev, R.similarity_reference(*r["samples"], include=inc, query=q, top_k=TOP_K, min_cosine=MIN_COS))


@pytest.mark.parametrize("case", ["g2", "g150", "normal"])
def test_equivalent_calls_give_the_same_bits(case):
    r = _run(case)
    e, end, G = r["e"], r["end"], r["G"]
    q = _queries(G)
    kw = dict(query=q, top_k=3, min_cosine=MIN_COS)
    first = e.similarity(N_RANGE, used=USED, end_iter=end, **kw)
    assert not _differences("again", first, e.similarity(N_RANGE, used=USED, end_iter=end, **kw))
    assert not _differences("at", e.similarity(10, **kw), e.similarity(10, end_iter=e.iter, **kw))              # bnmf_similarity is bnmf_similarity_at(iter)
    assert not _differences("ones", e.similarity(10, **kw), e.similarity_at(e.iter, 10, used=np.ones(10, dtype=np.int32), include=np.ones(G, dtype=np.int32), **kw))
    s2 = np.zeros(N_RANGE, dtype=np.int32)
    s2[[2, 9]] = 1                                                                                             # S = 2
    two = e.similarity(N_RANGE, used=s2, end_iter=end, **kw)
    assert two["n_used"] == 2
    back = e.iter - (end - N_RANGE + 1) + 1
    win = {nm: np.stack([e.window(nm, back)[i] for i in (2, 9)]) for nm in ("P", "E", "A")}
    assert not _differences("S = 2", two, R.similarity_reference(win["P"], win["E"], win["A"].reshape(2, -1), **kw))
    # each output NULL in turn, then all of them: the others and the info fields are the same (the pass over all pairs runs: top_k > 0)
    from bayesnmf_amd.engine import lib, BnmfSimilarityInfo
    L, dp, ip = lib(), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    Q = len(q)
    for skip in ARRAYS + ("all",):
        bufs = dict(neighbour_at=np.full((G, 3), -7, dtype=np.int32), neighbour=np.full((3, G, 3), -7.0), dense=np.full((3, Q, G), -7.0), tumour=np.full((3, G), -7.0))
        ptr = {k: (None if skip in (k, "all") else v.ctypes.data_as(ip if k == "neighbour_at" else dp)) for k, v in bufs.items()}
        info = BnmfSimilarityInfo()
        assert L.bnmf_similarity_at(e._h, end, N_RANGE, USED.ctypes.data_as(ip), None, q.ctypes.data_as(ip), Q, 3, MIN_COS, ptr["neighbour_at"], ptr["neighbour"],
                                    ptr["dense"], ptr["tumour"], C.byref(info)) == 0
        got = dict(bufs, **{k: getattr(info, k) for k in INFO})
        for k in ARRAYS:
            if skip in (k, "all"):
                assert (bufs[k] == -7).all(), k                                                                # (not written)
        assert not _differences(f"without {skip}", got, first, tuple(k for k in ARRAYS if skip not in (k, "all")))


def test_refusals():
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import lib, BnmfSimilarityInfo, BnmfError
    from bayesnmf_amd.setup import apply_hyperprior_params
    r = _run("g65")
    e, G, L = r["e"], r["G"], lib()
    info = BnmfSimilarityInfo()
    ip = C.POINTER(C.c_int32)
    before = e.similarity(N_RANGE, used=USED, end_iter=r["end"], top_k=TOP_K, query=[3])

    def err():
        msg = L.bnmf_last_error().decode()
        assert msg
        return msg

    def call(n=10, used=None, include=None, query=None, Q=None, k=3, mc=0.9, inf=info, at=None, h=None):
        u = None if used is None else used.ctypes.data_as(ip)
        i = None if include is None else include.ctypes.data_as(ip)
        qp = None if query is None else query.ctypes.data_as(ip)
        Q = (0 if query is None else len(query)) if Q is None else Q
        f = None if inf is None else C.byref(inf)
        h = e._h if h is None else h
        if at is None:
            return L.bnmf_similarity(h, n, u, i, qp, Q, k, mc, None, None, None, None, f)
        return L.bnmf_similarity_at(h, at, n, u, i, qp, Q, k, mc, None, None, None, None, f)

    for at in (None, e.iter):
        assert call(inf=None, at=at) == -1 and "null" in err()                                       # BNMF_EINVAL
        u = np.ones(10, dtype=np.int32); u[6] = 2
        assert call(used=u, at=at) == -1 and "used[6] = 2" in err()
        inc = np.ones(G, dtype=np.int32); inc[64] = -1
        assert call(include=inc, at=at) == -1 and "include[64] = -1" in err()
        assert call(Q=-1, at=at) == -1 and "Q = -1" in err()
        assert call(Q=2, at=at) == -1 and "query is null" in err()
        assert call(query=np.array([1, G], dtype=np.int32), at=at) == -1 and f"query[1] = {G}" in err()
        assert call(query=np.array([-1], dtype=np.int32), at=at) == -1 and "query[0] = -1" in err()
        inc = np.ones(G, dtype=np.int32); inc[7] = 0
        assert call(include=inc, query=np.array([3, 7], dtype=np.int32), at=at) == -1 and "query[1] = 7" in err() and "leaves out" in err()
        for k in (-1, 33):
            assert call(k=k, at=at) == -1 and f"top_k = {k}" in err()
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert call(mc=bad, at=at) == -1 and "min_cosine" in err()
        u = np.zeros(10, dtype=np.int32); u[3] = 1
        assert call(used=u, at=at) == -2 and "1 used sample" in err()                                # BNMF_ESIZE
        inc = np.zeros(G, dtype=np.int32); inc[5] = 1
        assert call(include=inc, at=at) == -2 and "1 included tumour" in err()
        assert call(include=np.zeros(G, dtype=np.int32), at=at) == -2 and "0 included tumours" in err()
    assert call(n=1) == -2 and err()
    assert call(n=W + 1) == -2 and err()
    # the range rule of bnmf_attribution_at: iterations [max(1, iter - window + 1), iter]
    assert call(n=5, at=e.iter + 1) == -2 and "are kept" in err()
    assert call(n=W + 1, at=e.iter) == -2 and "are kept" in err()
    assert call(n=3, at=e.iter - W + 1) == -2 and "are kept" in err()
    with pytest.raises(BnmfError, match="used has 3 entries"):
        e.similarity(10, used=[1, 1, 1])
    with pytest.raises(BnmfError, match="include has shape"):
        e.similarity(10, include=[1, 1, 1])
    with pytest.raises(BnmfError, match="top_k = 40"):
        e.similarity(10, top_k=40)
    # window = 0: BNMF_ESTATE
    from bayesnmf_amd.setup import synth_counts
    M, _, _ = synth_counts(8, 6, 3, 21, mean_total=1500)
    z = Engine(M, 3, prior="gamma", seed=4, window=0)
    apply_hyperprior_params(z, "gamma", M, 3)
    z.init(); z.run(5)
    assert call(n=3, h=z._h) == -7 and "window = 0" in err()
    assert call(n=3, at=z.iter, h=z._h) == -7 and "window = 0" in err()
    z.close()
    assert L.bnmf_version() == 100
    assert call(mc=-1.0, k=0) == 0 and info.n_used == 10 and info.n_similar_pairs == G * (G - 1) // 2 and info.top_k == 0     # any finite threshold is allowed
    # the handle is usable afterwards: the same bits as before the refusals
    assert not _differences("afterwards", before, e.similarity(N_RANGE, used=USED, end_iter=r["end"], top_k=TOP_K, query=[3]))


def test_the_call_is_read_only_for_the_chain():
    """a chain that calls similarity mid-run continues with the bits of a twin that never did"""
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import apply_hyperprior_params
    K, G, N, lk, prior, lr, fixed, seed = CASES["g65"]
    M = _data("g65")
    a, b = (Engine(M, N, likelihood=lk, prior=prior, seed=seed, window=W) for _ in range(2))
    for c in (a, b):
        apply_hyperprior_params(c, prior, M, N)
        c.init(); c.run(20)
    a.similarity(12, query=[0, 64], top_k=4)
    ra, rb = a.run(10), b.run(10)
    assert np.array_equal(_bits(ra), _bits(rb))
    for nm in ("P", "E", "A"):
        assert np.array_equal(_bits(a.get(nm)), _bits(b.get(nm))), nm
    a.close(); b.close()
