"""Group contrasts of exposures over a recorded range on the device (bnmf_contrast / bnmf_contrast_at, csrc/contrast.h) against the
numerical spec restated in numpy float64 (tests/contrast_ref.py, written from DESIGN.md 19): every output and every info field of every
case bit for bit, NaN compared as NaN, no tolerance — the operations are + - * /, comparisons and integer counts only; then the
equivalences and the refusals.

Every case keeps window = 16 samples and runs to iteration 40, so the kept range wraps the ring; the range is the 12 samples that end
2 iterations before `iter`, with a `used` mask that has gaps (tests/test_gpu_attribution.py's recipe).  The shapes are the smallest that
reach each path: interleaved membership with groups of 1, 64, 65 and 129 tumours (one accumulator, a full round, one element into the
second round, one into the third) and 5 tumours left out — that is 264 tumours, not the 200 the request for this case names, which
cannot hold these four groups; one group (no pair) and two; N = 3 / 5, 12, 20 and 30 for the four register tiles of 8, 16, 24 and 32
factors and N = 40 for the tiled form, with G = 70, not a multiple of 64; the rank-learning chain of test_gpu_attribution (its A is all
zero at iteration 31, a used sample: t = 0, the share 0, no NaN); real-valued data with negative cells; rings recorded by the MH sweep."""
import ctypes as C

import numpy as np
import pytest

import contrast_ref as R

pytestmark = pytest.mark.gpu

W, T_END, N_RANGE = 16, 40, 12
USED = np.array([1, 1, 0, 1, 1, 1, 0, 0, 1, 1, 1, 1], dtype=np.int32)
ARRAYS = ("group", "pair", "series", "sizes")
INFO = ("n_used", "n_groups", "n_pairs", "n_left_out", "n_credible", "min_load", "credible_interval")
MIN_LOAD, CI = 5.0, 0.9


def _interleaved():
    """264 tumours: groups of 1, 64, 65 and 129 dealt out in a fixed shuffle, 5 left out"""
    g = np.concatenate([np.full(1, 0), np.full(64, 1), np.full(65, 2), np.full(129, 3), np.full(5, -1)]).astype(np.int32)
    return np.random.default_rng(17).permutation(g)


def _cyclic(G, Cn, out_every=0):
    g = ((np.arange(G) * 7 + 3) % Cn).astype(np.int32)
    if out_every:
        g[1::out_every] = -1
    return g


# name: K, G, N, likelihood, prior, MH, learning_rank, seed, groups
CASES = {
    "interleaved": (8, 264, 3, "poisson", "gamma", False, False, 4, _interleaved()),
    "one_group": (96, 70, 5, "poisson", "gamma", False, False, 4, np.zeros(70, dtype=np.int32)),
    "two_groups": (96, 70, 5, "poisson", "gamma", False, False, 4, _cyclic(70, 2, 9)),
    "n12": (8, 70, 12, "poisson", "gamma", False, False, 4, _cyclic(70, 3)),               # the register tile of 16
    "n30": (8, 70, 30, "poisson", "gamma", False, False, 4, _cyclic(70, 2)),               # ... of 32
    "n40": (8, 70, 40, "poisson", "gamma", False, False, 4, _cyclic(70, 3, 13)),           # past the register tiles: the tiled form, 5 tiles
    "sbfi": (96, 8, 20, "poisson", "gamma", False, True, 14, _cyclic(8, 2)),               # the tile of 24; samples with A[n] = 0, one with A = 0
    "normal": (12, 10, 3, "normal", "exponential", False, False, 4, _cyclic(10, 3)),       # real-valued data, negative cells
    "ptn_mh": (96, 6, 5, "poisson", "truncnormal", True, False, 4, _cyclic(6, 2)),         # rings recorded by the MH sweep
}
SAME_CHAIN = {"two_groups": "one_group"}      # cases that differ in their groups alone share one chain


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
    K, G, N, lk, prior, MH, lr, seed, _ = CASES[case]
    M = _data(case)
    return Engine(M, N, likelihood=lk, prior=prior, MH=MH, learning_rank=lr, seed=seed, window=W, temperature=_temps() if lr else None), M


def _fresh(case):
    from bayesnmf_amd.setup import apply_hyperprior_params
    e, M = _create(case)
    apply_hyperprior_params(e, CASES[case][4], M, CASES[case][2])
    row1 = e.init()
    return e, M, row1


_CHAINS, _RUNS = {}, {}


def _chain(case):
    """the chain at iteration 40, its metric rows and the used samples of the range: made once per chain"""
    key = SAME_CHAIN.get(case, case)
    if key in _CHAINS:
        return _CHAINS[key]
    K, G, N, lk, prior, MH, lr, *_ = CASES[key]
    e, M, row1 = _fresh(key)
    rows = np.vstack([row1[None, :], e.run(T_END - 1, converged=MH)])
    assert e.iter == T_END
    end = T_END - 2
    first = end - N_RANGE + 1
    back = T_END - first + 1
    sel = np.where(USED == 1)[0]
    win = {nm: np.stack([e.window(nm, back)[i] for i in sel]) for nm in ("P", "E", "A")}
    samples = (win["P"], win["E"], win["A"].reshape(len(sel), N))
    _CHAINS[key] = dict(e=e, M=M, rows=rows, end=end, samples=samples)
    return _CHAINS[key]


def _run(case):
    """the chain, the device's contrast of the range and the restatement: made once per case"""
    if case in _RUNS:
        return _RUNS[case]
    ch = _chain(case)
    groups = CASES[case][8]
    ref = R.contrast_reference(*ch["samples"], groups, min_load=MIN_LOAD, credible_interval=CI)
    dev = ch["e"].contrast(N_RANGE, groups, used=USED, end_iter=ch["end"], min_load=MIN_LOAD, credible_interval=CI, series=True)
    _RUNS[case] = dict(ch, groups=groups, ref=ref, dev=dev)
    return _RUNS[case]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for r in _CHAINS.values():
        r["e"].close()
    _CHAINS.clear()
    _RUNS.clear()


def _differences(tag, a, b, arrays=ARRAYS):
    """the names of the outputs of a that are not b's, bit for bit with NaN equal to NaN (printed with the first place they differ)"""
    bad = []
    for k in arrays:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape:
            print(f"contrast[{tag}] {k}: shapes {x.shape} and {y.shape}")
            bad.append(k)
            continue
        if x.dtype.kind != "f":
            ne = x != y
        else:
            nx, ny = np.isnan(x), np.isnan(y)
            ne = (nx != ny) | (~nx & ~ny & (_bits(x).reshape(x.shape) != _bits(y).reshape(y.shape)))
        if ne.any():
            i = tuple(np.argwhere(ne)[0])
            print(f"contrast[{tag}] {k}: {int(ne.sum())} of {ne.size} differ, first at {i}: {x[i]!r} against {y[i]!r}")
            bad.append(k)
    for k in INFO:
        if k == "n_credible":
            same = list(a[k]) == list(b[k])
        else:
            same = _bits(float(a[k])) == _bits(float(b[k]))
        if not same:
            print(f"contrast[{tag}] {k}: {a[k]!r} against {b[k]!r}")
            bad.append(k)
    return bad


def _same(a, b, arrays=ARRAYS):
    assert not _differences("equivalence", a, b, arrays)


@pytest.mark.parametrize("case", list(CASES))
def test_every_output_is_the_restatement_bit_for_bit(case, monkeypatch):
    r = _run(case)
    K, G, N, lk, *_ = CASES[case]
    dev, ref, e, groups = r["dev"], r["ref"], r["e"], r["groups"]
    A = r["samples"][2]
    Cn = int(groups.max()) + 1
    NP = Cn * (Cn - 1) // 2
    print(f"contrast[{case}] S {dev['n_used']} sizes {dev['sizes'].tolist()} left out {dev['n_left_out']} n_credible {dev['n_credible']}; "
          f"samples that exclude a factor {int((A == 0).any(axis=1).sum())}, (s, g) with t == 0 {int((ref['t'] == 0).sum())}")
    if case == "interleaved":
        assert dev["sizes"].tolist() == [1, 64, 65, 129] and dev["n_left_out"] == 5
        assert (np.diff(np.where(groups == 3)[0]) > 1).any(), "the members are contiguous"
    if case == "sbfi":
        assert (A == 0).any() and (ref["t"] == 0).any(), "no used sample without a factor"
        assert not np.isnan(dev["series"]).any()
    if case == "normal":
        assert (np.asarray(r["M"]) < 0).any(), "no negative cell"
    S = int(USED.sum())
    assert dev["n_used"] == S and dev["group"].shape == (3, 4, N, Cn) and dev["pair"].shape == (3, 6, N, NP) and dev["series"].shape == (3, S, N, Cn)
    bad = _differences(case, dev, ref)
    # the other form of the kernel (tiles of 8 factors, the column read again): the same bits
    monkeypatch.setenv("BNMF_CON_FORM", "1")
    bad += _differences(case + ", tiled form", e.contrast(N_RANGE, groups, used=USED, end_iter=r["end"], min_load=MIN_LOAD, credible_interval=CI, series=True), ref)
    monkeypatch.delenv("BNMF_CON_FORM")
    # prevalence all 1 / all 0, and no interval: NaN rows
    for ml, ci in ((0.0, CI), (1e300, 0.0), (MIN_LOAD, -1.0)):
        d = e.contrast(N_RANGE, groups, used=USED, end_iter=r["end"], min_load=ml, credible_interval=ci, series=True)
        bad += _differences(f"{case}, min_load {ml:g}, interval {ci:g}", d, R.contrast_reference(*r["samples"], groups, min_load=ml, credible_interval=ci))
        if ml == 0.0:
            assert (d["series"][2] == 1.0).all()
        if ml == 1e300:
            assert (d["series"][2] == 0.0).all()
        if ci <= 0:
            assert np.isnan(d["group"][:, 2:]).all() and np.isnan(d["pair"][:, 2:4]).all() and d["n_credible"] == [0, 0, 0]
    assert not bad, bad


@pytest.mark.parametrize("case", ["interleaved", "sbfi", "normal"])
def test_equivalent_calls_give_the_same_bits(case):
    r = _run(case)
    e, end, groups = r["e"], r["end"], r["groups"]
    kw = dict(min_load=MIN_LOAD, credible_interval=CI, series=True)
    _same(r["dev"], e.contrast(N_RANGE, groups, used=USED, end_iter=end, **kw))                      # a second call
    _same(e.contrast(10, groups, **kw), e.contrast(10, groups, end_iter=e.iter, **kw))               # bnmf_contrast is bnmf_contrast_at(iter)
    _same(e.contrast(10, groups, **kw), e.contrast(10, groups, used=np.ones(10, dtype=np.int32), **kw))   # NULL is all ones
    _same(e.contrast(N_RANGE, groups, end_iter=end, **kw), e.contrast(N_RANGE, groups, used=np.ones(N_RANGE, dtype=np.int32), end_iter=end, **kw))
    # each output NULL in turn, then all of them: the others and the info fields are the same
    from bayesnmf_amd.engine import lib, BnmfContrastInfo
    L, dp, ip = lib(), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    N, Cn = CASES[case][2], int(groups.max()) + 1
    NP, S = Cn * (Cn - 1) // 2, int(USED.sum())
    g32 = np.ascontiguousarray(groups, dtype=np.int32)
    for skip in ("group", "pair", "series", "sizes", "all"):
        bufs = dict(group=np.full((3, 4, Cn, N), -7.0), pair=np.full((3, 6, NP, N), -7.0), series=np.full((3, S, Cn, N), -7.0), sizes=np.full(Cn, -7, dtype=np.int32))
        ptr = {k: (None if skip in (k, "all") else v.ctypes.data_as(ip if k == "sizes" else dp)) for k, v in bufs.items()}
        info = BnmfContrastInfo()
        assert L.bnmf_contrast_at(e._h, end, N_RANGE, USED.ctypes.data_as(ip), g32.ctypes.data_as(ip), MIN_LOAD, CI, ptr["group"], ptr["pair"], ptr["series"],
                                  ptr["sizes"], C.byref(info)) == 0
        got = dict(group=bufs["group"].transpose(0, 1, 3, 2), pair=bufs["pair"].transpose(0, 1, 3, 2), series=bufs["series"].transpose(0, 1, 3, 2), sizes=bufs["sizes"],
                   n_credible=[int(v) for v in info.n_credible], **{k: getattr(info, k) for k in INFO if k != "n_credible"})
        for k in ARRAYS:
            if skip in (k, "all"):
                assert (bufs[k] == -7).all(), k                                                          # (not written)
        _same(got, r["dev"], tuple(k for k in ARRAYS if skip not in (k, "all")))


def test_renumbering_the_groups_permutes_the_outputs():
    r = _run("interleaved")
    groups = r["groups"]
    perm = np.array([2, 0, 3, 1])                                                                    # old label -> new label
    g2 = np.where(groups < 0, -1, perm[np.maximum(groups, 0)]).astype(np.int32)
    d = r["e"].contrast(N_RANGE, g2, used=USED, end_iter=r["end"], min_load=MIN_LOAD, credible_interval=CI, series=True)
    assert np.array_equal(_bits(d["series"][:, :, :, perm]), _bits(r["dev"]["series"])) and np.array_equal(_bits(d["group"][:, :, :, perm]), _bits(r["dev"]["group"]))
    assert np.array_equal(d["sizes"][perm], r["dev"]["sizes"])
    assert not _differences("renumbered", d, R.contrast_reference(*r["samples"], g2, min_load=MIN_LOAD, credible_interval=CI))


@pytest.mark.parametrize("case", ["two_groups", "normal"])
def test_a_reopened_chain_gives_the_same_bits(case, tmp_path):
    r = _run(case)
    path = str(tmp_path / "state.bin")
    r["e"].save_state(path)
    c, _ = _create(case)
    assert c.load_state(path) == T_END
    _same(r["dev"], c.contrast(N_RANGE, r["groups"], used=USED, end_iter=r["end"], min_load=MIN_LOAD, credible_interval=CI, series=True))
    c.close()


def test_refusals():
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import lib, BnmfContrastInfo, BnmfError
    from bayesnmf_amd.setup import apply_hyperprior_params
    r = _run("two_groups")
    e, M, L = r["e"], r["M"], lib()
    G = CASES["two_groups"][1]
    info = BnmfContrastInfo()
    ip = C.POINTER(C.c_int32)
    good = np.ascontiguousarray(r["groups"], dtype=np.int32)

    def err():
        msg = L.bnmf_last_error().decode()
        assert msg
        return msg

    def call(n=10, used=None, groups=good, min_load=1.0, ci=0.9, inf=info, at=None, h=None):
        u = None if used is None else used.ctypes.data_as(ip)
        g = None if groups is None else groups.ctypes.data_as(ip)
        i = None if inf is None else C.byref(inf)
        h = e._h if h is None else h
        if at is None:
            return L.bnmf_contrast(h, n, u, g, min_load, ci, None, None, None, None, i)
        return L.bnmf_contrast_at(h, at, n, u, g, min_load, ci, None, None, None, None, i)

    for at in (None, e.iter):
        assert call(inf=None, at=at) == -1 and "null" in err()                                       # BNMF_EINVAL
        assert call(groups=None, at=at) == -1 and "null" in err()
        u = np.ones(10, dtype=np.int32); u[6] = 2
        assert call(used=u, at=at) == -1 and "used[6] = 2" in err()
        u[6] = -1
        assert call(used=u, at=at) == -1 and "used[6] = -1" in err()
        g = good.copy(); g[11] = -2
        assert call(groups=g, at=at) == -1 and "groups[11] = -2" in err()
        g[11] = 64
        assert call(groups=g, at=at) == -1 and "groups[11] = 64" in err()
        g = good.copy(); g[g == 1] = 3                                                               # labels 0 and 3: groups 1 and 2 are empty
        assert call(groups=g, at=at) == -1 and "group 1 has no member" in err()
        assert call(groups=np.full(G, -1, dtype=np.int32), at=at) == -1 and "no tumour is in any group" in err()
        for bad in (float("nan"), float("inf"), -float("inf"), -0.5):
            assert call(min_load=bad, at=at) == -1 and "min_load" in err()
        for bad in (float("nan"), 1.0, 1.5, float("inf")):
            assert call(ci=bad, at=at) == -1 and "credible_interval" in err()
        u = np.zeros(10, dtype=np.int32); u[3] = 1
        assert call(used=u, at=at) == -2 and "1 used sample" in err()                                # BNMF_ESIZE
    assert call(n=1) == -2 and err()
    assert call(n=W + 1) == -2 and err()
    # the range rule of bnmf_waic_at: iterations [max(1, iter - window + 1), iter]
    assert call(n=5, at=e.iter + 1) == -2 and "are kept" in err()
    assert call(n=W + 1, at=e.iter) == -2 and "are kept" in err()
    assert call(n=3, at=e.iter - W + 1) == -2 and "are kept" in err()
    with pytest.raises(BnmfError, match="used has 3 entries"):
        e.contrast(10, good, used=[1, 1, 1])
    with pytest.raises(BnmfError, match="G = 70 labels are needed"):
        e.contrast(10, good[:5])
    # window = 0: BNMF_ESTATE
    z = Engine(M, 3, prior="gamma", seed=4, window=0)
    apply_hyperprior_params(z, "gamma", M, 3)
    z.init(); z.run(5)
    assert call(n=3, h=z._h) == -7 and "window = 0" in err()
    assert call(n=3, at=z.iter, h=z._h) == -7 and "window = 0" in err()
    z.close()
    assert L.bnmf_version() == 100
    assert call(ci=0.0) == 0 and info.n_credible[0] == 0 and info.n_groups == 2 and info.n_pairs == 1   # no interval is allowed
    assert call(ci=-3.0) == 0
    # the handle is usable afterwards: the same bits as before the refusals
    _same(r["dev"], e.contrast(N_RANGE, r["groups"], used=USED, end_iter=r["end"], min_load=MIN_LOAD, credible_interval=CI, series=True))


@pytest.mark.parametrize("case", ["one_group", "ptn_mh", "sbfi"])
def test_the_call_is_read_only_for_the_chain(case):
    """a chain that calls contrast mid-run continues with the bits of a twin that never did"""
    r = _run(case)
    MH = CASES[case][5]
    b, _, row1 = _fresh(case)
    rows_b = np.vstack([row1[None, :], b.run(T_END - 1, converged=MH)])
    assert np.array_equal(_bits(rows_b), _bits(r["rows"]))
    more_a, more_b = r["e"].run(10, converged=MH), b.run(10, converged=MH)       # a called contrast at iteration 40, b never did
    assert np.array_equal(_bits(more_a), _bits(more_b))
    for nm in ("P", "E", "A"):
        assert np.array_equal(_bits(r["e"].get(nm)), _bits(b.get(nm))), nm
    b.close()
    key = SAME_CHAIN.get(case, case)                                             # (this chain has moved on)
    _CHAINS.pop(key)["e"].close()
    for c in [c for c in _RUNS if SAME_CHAIN.get(c, c) == key]:
        _RUNS.pop(c)
