"""Co-activity of signatures over a recorded range on the device (bnmf_coactivity / bnmf_coactivity_at, csrc/coactivity.h) against the
numerical spec restated in numpy float64 (tests/coactivity_ref.py, written from DESIGN.md 21): pair, series and every info field of every
case bit for bit, NaN compared as NaN, no tolerance — the operations are + - * /, sqrt, comparisons and whole numbers only; then the
forms, the equivalences and the refusals.

Every chain is a dozen iterations (the rank-learning one 40: its schedule excludes factors from iteration 21 on) with window = 16;
the range is the 12 samples that end 2 iterations before `iter`, with a `used` mask that has gaps.  The shapes are the smallest that reach
each path: N = 3 (one partial tile of either form), N = 5 and N = 9 (tile remainders on both axes: 3 tiles of 4, 5 of 2); G = 1,100 with
3, 63, 64, 65, 1,023, 1,024 and 1,025 members in a fixed shuffle (one wave round, a block boundary with one member in the last block;
sorted keys of 64, 128, 1,024 and 2,048); real-valued data; rings recorded by the MH sweep; a rank-learning chain whose samples exclude
factors; a chain whose first sample is a supplied E of multiples of 0.25 (tie groups)."""
import ctypes as C

import numpy as np
import pytest

import coactivity_ref as R

pytestmark = pytest.mark.gpu

W, N_RANGE = 16, 12
USED = np.array([1, 1, 0, 1, 1, 1, 0, 0, 1, 1, 1, 1], dtype=np.int32)
ARRAYS = ("pair", "series")
INTS = ("n_used", "n_included", "n_left_out", "n_pairs", "n_blocks", "max_cosine_at")
REALS = ("max_cosine", "min_load", "credible_interval")
CI, ML = 0.9, 1.0


def _include(G, m, seed=17):
    """m of the G tumours in a fixed shuffle"""
    inc = np.zeros(G, dtype=np.int32)
    inc[np.random.default_rng(seed).permutation(G)[:m]] = 1
    return inc


# chain: K, G, N, likelihood, prior, MH, learning_rank, seed, last iteration
CHAINS = {
    "g70": (8, 70, 3, "poisson", "gamma", False, False, 4, 14),
    "g1100": (8, 1100, 5, "poisson", "gamma", False, False, 4, 14),
    "n9": (8, 70, 9, "poisson", "gamma", False, False, 4, 14),
    "normal": (12, 10, 3, "normal", "exponential", False, False, 4, 14),             # real-valued data, negative cells
    "ptn_mh": (96, 6, 5, "poisson", "truncnormal", True, False, 4, 14),              # rings recorded by the MH sweep
    "sbfi": (96, 8, 20, "poisson", "gamma", False, True, 14, 40),                    # samples with A[n] = 0
    "ties": (8, 70, 3, "poisson", "gamma", False, False, 4, 12),                     # sample 0 is the supplied state
}
# case: chain, include (None = all)
CASES = {
    "g70": ("g70", None),
    "m1025": ("g1100", _include(1100, 1025)),
    "m3": ("g1100", _include(1100, 3)),
    "m63": ("g1100", _include(1100, 63)),
    "m64": ("g1100", _include(1100, 64)),
    "m65": ("g1100", _include(1100, 65)),
    "m1023": ("g1100", _include(1100, 1023)),
    "m1024": ("g1100", _include(1100, 1024)),
    "n9": ("n9", _include(70, 66)),
    "normal": ("normal", None),
    "ptn_mh": ("ptn_mh", None),
    "sbfi": ("sbfi", None),
    "ties": ("ties", None),
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _data(chain):
    from bayesnmf_amd.setup import synth_counts
    K, G, N, lk, *_ = CHAINS[chain]
    if lk == "normal":
        rng = np.random.default_rng(11)
        return np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, 3)) @ rng.gamma(0.5, 1.0, size=(3, G)) + rng.normal(0.0, 0.5, size=(K, G)))
    M, _, _ = synth_counts(K, G, min(3, N), 21, mean_total=1500)
    return M


def _temps():
    return np.concatenate([np.ones(20), np.zeros(3), 10.0 ** np.linspace(-6, 0, 60), np.ones(100)])


def _create(chain):
    from bayesnmf_amd import Engine
    K, G, N, lk, prior, MH, lr, seed, _ = CHAINS[chain]
    M = _data(chain)
    return Engine(M, N, likelihood=lk, prior=prior, MH=MH, learning_rank=lr, seed=seed, window=W, temperature=_temps() if lr else None), M


def _tied_E(N, G):
    """positive multiples of 0.25, no zero: 1 .. 40 quarters, so a factor has single values, groups of 2 and of 3 or more among 70 tumours"""
    return np.asfortranarray(0.25 * np.random.default_rng(5).integers(1, 41, size=(N, G)).astype(np.float64))


def _fresh(chain):
    from bayesnmf_amd.setup import apply_hyperprior_params
    e, M = _create(chain)
    apply_hyperprior_params(e, CHAINS[chain][4], M, CHAINS[chain][2])
    if chain == "ties":
        e.set("E", _tied_E(CHAINS[chain][2], CHAINS[chain][1]))
    row1 = e.init()
    return e, M, row1


_CHAINS, _RUNS = {}, {}


def _range(chain):
    """(end_iter, n, used) of the chain's range: the ties chain starts at iteration 1, which keeps the supplied state verbatim"""
    t_end = CHAINS[chain][8]
    return (t_end, t_end, USED) if chain == "ties" else (t_end - 2, N_RANGE, USED)


def _chain(chain):
    """the chain at its last iteration, its metric rows and the used samples of the range: made once per chain"""
    if chain in _CHAINS:
        return _CHAINS[chain]
    K, G, N, lk, prior, MH, lr, _, t_end = CHAINS[chain]
    e, M, row1 = _fresh(chain)
    rows = np.vstack([row1[None, :], e.run(t_end - 1, converged=MH)])
    assert e.iter == t_end
    end, n, used = _range(chain)
    first = end - n + 1
    back = t_end - first + 1
    sel = np.where(used == 1)[0]
    win = {nm: np.stack([e.window(nm, back)[i] for i in sel]) for nm in ("P", "E", "A")}
    samples = (win["P"], win["E"], win["A"].reshape(len(sel), N))
    _CHAINS[chain] = dict(e=e, M=M, rows=rows, end=end, n=n, used=used, samples=samples)
    return _CHAINS[chain]


def _call(e, r, inc, **kw):
    kw = dict(dict(include=inc, used=r["used"], end_iter=r["end"], min_load=ML, credible_interval=CI, series=True), **kw)
    return e.coactivity(r["n"], **kw)


def _run(case):
    """the chain, the device's co-activity over the range and the restatement: made once per case"""
    if case in _RUNS:
        return _RUNS[case]
    chain, inc = CASES[case]
    ch = _chain(chain)
    ref = R.coactivity_reference(*ch["samples"], include=inc, min_load=ML, credible_interval=CI)
    dev = _call(ch["e"], ch, inc)
    _RUNS[case] = dict(ch, chain=chain, inc=inc, ref=ref, dev=dev)
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
            print(f"coactivity[{tag}] {k}: shapes {x.shape} and {y.shape}")
            bad.append(k)
            continue
        nx, ny = np.isnan(x), np.isnan(y)
        ne = (nx != ny) | (~nx & ~ny & (_bits(x).reshape(x.shape) != _bits(y).reshape(y.shape)))
        if ne.any():
            i = tuple(np.argwhere(ne)[0])
            print(f"coactivity[{tag}] {k}: {int(ne.sum())} of {ne.size} differ, first at {i}: {x[i]!r} against {y[i]!r}")
            bad.append(k)
    for k in INTS + REALS + ("n_credible",):
        if k == "n_credible":
            same = [int(v) for v in a[k]] == [int(v) for v in b[k]]
        elif k in INTS:
            same = int(a[k]) == int(b[k])
        else:
            fa, fb = float(a[k]), float(b[k])
            same = (np.isnan(fa) and np.isnan(fb)) or _bits(fa) == _bits(fb)
        if not same:
            print(f"coactivity[{tag}] {k}: {a[k]!r} against {b[k]!r}")
            bad.append(k)
    return bad


def _same(a, b, arrays=ARRAYS):
    assert not _differences("equivalence", a, b, arrays)


@pytest.mark.parametrize("case", list(CASES))
def test_every_output_is_the_restatement_bit_for_bit(case):
    r = _run(case)
    chain, inc = CASES[case]
    K, G, N, *_ = CHAINS[chain]
    dev, ref, e = r["dev"], r["ref"], r["e"]
    A = r["samples"][2]
    S, NP = int(r["used"].sum()), N * (N - 1) // 2
    print(f"coactivity[{case}] S {dev['n_used']} included {dev['n_included']} left out {dev['n_left_out']} pairs {dev['n_pairs']} blocks {dev['n_blocks']} "
          f"n_credible {dev['n_credible']} max_cosine {dev['max_cosine']:.4g} at {dev['max_cosine_at']}; samples that exclude a factor "
          f"{int((A == 0).any(axis=1).sum())}; NaN in the series {np.isnan(dev['series']).sum(axis=(1, 2)).tolist()}")
    m = G if inc is None else int(inc.sum())
    assert ref["n_included"] == m and ref["n_blocks"] == (m + 1023) // 1024
    if case == "m1025":
        assert ref["n_blocks"] == 2 and (np.diff(np.where(inc == 1)[0]) > 1).any(), "the members are contiguous"
    if case == "sbfi":
        nv = ref["pair"][:, 6]
        assert (A == 0).any() and (nv < S).any() and (nv >= 2).any(), "the chain has no sample that excludes a factor, or no pair left"
    if case == "normal":
        assert (np.asarray(r["M"]) < 0).any(), "no negative cell"
    if case == "ties":
        x0 = ref["x"][0]                                                            # sample 0: the supplied E times the column sums
        sizes = np.concatenate([np.unique(x0[n], return_counts=True)[1] for n in range(N)])
        assert (sizes == 2).any() and (sizes >= 3).any(), "no tie groups in the first sample"
        assert np.array_equal(r["samples"][1][0], _tied_E(N, G)), "iteration 1 did not keep the supplied E"
    assert dev["n_used"] == S and dev["pair"].shape == (4, 7, NP) and dev["series"].shape == (4, S, NP) and dev["pairs"] == ref["pairs"]
    bad = _differences(case, dev, ref)
    # no interval: NaN bounds, nothing counted; another interval
    for ci in (0.0, -1.0, 0.5):
        d = _call(e, r, inc, credible_interval=ci)
        bad += _differences(f"{case}, interval {ci:g}", d, R.coactivity_reference(*r["samples"], include=inc, min_load=ML, credible_interval=ci))
        if ci <= 0:
            assert np.isnan(d["pair"][:, 2:4]).all() and d["n_credible"] == [0, 0, 0]
    assert not bad, bad


def _reopened(r, tmp_path):
    """the chain of r in a fresh handle (saved and loaded)"""
    path = str(tmp_path / "state.bin")
    r["e"].save_state(path)
    c, _ = _create(r["chain"])
    assert c.load_state(path) == CHAINS[r["chain"]][8]
    return c


FORMS = [dict(BNMF_COA_CHUNK="64"), dict(BNMF_COA_CHUNK="256"), dict(BNMF_COA_BATCH="1"), dict(BNMF_COA_BATCH="3"), dict(BNMF_COA_FORM="1"),
         dict(BNMF_COA_FORM="0"), dict(BNMF_COA_FORM="1", BNMF_COA_CHUNK="256", BNMF_COA_BATCH="3"), dict(BNMF_COA_WIDTH="256")]


@pytest.mark.parametrize("case", ["m1025", "n9", "ties", "sbfi"])
def test_every_form_gives_the_same_bits(case, tmp_path, monkeypatch):
    """the chunk of the sort (several chunks and a padded last one), the batch of samples, the narrow tiles with the ranks through the
    scratch, the width of the sorting workgroup: each in a fresh handle, each the bits of the restatement"""
    r = _run(case)
    bad = []
    for env in FORMS:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        c = _reopened(r, tmp_path)
        bad += _differences(f"{case}, {env}", _call(c, r, r["inc"]), r["ref"])
        c.close()
        for k in env:
            monkeypatch.delenv(k)
    assert not bad, bad


def _raw(e, r, inc, skip=()):
    """bnmf_coactivity_at through ctypes with the outputs in `skip` NULL -> (the Engine.coactivity layout of the others, the untouched buffers)"""
    from bayesnmf_amd.engine import lib, BnmfCoactivityInfo
    L, dp, ip = lib(), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    N, S = e.N, int(r["used"].sum())
    NP = N * (N - 1) // 2
    bufs = dict(pair=np.full((4, 7, NP), -7.0), series=np.full((4, S, NP), -7.0))
    ptr = {k: (None if k in skip else v.ctypes.data_as(dp)) for k, v in bufs.items()}
    info = BnmfCoactivityInfo()
    assert L.bnmf_coactivity_at(e._h, r["end"], r["n"], r["used"].ctypes.data_as(ip), None if inc is None else inc.ctypes.data_as(ip), ML, CI,
                                ptr["pair"], ptr["series"], C.byref(info)) == 0
    got = dict(bufs, n_credible=[int(v) for v in info.n_credible], **{k: getattr(info, k) for k in INTS + REALS})
    return got, bufs


@pytest.mark.parametrize("case", ["m1025", "sbfi", "normal"])
def test_equivalent_calls_give_the_same_bits(case, tmp_path):
    r = _run(case)
    e, end, inc, n, used = r["e"], r["end"], r["inc"], r["n"], r["used"]
    G = CHAINS[r["chain"]][1]
    kw = dict(include=inc, min_load=ML, credible_interval=CI, series=True)
    _same(r["dev"], _call(e, r, inc))                                                                   # a second call
    _same(e.coactivity(10, **kw), e.coactivity_at(e.iter, 10, **kw))                                    # bnmf_coactivity is bnmf_coactivity_at(iter)
    _same(e.coactivity(10, **kw), e.coactivity(10, used=np.ones(10, dtype=np.int32), **kw))             # NULL used is all ones
    _same(_call(e, r, None), _call(e, r, np.ones(G, dtype=np.int32)))                                   # NULL include too
    # the series of a sub-range are the matching rows of the full range's: through _at, and through used[] with gaps
    full = e.coactivity_at(end, n, **kw)["series"]
    assert np.array_equal(_bits(np.nan_to_num(r["dev"]["series"], nan=-9.0)), _bits(np.nan_to_num(full[:, used == 1], nan=-9.0)))
    sub = e.coactivity_at(end - 2, n - 5, **kw)["series"]
    assert np.array_equal(_bits(np.nan_to_num(sub, nan=-9.0)), _bits(np.nan_to_num(full[:, 3:n - 2], nan=-9.0)))
    # min_load moves the co-presence alone
    other = _call(e, r, inc, min_load=25.0)
    assert other["min_load"] == 25.0
    for q in (0, 1, 3):
        assert not _differences(f"min_load, statistic {q}", dict(r["dev"], pair=other["pair"][q], series=other["series"][q]),
                                dict(r["dev"], pair=r["dev"]["pair"][q], series=r["dev"]["series"][q]))
    assert not _differences("min_load against the restatement", other, R.coactivity_reference(*r["samples"], include=inc, min_load=25.0, credible_interval=CI))
    # each output NULL in turn, then both: the other and the info fields are the same
    for skip in [(k,) for k in ARRAYS] + [ARRAYS]:
        got, bufs = _raw(e, r, inc, skip)
        for k in skip:
            assert (bufs[k] == -7).all(), k                                                             # (not written)
        _same(got, r["dev"], tuple(k for k in ARRAYS if k not in skip))
    # a chain reopened with bnmf_load_state
    c = _reopened(r, tmp_path)
    _same(r["dev"], _call(c, r, inc))
    c.close()


def test_refusals():
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import lib, BnmfCoactivityInfo, BnmfError
    from bayesnmf_amd.setup import apply_hyperprior_params
    r = _run("g70")
    e, M, L = r["e"], r["M"], lib()
    G = 70
    info = BnmfCoactivityInfo()
    ip = C.POINTER(C.c_int32)

    def err():
        msg = L.bnmf_last_error().decode()
        assert msg
        return msg

    def call(n=10, used=None, include=None, ml=1.0, ci=0.9, inf=info, at=None, h=None):
        u = None if used is None else used.ctypes.data_as(ip)
        c = None if include is None else include.ctypes.data_as(ip)
        i = None if inf is None else C.byref(inf)
        h = e._h if h is None else h
        if at is None:
            return L.bnmf_coactivity(h, n, u, c, ml, ci, None, None, i)
        return L.bnmf_coactivity_at(h, at, n, u, c, ml, ci, None, None, i)

    for at in (None, e.iter):
        assert call(inf=None, at=at) == -1 and "null" in err()                                       # BNMF_EINVAL
        u = np.ones(10, dtype=np.int32); u[6] = 2
        assert call(used=u, at=at) == -1 and "used[6] = 2" in err()
        c = np.ones(G, dtype=np.int32); c[11] = 2
        assert call(include=c, at=at) == -1 and "include[11] = 2" in err()
        c[11] = -1
        assert call(include=c, at=at) == -1 and "include[11] = -1" in err()
        for bad in (float("nan"), float("inf"), -1.0):
            assert call(ml=bad, at=at) == -1 and "min_load" in err()
        for bad in (float("nan"), 1.0, 1.5, float("inf")):
            assert call(ci=bad, at=at) == -1 and "credible_interval" in err()
        u = np.zeros(10, dtype=np.int32); u[3] = 1
        assert call(used=u, at=at) == -2 and "1 used sample" in err()                                # BNMF_ESIZE
        assert call(include=_include(G, 2), at=at) == -2 and "2 included tumours" in err()
        assert call(include=np.zeros(G, dtype=np.int32), at=at) == -2 and "0 included tumours" in err()
        assert call(include=_include(G, 3), at=at) == 0
        # the order among them is bnmf_regress's: used, include, then the numbers, then the sizes
        c = np.ones(G, dtype=np.int32); c[11] = 2
        assert call(used=u, include=c, ml=-1.0, at=at) == -1 and "include[11]" in err()
        assert call(used=u, ml=-1.0, ci=2.0, at=at) == -1 and "min_load" in err()
        assert call(used=u, ci=2.0, include=_include(G, 2), at=at) == -1 and "credible_interval" in err()
        assert call(used=u, include=_include(G, 2), at=at) == -2 and "1 used sample" in err()
    assert call(n=1) == -2 and err()
    assert call(n=W + 1) == -2 and err()
    # the range rule of bnmf_waic_at: iterations [max(1, iter - window + 1), iter]
    assert call(n=5, at=e.iter + 1) == -2 and "are kept" in err()
    assert call(n=W + 1, at=e.iter) == -2 and "are kept" in err()
    with pytest.raises(BnmfError, match="used has 3 entries"):
        e.coactivity(10, used=[1, 1, 1])
    with pytest.raises(BnmfError, match="G = 70 flags are needed"):
        e.coactivity(10, include=[1, 1])
    # N < 2: BNMF_ESIZE;  window = 0: BNMF_ESTATE
    for N1, win, code, word in ((1, W, -2, "N = 1"), (3, 0, -7, "window = 0")):
        z = Engine(M, N1, prior="gamma", seed=4, window=win)
        apply_hyperprior_params(z, "gamma", M, N1)
        z.init(); z.run(5)
        assert call(n=3, h=z._h) == code and word in err()
        assert call(n=3, at=z.iter, h=z._h) == code and word in err()
        z.close()
    # more than 1,000,000 tumours: refused on a chain of one mutation type, before any device work
    big = Engine(np.ones((1, 1000001), dtype=np.int32), 2, prior="gamma", seed=4, window=2)
    apply_hyperprior_params(big, "gamma", np.ones((1, 1000001), dtype=np.int32), 2)
    big.init(); big.run(1)
    assert call(n=2, h=big._h) == -2 and "1000001 included tumours" in err()
    big.close()
    assert call(ci=0.0) == 0 and info.n_credible[0] == 0 and info.n_included == G and info.n_blocks == 1 and info.n_pairs == 3   # no interval is allowed
    assert call(ci=-3.0) == 0
    # the handle is usable afterwards: the same bits as before the refusals
    _same(r["dev"], _call(e, r, r["inc"]))


@pytest.mark.parametrize("case", ["n9", "ptn_mh", "sbfi"])
def test_the_call_is_read_only_for_the_chain(case):
    """a chain that calls coactivity mid-run continues with the bits of a twin that never did"""
    r = _run(case)
    chain = r["chain"]
    MH, t_end = CHAINS[chain][5], CHAINS[chain][8]
    b, _, row1 = _fresh(chain)
    rows_b = np.vstack([row1[None, :], b.run(t_end - 1, converged=MH)])
    assert np.array_equal(_bits(rows_b), _bits(r["rows"]))
    more_a, more_b = r["e"].run(5, converged=MH), b.run(5, converged=MH)         # a called coactivity, b never did
    assert np.array_equal(_bits(more_a), _bits(more_b))
    for nm in ("P", "E", "A"):
        assert np.array_equal(_bits(r["e"].get(nm)), _bits(b.get(nm))), nm
    b.close()
    _CHAINS.pop(chain)["e"].close()                                              # (this chain has moved on)
    for c in [c for c in _RUNS if CASES[c][0] == chain]:
        _RUNS.pop(c)
