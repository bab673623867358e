"""Cohort summary of signatures over a recorded range on the device (bnmf_summary / bnmf_summary_at, csrc/summary.h) against the
numerical spec restated in numpy float64 (tests/summary_ref.py, written from DESIGN.md 29): stat, series and every info field of every
case bit for bit, NaN compared as NaN, no tolerance — the operations are + - * /, comparisons and counts only and an order statistic is
exact; then the forms, the equivalences and the refusals.

Every chain runs to iteration 40 with window = 16; the range is the 12 samples that end 2 iterations before `iter`, so it wraps the ring,
with a `used` mask that has gaps.  The shapes are the smallest that reach each path: K = 8, N = 3 with 1, 2, 63, 64 and 65 members (one
key, a pair, the padding of 64 keys by one, none, and 128 keys); N = 5 with 1,023, 1,024 and 1,025 of G = 1,100 tumours in a fixed shuffle
(the block boundary of canonB, 1,024 and 2,048 keys); the general form forced with chunks of 64 at 200 and 1,025 members (a padded last
chunk, 4 and 17 chunks); a fixed-rank chain with excluded factors; real-valued data with negative cells."""
import ctypes as C

import numpy as np
import pytest

import summary_ref as R

pytestmark = pytest.mark.gpu

W, N_RANGE, T_END = 16, 12, 40
USED = np.array([1, 1, 0, 1, 1, 1, 0, 0, 1, 1, 1, 1], dtype=np.int32)
ARRAYS = ("stat", "series")
INTS = ("n_used", "n_aligned", "n_included", "n_left_out", "n_levels", "n_blocks", "n_nonfinite")
REALS = ("min_load", "credible_interval")
CI, ML = 0.9, 1.0
PROBS = (0.05, 0.25, 0.5, 0.75, 0.95)
PROBS8 = (0.0, 0.1, 0.3, 0.5, 0.625, 0.8, 0.99, 1.0)


def _include(G, m, seed=17):
    """m of the G tumours in a fixed shuffle"""
    inc = np.zeros(G, dtype=np.int32)
    inc[np.random.default_rng(seed).permutation(G)[:m]] = 1
    return inc


# chain: K, G, N, likelihood, prior, supplied A (None = all ones), seed
CHAINS = {
    "g70": (8, 70, 3, "poisson", "gamma", None, 4),
    "g1100": (8, 1100, 5, "poisson", "gamma", None, 4),
    "excluded": (8, 70, 5, "poisson", "gamma", [1.0, 0.0, 1.0, 1.0, 0.0], 12),          # the rank is not learned: factors 1 and 4 stay out
    "normal": (12, 10, 3, "normal", "exponential", None, 4),                            # real-valued data, negative cells
}
# case: chain, include (None = all), probs
CASES = {
    "g70": ("g70", None, PROBS),
    "m1": ("g70", _include(70, 1), PROBS),
    "m2": ("g70", _include(70, 2), PROBS),
    "m63": ("g70", _include(70, 63), PROBS),
    "m64": ("g70", _include(70, 64), PROBS),
    "m65": ("g70", _include(70, 65), PROBS8),
    "m200": ("g1100", _include(1100, 200), PROBS),
    "m1023": ("g1100", _include(1100, 1023), PROBS),
    "m1024": ("g1100", _include(1100, 1024), (0.5,)),
    "m1025": ("g1100", _include(1100, 1025), PROBS8),
    "excluded": ("excluded", None, PROBS),
    "normal": ("normal", None, PROBS),
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


def _create(chain):
    from bayesnmf_amd import Engine
    K, G, N, lk, prior, A0, seed = CHAINS[chain]
    M = _data(chain)
    return Engine(M, N, likelihood=lk, prior=prior, seed=seed, window=W), M


def _fresh(chain):
    from bayesnmf_amd.setup import apply_hyperprior_params
    K, G, N, lk, prior, A0, seed = CHAINS[chain]
    e, M = _create(chain)
    apply_hyperprior_params(e, prior, M, N)
    if A0 is not None:
        e.set("A", np.array([A0]))
    e.init()
    return e, M


_CHAINS, _RUNS = {}, {}


def _chain(chain):
    """the chain at iteration 40 and the used samples of the range: made once per chain"""
    if chain in _CHAINS:
        return _CHAINS[chain]
    N = CHAINS[chain][2]
    e, M = _fresh(chain)
    e.run(T_END - 1)
    assert e.iter == T_END
    end, n = T_END - 2, N_RANGE
    back = T_END - (end - n + 1) + 1
    sel = np.where(USED == 1)[0]
    win = {nm: np.stack([e.window(nm, back)[i] for i in sel]) for nm in ("P", "E", "A")}
    _CHAINS[chain] = dict(e=e, M=M, end=end, n=n, used=USED, samples=(win["P"], win["E"], win["A"].reshape(len(sel), N)))
    return _CHAINS[chain]


def _call(e, r, inc, probs=PROBS, **kw):
    kw = dict(dict(probs=probs, include=inc, used=r["used"], end_iter=r["end"], min_load=ML, credible_interval=CI, series=True), **kw)
    return e.summary(r["n"], **kw)


def _run(case):
    """the chain, the device's summary over the range and the restatement: made once per case"""
    if case in _RUNS:
        return _RUNS[case]
    chain, inc, probs = CASES[case]
    ch = _chain(chain)
    ref = R.summary_reference(*ch["samples"], probs=probs, include=inc, min_load=ML, credible_interval=CI)
    dev = _call(ch["e"], ch, inc, probs)
    _RUNS[case] = dict(ch, chain=chain, inc=inc, probs=probs, ref=ref, dev=dev)
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
            print(f"summary[{tag}] {k}: shapes {x.shape} and {y.shape}")
            bad.append(k)
            continue
        nx, ny = np.isnan(x), np.isnan(y)
        ne = (nx != ny) | (~nx & ~ny & (_bits(x).reshape(x.shape) != _bits(y).reshape(y.shape)))
        if ne.any():
            i = tuple(np.argwhere(ne)[0])
            print(f"summary[{tag}] {k}: {int(ne.sum())} of {ne.size} differ, first at {i}: {x[i]!r} against {y[i]!r}")
            bad.append(k)
    for k in INTS + REALS:
        same = int(a[k]) == int(b[k]) if k in INTS else _bits(float(a[k])) == _bits(float(b[k]))
        if not same:
            print(f"summary[{tag}] {k}: {a[k]!r} against {b[k]!r}")
            bad.append(k)
    return bad


def _same(a, b, arrays=ARRAYS):
    assert not _differences("equivalence", a, b, arrays)


@pytest.mark.parametrize("case", list(CASES))
def test_every_output_is_the_restatement_bit_for_bit(case):
    r = _run(case)
    chain, inc, probs = CASES[case]
    K, G, N, *_ = CHAINS[chain]
    dev, ref, e = r["dev"], r["ref"], r["e"]
    A = r["samples"][2]
    S, L = int(r["used"].sum()), len(probs)
    m = G if inc is None else int(inc.sum())
    print(f"summary[{case}] S {dev['n_used']} aligned {dev['n_aligned']} included {dev['n_included']} blocks {dev['n_blocks']} levels {dev['n_levels']} "
          f"nonfinite {dev['n_nonfinite']}; samples that exclude a factor {int((A == 0).any(axis=1).sum())}; NaN in the series "
          f"{int(np.isnan(dev['series']).sum())}; mean prevalence {dev['stat'][0, 0].round(3).tolist()}")
    assert ref["n_included"] == m and ref["n_blocks"] == (m + 1023) // 1024 and dev["names"] == ref["names"] and len(ref["names"]) == 4 + 3 * L
    assert dev["n_used"] == S and dev["stat"].shape == (4 + 3 * L, 5, N) and dev["series"].shape == (4 + 3 * L, S, N)
    if case == "m1025":
        assert ref["n_blocks"] == 2 and (np.diff(np.where(inc == 1)[0]) > 1).any(), "the members are contiguous"
    if case == "excluded":
        assert (A[:, [1, 4]] == 0).all() and (A[:, [0, 2, 3]] != 0).all(), "the supplied A did not hold"
        assert (ref["series"][1][:, [1, 4]] == 0).all() and (ref["series"][4:4 + L][:, :, [1, 4]] == 0).all()       # every load is +0.0
        assert np.isnan(ref["series"][4 + L:4 + 2 * L][:, :, [1, 4]]).all(), "an excluded factor has carriers"
    if case == "normal":
        assert (np.asarray(r["M"]) < 0).any(), "no negative cell"
    bad = _differences(case, dev, ref)
    # min_load 0: every tumour is a carrier, the suffix is the whole set; a min_load above every load: no carrier
    top = float(np.nanmax(ref["x"])) * 2.0 + 1.0
    for ml in (0.0, top):
        d = _call(e, r, inc, probs, min_load=ml)
        f = R.summary_reference(*r["samples"], probs=probs, include=inc, min_load=ml, credible_interval=CI)
        bad += _differences(f"{case}, min_load {ml:g}", d, f)
        if ml == 0.0 and (ref["x"] < 0).any():
            assert (d["series"][0] < 1.0).any()                                     # a negative load is no carrier at min_load 0
        elif ml == 0.0:
            assert (d["series"][0] == 1.0).all() and np.array_equal(_bits(d["series"][4:4 + L]), _bits(d["series"][4 + L:4 + 2 * L]))
        else:
            assert (d["series"][0] == 0.0).all() and np.isnan(d["series"][3]).all() and np.isnan(d["series"][4 + L:4 + 2 * L]).all()
            assert (d["stat"][3, 4] == 0).all() and np.isnan(d["stat"][3, :4]).all() and (d["stat"][4 + L:4 + 2 * L, 4] == 0).all()
    # no interval: NaN bounds; another interval
    for ci in (0.0, 0.5):
        d = _call(e, r, inc, probs, credible_interval=ci)
        bad += _differences(f"{case}, interval {ci:g}", d, R.summary_reference(*r["samples"], probs=probs, include=inc, min_load=ML, credible_interval=ci))
        if ci <= 0:
            assert np.isnan(d["stat"][:, 2:4]).all()
    assert not bad, bad


def _reopened(r, tmp_path):
    """the chain of r in a fresh handle (saved and loaded)"""
    path = str(tmp_path / "state.bin")
    r["e"].save_state(path)
    c, _ = _create(r["chain"])
    assert c.load_state(path) == T_END
    return c


FORMS = [dict(BNMF_SUM_CHUNK="64"), dict(BNMF_SUM_BATCH="5"), dict(BNMF_SUM_CHUNK="64", BNMF_SUM_BATCH="5"), dict(BNMF_SUM_CHUNK="256", BNMF_SUM_BATCH="1")]


@pytest.mark.parametrize("case", ["m200", "m1025", "m65", "excluded", "normal"])
def test_every_form_gives_the_same_bits(case, tmp_path, monkeypatch):
    """the general form through sorted chunks of 64 (several chunks and a padded last one) and the batch of samples: each in a fresh
    handle, each the bits of the one-chunk form and of the restatement"""
    r = _run(case)
    bad = []
    for env in FORMS:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        c = _reopened(r, tmp_path)
        d = _call(c, r, r["inc"], r["probs"])
        bad += _differences(f"{case}, {env}, against the one-chunk form", d, r["dev"]) + _differences(f"{case}, {env}", d, r["ref"])
        c.close()
        for k in env:
            monkeypatch.delenv(k)
    assert not bad, bad


def _perm(N, S_range, swapped, left):
    """the identity but for sample `swapped` of the range (factors 0 and 1 exchanged) and sample `left` (left out)"""
    pm = np.tile(np.arange(N, dtype=np.int32), (S_range, 1))
    pm[swapped, [0, 1]] = [1, 0]
    pm[left] = -1
    return pm


@pytest.mark.parametrize("case", ["g70", "m1025"])
def test_perm_moves_the_values_to_their_labels(case, monkeypatch, tmp_path):
    r = _run(case)
    e, inc, probs = r["e"], r["inc"], r["probs"]
    N = CHAINS[r["chain"]][2]
    pm = _perm(N, r["n"], 3, 8)                                                       # both are used samples
    assert r["used"][3] == 1 and r["used"][8] == 1
    dev = _call(e, r, inc, probs, perm=pm)
    ref = R.summary_reference(*r["samples"], probs=probs, include=inc, perm=pm[r["used"] == 1], min_load=ML, credible_interval=CI)
    assert dev["n_aligned"] == dev["n_used"] - 1
    assert not _differences(f"{case}, perm", dev, ref)
    rows = np.where(r["used"] == 1)[0]
    s_sw, s_out = int(np.where(rows == 3)[0][0]), int(np.where(rows == 8)[0][0])
    base = r["dev"]["series"]
    assert np.isnan(dev["series"][:, s_out]).all() and (dev["stat"][:, 4] == dev["n_used"] - 1).all()
    assert np.array_equal(_bits(np.nan_to_num(dev["series"][:, s_sw][:, [1, 0]], nan=-9.0)), _bits(np.nan_to_num(base[:, s_sw][:, [0, 1]], nan=-9.0)))
    keep = [s for s in range(len(rows)) if s not in (s_sw, s_out)]
    assert np.array_equal(_bits(np.nan_to_num(dev["series"][:, keep], nan=-9.0)), _bits(np.nan_to_num(base[:, keep], nan=-9.0)))
    # the identity given in full is NULL
    _same(r["dev"], _call(e, r, inc, probs, perm=np.tile(np.arange(N, dtype=np.int32), (r["n"], 1))))
    if case == "m1025":                                                              # the general form puts a value at its label too
        monkeypatch.setenv("BNMF_SUM_CHUNK", "64")
        c = _reopened(r, tmp_path)
        assert not _differences(f"{case}, perm, chunks of 64", _call(c, r, inc, probs, perm=pm), ref)
        c.close()


def _raw(e, r, inc, probs, skip=()):
    """bnmf_summary_at through ctypes with the outputs in `skip` NULL -> (the Engine.summary layout of the others, the untouched buffers)"""
    from bayesnmf_amd.engine import lib, BnmfSummaryInfo
    L, dp, ip = lib(), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    N, S, nl = e.N, int(r["used"].sum()), len(probs)
    bufs = dict(stat=np.full((4 + 3 * nl, 5, N), -7.0), series=np.full((4 + 3 * nl, S, N), -7.0))
    ptr = {k: (None if k in skip else v.ctypes.data_as(dp)) for k, v in bufs.items()}
    pr = np.asarray(probs, dtype=np.float64)
    info = BnmfSummaryInfo()
    assert L.bnmf_summary_at(e._h, r["end"], r["n"], r["used"].ctypes.data_as(ip), None if inc is None else inc.ctypes.data_as(ip), None, ML, pr.ctypes.data_as(dp),
                             nl, CI, ptr["stat"], ptr["series"], C.byref(info)) == 0
    return dict(bufs, **{k: getattr(info, k) for k in INTS + REALS}), bufs


@pytest.mark.parametrize("case", ["m1025", "excluded", "normal"])
def test_equivalent_calls_give_the_same_bits(case, tmp_path):
    r = _run(case)
    e, end, inc, n, used, probs = r["e"], r["end"], r["inc"], r["n"], r["used"], r["probs"]
    G = CHAINS[r["chain"]][1]
    kw = dict(probs=probs, include=inc, min_load=ML, credible_interval=CI, series=True)
    _same(r["dev"], _call(e, r, inc, probs))                                                        # a second call
    _same(e.summary(10, **kw), e.summary_at(e.iter, 10, **kw))                                      # bnmf_summary is bnmf_summary_at(iter)
    _same(e.summary(10, **kw), e.summary(10, used=np.ones(10, dtype=np.int32), **kw))               # NULL used is all ones
    _same(_call(e, r, None, probs), _call(e, r, np.ones(G, dtype=np.int32), probs))                 # NULL include too
    # the series of a sub-range are the matching rows of the full range's
    full = e.summary_at(end, n, **kw)["series"]
    assert np.array_equal(_bits(np.nan_to_num(r["dev"]["series"], nan=-9.0)), _bits(np.nan_to_num(full[:, used == 1], nan=-9.0)))
    sub = e.summary_at(end - 2, n - 5, **kw)["series"]
    assert np.array_equal(_bits(np.nan_to_num(sub, nan=-9.0)), _bits(np.nan_to_num(full[:, 3:n - 2], nan=-9.0)))
    # a level's values do not depend on the other levels: L = 1 against its row among the L levels
    at = len(probs) // 2
    one = _call(e, r, inc, (probs[at],))
    nl = len(probs)
    assert one["n_levels"] == 1 and one["stat"].shape[0] == 7
    for fam in range(3):
        assert np.array_equal(_bits(np.nan_to_num(one["series"][4 + fam], nan=-9.0)), _bits(np.nan_to_num(r["dev"]["series"][4 + fam * nl + at], nan=-9.0)))
    # each output NULL in turn, then both: the other and the info fields are the same
    for skip in [(k,) for k in ARRAYS] + [ARRAYS]:
        got, bufs = _raw(e, r, inc, probs, skip)
        for k in skip:
            assert (bufs[k] == -7).all(), k                                                         # (not written)
        _same(got, r["dev"], tuple(k for k in ARRAYS if k not in skip))
    # a chain reopened with bnmf_load_state
    c = _reopened(r, tmp_path)
    _same(r["dev"], _call(c, r, inc, probs))
    c.close()


def test_refusals_and_the_version():
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import lib, BnmfSummaryInfo, BnmfError
    from bayesnmf_amd.setup import apply_hyperprior_params
    r = _run("g70")
    e, M, L = r["e"], r["M"], lib()
    assert L.bnmf_version() == 100
    G, N = 70, 3
    info = BnmfSummaryInfo()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)

    def err():
        msg = L.bnmf_last_error().decode()
        assert msg
        return msg

    def call(n=10, used=None, include=None, perm=None, ml=1.0, probs=(0.5,), nl=None, ci=0.9, inf=info, at=None, h=None):
        u = None if used is None else used.ctypes.data_as(ip)
        c = None if include is None else include.ctypes.data_as(ip)
        p = None if perm is None else perm.ctypes.data_as(ip)
        pr = None if probs is None else np.asarray(probs, dtype=np.float64)
        q = None if pr is None else pr.ctypes.data_as(dp)
        nl = (0 if pr is None else pr.size) if nl is None else nl
        i = None if inf is None else C.byref(inf)
        h = e._h if h is None else h
        if at is None:
            return L.bnmf_summary(h, n, u, c, p, ml, q, nl, ci, None, None, i)
        return L.bnmf_summary_at(h, at, n, u, c, p, ml, q, nl, ci, None, None, i)

    for at in (None, e.iter):
        assert call(inf=None, at=at) == -1 and "null" in err()                                       # BNMF_EINVAL
        assert call(probs=None, nl=1, at=at) == -1 and "null" in err()
        u = np.ones(10, dtype=np.int32); u[6] = 2
        assert call(used=u, at=at) == -1 and "used[6] = 2" in err()
        c = np.ones(G, dtype=np.int32); c[11] = 2
        assert call(include=c, at=at) == -1 and "include[11] = 2" in err()
        pm = np.tile(np.arange(N, dtype=np.int32), (10, 1)); pm[4] = [0, 0, 2]
        assert call(perm=pm, at=at) == -1 and "perm[4]" in err()
        pm[4] = [0, 1, 3]
        assert call(perm=pm, at=at) == -1 and "perm[4]" in err()
        pm[4] = [-1, 1, 2]
        assert call(perm=pm, at=at) == -1 and "perm[4]" in err()
        for bad in (float("nan"), float("inf"), -1.0):
            assert call(ml=bad, at=at) == -1 and "min_load" in err()
        assert call(probs=(0.5,), nl=0, at=at) == -1 and "L = 0" in err()
        assert call(probs=tuple(np.linspace(0, 1, 9)), at=at) == -1 and "L = 9" in err()
        assert call(probs=(0.1, float("nan")), at=at) == -1 and "probs[1]" in err()
        assert call(probs=(-0.1, 0.5), at=at) == -1 and "probs[0]" in err()
        assert call(probs=(0.1, 1.5), at=at) == -1 and "probs[1]" in err()
        assert call(probs=(0.1, 0.5, 0.5), at=at) == -1 and "probs[2]" in err()
        assert call(probs=(0.5, 0.1), at=at) == -1 and "probs[1]" in err()
        for bad in (float("nan"), 1.0, 1.5, float("inf")):
            assert call(ci=bad, at=at) == -1 and "credible_interval" in err()
        u = np.zeros(10, dtype=np.int32); u[3] = 1
        assert call(used=u, at=at) == -2 and "1 used sample" in err()                                # BNMF_ESIZE
        pm = np.full((10, N), -1, dtype=np.int32); pm[2] = [2, 0, 1]
        assert call(perm=pm, at=at) == -2 and "1 aligned sample" in err()
        assert call(include=np.zeros(G, dtype=np.int32), at=at) == -2 and "no included tumour" in err()
        assert call(include=_include(G, 1), at=at) == 0
        # the order among them: used, include, perm, then the numbers, then the sizes
        c = np.ones(G, dtype=np.int32); c[11] = 2
        assert call(used=u, include=c, ml=-1.0, at=at) == -1 and "include[11]" in err()
        assert call(used=u, ml=-1.0, probs=(2.0,), at=at) == -1 and "min_load" in err()
        assert call(used=u, probs=(2.0,), ci=2.0, at=at) == -1 and "probs[0]" in err()
        assert call(used=u, ci=2.0, at=at) == -1 and "credible_interval" in err()
    assert call(n=1) == -2 and err()
    assert call(n=W + 1) == -2 and err()
    # the range rule of bnmf_waic_at: iterations [max(1, iter - window + 1), iter]
    assert call(n=5, at=e.iter + 1) == -2 and "are kept" in err()
    assert call(n=W + 1, at=e.iter) == -2 and "are kept" in err()
    with pytest.raises(BnmfError, match="used has 3 entries"):
        e.summary(10, used=[1, 1, 1])
    with pytest.raises(BnmfError, match="G = 70 flags are needed"):
        e.summary(10, include=[1, 1])
    with pytest.raises(BnmfError, match="perm is"):
        e.summary(10, perm=np.zeros((3, 3), dtype=np.int32))
    z = Engine(M, 3, prior="gamma", seed=4, window=0)                                                # window = 0: BNMF_ESTATE
    apply_hyperprior_params(z, "gamma", M, 3)
    z.init(); z.run(5)
    assert call(n=3, h=z._h) == -7 and "window = 0" in err()
    assert call(n=3, at=z.iter, h=z._h) == -7 and "window = 0" in err()
    z.close()
    # more than 1,000,000 tumours: refused on a chain of one mutation type, before any device work
    big = Engine(np.ones((1, 1000001), dtype=np.int32), 2, prior="gamma", seed=4, window=2)
    apply_hyperprior_params(big, "gamma", np.ones((1, 1000001), dtype=np.int32), 2)
    big.init(); big.run(1)
    assert call(n=2, h=big._h) == -2 and "1000001 included tumours" in err()
    big.close()
    assert call(ci=0.0) == 0 and info.n_included == G and info.n_blocks == 1 and info.n_levels == 1 and info.n_aligned == 10   # no interval is allowed
    assert call(ci=-3.0) == 0
    # the handle is usable afterwards: the same bits as before the refusals
    _same(r["dev"], _call(e, r, r["inc"], r["probs"]))


@pytest.mark.parametrize("case", ["m1025", "excluded", "normal"])
def test_the_call_is_read_only_for_the_chain(case):
    """a chain that called summary continues with the bits of a twin that never did"""
    r = _run(case)
    chain = r["chain"]
    b, _ = _fresh(chain)
    b.run(T_END - 1)
    more_a, more_b = r["e"].run(1), b.run(1)                                         # a called summary, b never did
    assert np.array_equal(_bits(more_a), _bits(more_b))
    for nm in ("P", "E", "A"):
        assert np.array_equal(_bits(r["e"].get(nm)), _bits(b.get(nm))), nm
    b.close()
    _CHAINS.pop(chain)["e"].close()                                                  # (this chain has moved on)
    for c in [c for c in _RUNS if CASES[c][0] == chain]:
        _RUNS.pop(c)
