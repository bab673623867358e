"""Subtypes of tumours over a recorded range on the device (bnmf_subtypes / bnmf_subtypes_at, csrc/subtypes.h) against the numerical
spec restated in numpy float64 (tests/subtypes_ref.py, written from DESIGN.md 25): every output and every info field of every case bit
for bit, NaN compared as NaN, no tolerance — the operations are + - * /, comparisons and whole numbers only; then the equivalences and
the refusals.

Every case keeps window = 16 samples and runs to iteration 40, so the kept range wraps the ring; the range is the 12 samples that end 2
iterations before `iter`, with a `used` mask that has gaps (tests/test_gpu_contrast.py's recipe).  The shapes are the smallest that
reach each path of the kernel:
  G = 200, N = 5 with C = 2 and 3: the form for small N C (N <= 8 and C <= 4), one tile;
  the same chain with C = 5: the tiled form, one chunk of 8 clusters; with C = 9: two chunks of clusters and two tiles of clusters;
  G = 1,100: the member list crosses a block of 1,024 positions with a ragged last block (also with tumours left out on both sides of
  the boundary);
  G = 8,300: 9 blocks of positions, so the 8 waves take a second round of blocks and the running sums are carried across rounds;
  N = 128 with C = 32: the largest N and C, N C = 4,096 centres in the LDS (the strided loops over more than 512 lanes' worth), 32 tiles
  of factors by 4 of clusters, 4 chunks of clusters (10 steps at most: the restatement loops over N C);
  a rank-learning chain with N = 20 (five tiles of factors, samples with A[n] = 0 and one with A all zero: every tumour unassigned);
  real-valued Normal data.
Both forms (BNMF_SUB_FORM) and batches of 1 and 3 samples (BNMF_SUB_BATCH) must give the same bits.

The rings cannot be written from outside, so a zero-total tumour in one sample only cannot be planted on the device: that convention is
pinned on the restatement (tests/test_subtypes_host.py) and held on the device where a chain produces it (the rank-learning chain's
sample without any factor)."""
import ctypes as C

import numpy as np
import pytest

import subtypes_ref as R

pytestmark = pytest.mark.gpu

W, T_END, N_RANGE = 16, 40, 12
USED = np.array([1, 1, 0, 1, 1, 1, 0, 0, 1, 1, 1, 1], dtype=np.int32)
ARRAYS = ("membership", "label", "tumour", "centre", "size", "together", "labels", "series")
INFO = ("n_used", "n_matched", "n_unmatched", "n_included", "n_left_out", "C", "n_steps", "n_query", "n_not_converged", "n_certain", "n_never_assigned",
        "smallest_subtype_at", "least_certain_at", "mean_certainty", "least_certain", "smallest_subtype", "min_certainty")

# name: K, G, N, likelihood, prior, learning_rank, seed
CASES = {
    "g200": (8, 200, 5, "poisson", "gamma", False, 4),
    "g1100": (6, 1100, 3, "poisson", "gamma", False, 4),                   # two blocks of member positions, the last ragged
    "g8300": (6, 8300, 3, "poisson", "gamma", False, 4),                   # 9 blocks: a second round of blocks for the 8 waves
    "n128": (8, 40, 128, "poisson", "gamma", False, 4),                    # the largest N; with C = 32 the largest N C
    "sbfi": (96, 8, 20, "poisson", "gamma", True, 14),                     # samples with A[n] = 0, one with A = 0; N > 8: the tiled form
    "normal": (12, 10, 3, "normal", "exponential", False, 4),              # real-valued data
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
    """the chain at iteration 40 and the used samples of the range: once per case"""
    if case in _RUNS:
        return _RUNS[case]
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import apply_hyperprior_params
    K, G, N, lk, prior, lr, seed = CASES[case]
    M = _data(case)
    e = Engine(M, N, likelihood=lk, prior=prior, learning_rank=lr, seed=seed, window=W, temperature=_temps() if lr else None)
    apply_hyperprior_params(e, prior, M, N)
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


def _centres(r, Cn):
    """a start: the share profiles of Cn tumours spread over the cohort in one used sample"""
    x = R.loads(*r["samples"])
    for s in range(len(x) - 1, -1, -1):                                                                        # the newest used sample with enough assigned tumours
        q, ok = R.profiles(x[s])
        if ok.sum() >= Cn:
            break
    seeds = [int(g) for g in np.where(ok)[0][np.linspace(0, int(ok.sum()) - 1, Cn).astype(int)]]
    return np.asfortranarray(q[:, seeds])


def _differences(tag, a, b, arrays=ARRAYS, info=INFO):
    """the names of the outputs of a that are not b's, bit for bit with NaN equal to NaN (printed with the first place they differ)"""
    bad = []
    for k in arrays:
        if k not in a and k not in b:
            continue
        if (k in a) != (k in b):
            if np.asarray(a[k] if k in a else b[k]).size == 0:                                                # (no query: the binding leaves it out)
                continue
            print(f"subtypes[{tag}] {k}: only one side has it")
            bad.append(k)
            continue
        x, y = np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)
        if x.shape != y.shape:
            print(f"subtypes[{tag}] {k}: shapes {x.shape} and {y.shape}")
            bad.append(k)
            continue
        nx, ny = np.isnan(x), np.isnan(y)
        ne = (nx != ny) | (~nx & ~ny & (_bits(x).reshape(x.shape) != _bits(y).reshape(y.shape)))
        if ne.any():
            i = tuple(np.argwhere(ne)[0])
            print(f"subtypes[{tag}] {k}: {int(ne.sum())} of {ne.size} differ, first at {i}: {x[i]!r} against {y[i]!r}")
            bad.append(k)
    for k in info:
        fa, fb = float(a[k]), float(b[k])
        if not ((np.isnan(fa) and np.isnan(fb)) or _bits(fa) == _bits(fb)):
            print(f"subtypes[{tag}] {k}: {a[k]!r} against {b[k]!r}")
            bad.append(k)
    return bad


def _queries(G):
    return np.array(sorted({0, G - 1, G // 2}) + [0], dtype=np.int32)                                          # the ends, the middle, one named twice


@pytest.mark.parametrize("case,Cn,steps", [("g200", 2, 50), ("g200", 3, 50), ("g200", 5, 50), ("g200", 9, 50), ("g1100", 3, 50), ("g8300", 3, 50),
                                           ("n128", 32, 10), ("sbfi", 3, 50), ("normal", 5, 50)])
def test_every_output_is_the_restatement_bit_for_bit(case, Cn, steps, monkeypatch):
    r = _run(case)
    e, G, N = r["e"], r["G"], r["N"]
    q, c0 = _queries(G), _centres(r, Cn)
    kw = dict(used=USED, end_iter=r["end"], query=q, n_steps=steps, min_certainty=0.9, labels=True)
    ref = R.subtypes_reference(*r["samples"], c0, query=q, n_steps=steps, min_certainty=0.9)
    dev = e.subtypes(N_RANGE, c0, **kw)
    A = r["samples"][2]
    print(f"subtypes[{case}, C {Cn}] S {dev['n_used']} m {dev['n_included']} steps {dev['series'][1]} not converged {dev['n_not_converged']} certain "
          f"{dev['n_certain']} mean certainty {dev['mean_certainty']!r} sizes {dev['size'][0]}; samples that exclude a factor {int((A == 0).any(axis=1).sum())}")
    assert dev["membership"].shape == (Cn, G) and dev["centre"].shape == (4, N, Cn) and dev["size"].shape == (4, Cn) and dev["labels"].shape == (9, G)
    assert dev["together"].shape == (len(q), G) and dev["series"].shape == (3, 9) and dev["tumour"].shape == (3, G)
    bad = _differences(f"{case} C {Cn}", dev, ref)
    if case == "sbfi":
        assert (A == 0).any() and (A == 0).all(axis=1).any(), "no used sample without a factor"
        s0 = int(np.where((A == 0).all(axis=1))[0][0])
        assert (dev["labels"][s0] == -1).all() and dev["series"][1, s0] == 1 and dev["series"][2, s0] == 0   # every tumour unassigned: one step, no change
        assert (dev["tumour"][1] < 1.0).all()
    # the other form and small batches of samples through the scratch: the same bits
    for form, batch in (("1", None), (None, "1"), ("1", "3")):
        if form:
            monkeypatch.setenv("BNMF_SUB_FORM", form)
        if batch:
            monkeypatch.setenv("BNMF_SUB_BATCH", batch)
        bad += _differences(f"{case} C {Cn}, form {form}, batch {batch}", e.subtypes(N_RANGE, c0, **kw), ref)
        monkeypatch.delenv("BNMF_SUB_FORM", raising=False)
        monkeypatch.delenv("BNMF_SUB_BATCH", raising=False)
    assert not bad, bad


def test_include_drops_tumours_on_both_sides_of_a_block_boundary():
    r = _run("g1100")
    e, G = r["e"], r["G"]
    inc = np.ones(G, dtype=np.int32)
    inc[[0, 500, 1020, 1023, 1024, 1030, G - 1]] = 0                                                           # the boundary of the positions moves to tumour 1,028
    q = np.array([1, 1023 + 5, G - 2], dtype=np.int32)
    c0 = _centres(r, 4)
    dev = e.subtypes(N_RANGE, c0, include=inc, query=q, used=USED, end_iter=r["end"], labels=True)
    ref = R.subtypes_reference(*r["samples"], c0, include=inc, query=q)
    assert dev["n_left_out"] == 7 and np.isnan(dev["tumour"][:, inc == 0]).all() and (dev["label"][inc == 0] == -1).all()
    assert (dev["labels"][:, inc == 0] == -2).all() and np.isnan(dev["together"][:, inc == 0]).all() and np.isnan(dev["membership"][:, inc == 0]).all()
    assert not _differences("include", dev, ref)


@pytest.mark.parametrize("case", ["g200", "normal"])
def test_equivalent_calls_give_the_same_bits(case):
    r = _run(case)
    e, end, G, N = r["e"], r["end"], r["G"], r["N"]
    q, c0 = _queries(G), _centres(r, 3)
    kw = dict(query=q, n_steps=20, labels=True)
    first = e.subtypes(N_RANGE, c0, used=USED, end_iter=end, **kw)
    assert not _differences("again", first, e.subtypes(N_RANGE, c0, used=USED, end_iter=end, **kw))
    assert not _differences("at", e.subtypes(10, c0, **kw), e.subtypes(10, c0, end_iter=e.iter, **kw))        # bnmf_subtypes is bnmf_subtypes_at(iter)
    ident = np.tile(np.arange(N, dtype=np.int32), (10, 1))
    assert not _differences("ones", e.subtypes(10, c0, **kw), e.subtypes_at(e.iter, 10, c0, used=np.ones(10, dtype=np.int32), include=np.ones(G, dtype=np.int32),
                                                                            perm=ident, **kw))
    s2 = np.zeros(N_RANGE, dtype=np.int32)
    s2[[2, 9]] = 1                                                                                             # S = 2
    two = e.subtypes(N_RANGE, c0, used=s2, end_iter=end, **kw)
    assert two["n_used"] == 2
    back = e.iter - (end - N_RANGE + 1) + 1
    win = {nm: np.stack([e.window(nm, back)[i] for i in (2, 9)]) for nm in ("P", "E", "A")}
    assert not _differences("S = 2", two, R.subtypes_reference(win["P"], win["E"], win["A"].reshape(2, -1), c0, query=q, n_steps=20))
    # every output NULL: the info fields are the same
    from bayesnmf_amd.engine import lib, BnmfSubtypesInfo
    L, dp, ip = lib(), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    info = BnmfSubtypesInfo()
    assert L.bnmf_subtypes_at(e._h, end, N_RANGE, USED.ctypes.data_as(ip), None, None, c0.ctypes.data_as(dp), 3, 20, q.ctypes.data_as(ip), len(q), 0.9, None, None,
                              None, None, None, None, None, None, C.byref(info)) == 0
    assert not _differences("all NULL", {k: getattr(info, k) for k in INFO}, first, arrays=())


def test_perm_from_relabel_by_hand_and_an_unmatched_sample():
    r = _run("g200")
    e, end, G, N = r["e"], r["end"], r["G"], r["N"]
    c0 = _centres(r, 3)
    sel = np.where(USED == 1)[0]
    rel = np.asarray(e.relabel(N_RANGE, used=USED, end_iter=end)["perm"], dtype=np.int32)                     # a row per used sample
    assert rel.shape == (len(sel), N)
    rng = np.random.default_rng(2)
    hand = np.stack([rng.permutation(N) for _ in sel]).astype(np.int32)
    hand[4] = -1                                                                                               # an unmatched sample
    hand[0] = np.arange(N)[::-1]
    for tag, rows in (("relabel", rel), ("by hand", hand)):
        perm = np.full((N_RANGE, N), -1, dtype=np.int32)                                                       # scattered into the range's rows
        perm[sel] = rows
        perm[2] = 7                                                                                            # (a row of an unused sample is not read)
        dev = e.subtypes(N_RANGE, c0, perm=perm, used=USED, end_iter=end, query=[3], labels=True)
        ref = R.subtypes_reference(*r["samples"], c0, perm=rows, query=[3])
        assert not _differences(tag, dev, ref)
    assert dev["n_unmatched"] == 1 and dev["n_matched"] == len(sel) - 1 and (dev["labels"][4] == -2).all() and np.isnan(dev["series"][:, 4]).all()
    # permuting the factors of every sample and of the start alike changes the order of the sums over j only: the labels agree where no
    # distance is within rounding of another; the identity perm is no perm, bit for bit
    ident = np.tile(np.arange(N, dtype=np.int32), (N_RANGE, 1))
    assert not _differences("identity", e.subtypes(N_RANGE, c0, perm=ident, used=USED, end_iter=end), e.subtypes(N_RANGE, c0, used=USED, end_iter=end))


def test_equal_columns_one_step_restart_and_renumbering():
    r = _run("g200")
    e, end, G, N = r["e"], r["end"], r["G"], r["N"]
    kw = dict(used=USED, end_iter=end, labels=True)
    c0 = _centres(r, 3)
    # two equal columns: in the step that meets them the lower label takes all and the empty cluster keeps its centre in every sample
    # (in a later step the kept centre may win tumours back from the one that moved: the whole run is held to the restatement only)
    dup = np.asfortranarray(c0[:, [0, 1, 1]])
    assert not _differences("equal columns, the whole run", e.subtypes(N_RANGE, dup, **kw), R.subtypes_reference(*r["samples"], dup))
    dev = e.subtypes(N_RANGE, dup, n_steps=1, **kw)
    ref = R.subtypes_reference(*r["samples"], dup, n_steps=1)
    assert not _differences("equal columns", dev, ref)
    assert (dev["labels"] != 2).all() and (dev["size"][0, 2] == 0.0) and (dev["size"][1, 2] == 0.0)
    assert (ref["sample_centres"][:, :, 2] == dup[:, 2]).all() and (dev["centre"][2:, :, 2] == dup[:, 2]).all()   # (the quantiles of a constant are the constant)
    assert (dev["membership"][2][~np.isnan(dev["membership"][2])] == 0.0).all() and dev["smallest_subtype_at"] == 2
    # n_steps = 1 is the nearest-centre assignment
    one = e.subtypes(N_RANGE, c0, n_steps=1, **kw)
    assert not _differences("one step", one, R.subtypes_reference(*r["samples"], c0, n_steps=1))
    x = R.loads(*r["samples"])
    for s in (0, 5):
        q, ok = R.profiles(x[s])
        d = ((q[:, :, None] - c0[:, None, :]) ** 2).sum(axis=0)                                                # a plain nearest centre
        clear = np.sort(d, axis=1)[:, 1] - np.sort(d, axis=1)[:, 0] > 1e-9
        assert np.array_equal(one["labels"][s][ok & clear], d.argmin(axis=1)[ok & clear]) and (one["series"][1] == 1).all()
    # a second call started from the first call's mean centres runs, and its restatement holds
    full = e.subtypes(N_RANGE, c0, **kw)
    again = e.subtypes(N_RANGE, np.asfortranarray(full["centre"][0]), **kw)
    assert not _differences("restart", again, R.subtypes_reference(*r["samples"], np.asfortranarray(full["centre"][0])))
    # renumbering the columns of a start without ties renumbers the outputs
    order = np.array([2, 0, 1])
    ren = e.subtypes(N_RANGE, np.asfortranarray(c0[:, order]), query=[5], **kw)
    base = e.subtypes(N_RANGE, c0, query=[5], **kw)
    assert np.array_equal(np.where(ren["labels"] >= 0, order[np.maximum(ren["labels"], 0)], ren["labels"]), base["labels"])
    assert not _differences("renumbered", dict(membership=ren["membership"][np.argsort(order)], centre=ren["centre"][:, :, np.argsort(order)],
                                               size=ren["size"][:, np.argsort(order)], together=ren["together"], series=ren["series"]),
                            dict(membership=base["membership"], centre=base["centre"], size=base["size"], together=base["together"], series=base["series"]),
                            info=())


def test_refusals():
    from bayesnmf_amd import Engine
    from bayesnmf_amd.engine import lib, BnmfSubtypesInfo, BnmfError
    from bayesnmf_amd.setup import apply_hyperprior_params, synth_counts
    r = _run("g200")
    e, G, N, L = r["e"], r["G"], r["N"], lib()
    info = BnmfSubtypesInfo()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    c0 = _centres(r, 3)
    before = e.subtypes(N_RANGE, c0, used=USED, end_iter=r["end"], query=[3])

    def err():
        msg = L.bnmf_last_error().decode()
        assert msg
        return msg

    def call(n=10, used=None, include=None, perm=None, cen=c0, Cn=3, steps=5, query=None, Q=None, mc=0.9, inf=info, at=None, h=None):
        pt = lambda v: None if v is None else v.ctypes.data_as(ip)  # noqa: E731
        Q = (0 if query is None else len(query)) if Q is None else Q
        f = None if inf is None else C.byref(inf)
        cp = None if cen is None else cen.ctypes.data_as(dp)
        h = e._h if h is None else h
        rest = (pt(used), pt(include), pt(perm), cp, Cn, steps, pt(query), Q, mc, None, None, None, None, None, None, None, None, f)
        return L.bnmf_subtypes(h, n, *rest) if at is None else L.bnmf_subtypes_at(h, at, n, *rest)

    for at in (None, e.iter):
        assert call(inf=None, at=at) == -1 and "null" in err()                                       # BNMF_EINVAL
        assert call(cen=None, at=at) == -1 and "null" in err()
        u = np.ones(10, dtype=np.int32); u[6] = 2
        assert call(used=u, at=at) == -1 and "used[6] = 2" in err()
        inc = np.ones(G, dtype=np.int32); inc[64] = -1
        assert call(include=inc, at=at) == -1 and "include[64] = -1" in err()
        for bad in (1, 33):
            assert call(Cn=bad, cen=np.zeros((N, 33), order="F"), at=at) == -1 and f"C = {bad}" in err()
        for bad in (0, 1001):
            assert call(steps=bad, at=at) == -1 and f"n_steps = {bad}" in err()
        assert call(Q=-1, at=at) == -1 and "Q = -1" in err()
        assert call(Q=2, at=at) == -1 and "query is null" in err()
        assert call(query=np.array([1, G], dtype=np.int32), at=at) == -1 and f"query[1] = {G}" in err()
        inc = np.ones(G, dtype=np.int32); inc[7] = 0
        assert call(include=inc, query=np.array([3, 7], dtype=np.int32), at=at) == -1 and "query[1] = 7" in err() and "leaves out" in err()
        for bad in (float("nan"), float("inf"), -1.0):
            cb = c0.copy(order="F"); cb[2, 1] = bad
            assert call(cen=cb, at=at) == -1 and "centres0[2, 1]" in err()
        for bad in (float("nan"), -0.1, 1.5):
            assert call(mc=bad, at=at) == -1 and "min_certainty" in err()
        pm = np.tile(np.arange(N, dtype=np.int32), (10, 1)); pm[3, 1] = 0                             # a factor named twice
        assert call(perm=pm, at=at) == -1 and "perm[3]" in err() and "sample 3" in err()
        pm[3] = -1; pm[3, 0] = 2                                                                      # -1 in part
        assert call(perm=pm, at=at) == -1 and "perm[3]" in err()
        u = np.zeros(10, dtype=np.int32); u[3] = 1
        assert call(used=u, at=at) == -2 and "1 used sample" in err()                                # BNMF_ESIZE
        pm = np.full((10, N), -1, dtype=np.int32); pm[5] = np.arange(N)
        assert call(perm=pm, at=at) == -2 and "1 matched sample" in err()
        inc = np.zeros(G, dtype=np.int32); inc[[5, 9]] = 1
        assert call(include=inc, at=at) == -2 and "2 included tumours for C = 3" in err()
    assert call(n=W + 1) == -2 and err()
    assert call(n=5, at=e.iter + 1) == -2 and "are kept" in err()
    assert call(n=3, at=e.iter - W + 1) == -2 and "are kept" in err()
    with pytest.raises(BnmfError, match="used has 3 entries"):
        e.subtypes(10, c0, used=[1, 1, 1])
    with pytest.raises(BnmfError, match="include has shape"):
        e.subtypes(10, c0, include=[1, 1, 1])
    with pytest.raises(BnmfError, match="centres0 has shape"):
        e.subtypes(10, c0[:2])
    with pytest.raises(BnmfError, match="perm is"):
        e.subtypes(10, c0, perm=np.zeros((3, N), dtype=np.int32))
    # window = 0: BNMF_ESTATE
    M, _, _ = synth_counts(8, 6, N, 21, mean_total=1500)
    z = Engine(M, N, prior="gamma", seed=4, window=0)
    apply_hyperprior_params(z, "gamma", M, N)
    z.init(); z.run(5)
    assert call(n=3, h=z._h) == -7 and "window = 0" in err()
    assert call(n=3, at=z.iter, h=z._h) == -7 and "window = 0" in err()
    z.close()
    # more factors than BNMF_SUB_MAX_N: BNMF_ESIZE, the limit named (the kernel's LDS arrays are sized by it)
    big = Engine(M, 129, prior="gamma", seed=4, window=4)
    apply_hyperprior_params(big, "gamma", M, 129)
    big.init(); big.run(3)
    cbig = np.asfortranarray(np.full((129, 3), 1.0 / 129))
    assert call(n=3, cen=cbig, h=big._h) == -2 and "N = 129 factors, at most 128" in err()
    assert call(n=3, cen=cbig, at=big.iter, h=big._h) == -2 and "N = 129 factors, at most 128" in err()
    big.close()
    assert L.bnmf_version() == 100
    # the handle is usable afterwards: the same bits as before the refusals
    assert not _differences("afterwards", before, e.subtypes(N_RANGE, c0, used=USED, end_iter=r["end"], query=[3]))


def test_more_queries_than_one_launch_of_the_counting_kernel_takes():
    """Q has no upper bound: the queries pass through k_sub_count in slices of 65,534 (the grid's y is 16 bits wide).  70,000 queries
    that repeat 4 tumours: every row is the row of its tumour in a call with those 4 alone, and everything else is the same"""
    r = _run("g200")
    e, G = r["e"], r["G"]
    c0 = _centres(r, 3)
    four = np.array([0, 7, 101, G - 1], dtype=np.int32)
    few = e.subtypes(N_RANGE, c0, query=four, used=USED, end_iter=r["end"])
    many = e.subtypes(N_RANGE, c0, query=np.tile(four, 17500), used=USED, end_iter=r["end"])
    assert many["n_query"] == 70000 and many["together"].shape == (70000, G)
    t = many["together"].reshape(17500, 4, G)
    assert not np.isnan(few["together"]).all()
    assert np.array_equal(np.isnan(t), np.broadcast_to(np.isnan(few["together"]), t.shape))
    assert np.array_equal(np.nan_to_num(t, nan=-1.0), np.broadcast_to(np.nan_to_num(few["together"], nan=-1.0), t.shape))
    assert not _differences("many queries", many, few, arrays=tuple(k for k in ARRAYS if k != "together"), info=tuple(k for k in INFO if k != "n_query"))


def test_the_call_is_read_only_for_the_chain():
    """a chain that calls subtypes mid-run continues with the bits of a twin that never did"""
    from bayesnmf_amd import Engine
    from bayesnmf_amd.setup import apply_hyperprior_params
    K, G, N, lk, prior, lr, seed = CASES["g200"]
    M = _data("g200")
    a, b = (Engine(M, N, likelihood=lk, prior=prior, seed=seed, window=W) for _ in range(2))
    for c in (a, b):
        apply_hyperprior_params(c, prior, M, N)
        c.init(); c.run(20)
    a.subtypes(12, _centres(_run("g200"), 3), query=[0, 64], labels=True)
    ra, rb = a.run(10), b.run(10)
    assert np.array_equal(_bits(ra), _bits(rb))
    for nm in ("P", "E", "A"):
        assert np.array_equal(_bits(a.get(nm)), _bits(b.get(nm))), nm
    a.close(); b.close()
