"""CPU tests of the two static allocation schedules (csrc/zplan.h plan_zsort / plan_zstep, through bnmf_test_zsort_plan /
bnmf_test_zstep_plan): the plan the host would upload is decoded with plain numpy and checked against the contract the kernels
rely on ("Contract of the sorted schedule"), for several CU counts and for the data no chain-level test feeds them:
all-zero columns, G between one and two times the CU count, blocks without a column, large cells exported into such blocks,
and the boundaries of every size rule.  No GPU is involved: a plan that breaks the contract is a wild load on a device."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CUS = (4, 104, 256, 304)
SWITCHES = ("BNMF_ZSORT", "BNMF_ZSSPREAD", "BNMF_ZSLDS", "BNMF_ZSW", "BNMF_ZSQMAX", "BNMF_ZSIT16", "BNMF_ZSPK", "BNMF_ZSTEP", "BNMF_ZPGB", "BNMF_ZPIT16")
ZP_KC, ZP_QMAX = 32, 60                         # zalloc_step.h: rows per chunk, quads per item
ZS_BIG, ZS_HOME = 8192, 16                      # plan_zsort: a cell above ZS_BIG counts keeps ZS_HOME fragments at home


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)


def _lib():
    from bayesnmf_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = engine.lib()
    vp, ll = C.c_void_p, C.POINTER(C.c_longlong)
    L.bnmf_test_zsort_plan.argtypes = [C.c_int] * 5 + [vp, ll] + [vp] * 5
    L.bnmf_test_zstep_plan.argtypes = [C.c_int] * 5 + [vp, ll] + [vp] * 6
    return L


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Plan:
    pass


def zsort_plan(M, N, save_Z, n_cu):
    L = _lib()
    M = np.asfortranarray(M, dtype=np.int32)
    K, G = M.shape
    d = (C.c_longlong * 14)()
    assert L.bnmf_test_zsort_plan(K, G, N, int(save_Z), n_cu, _ptr(M), d, None, None, None, None, None) == 0, L.bnmf_last_error()
    p = Plan()
    (p.ok, p.KP, p.GBc, p.nb, p.W, p.qmax, p.it16, p.pk, p.shared, p.nempty, ncols, nitems, nmblk, p.nblk) = [int(x) for x in d]
    if not p.ok:
        return p
    p.blocks = np.zeros((p.nb, 4), np.int32)
    p.cols = np.full(ncols, -12345, np.int32)
    p.items = np.zeros(nitems, np.uint32)
    p.items16 = np.zeros(nitems if p.it16 else 0, np.uint16)
    p.Mblk = np.zeros(nmblk, np.int32)
    d2 = (C.c_longlong * 14)()
    assert L.bnmf_test_zsort_plan(K, G, N, int(save_Z), n_cu, _ptr(M), d2, _ptr(p.blocks), _ptr(p.cols), _ptr(p.items),
                                  _ptr(p.items16) if p.it16 else None, _ptr(p.Mblk)) == 0
    assert list(d) == list(d2)                                                    # the planner is deterministic (the fill plans again)
    return p


def zstep_plan(M, N, save_Z, n_cu):
    L = _lib()
    M = np.asfortranarray(M, dtype=np.int32)
    K, G = M.shape
    d = (C.c_longlong * 11)()
    rc = L.bnmf_test_zstep_plan(K, G, N, int(save_Z), n_cu, _ptr(M), d, None, None, None, None, None, None)
    p = Plan()
    p.rc = rc
    if rc:
        return p
    (p.ok, p.nch, p.nwg, p.W, p.GBP, p.it16, p.maxfrag, nbat, nsteps, ncols, nitems) = [int(x) for x in d]
    if not p.ok:
        return p
    p.wgs = np.zeros((p.nwg, 2), np.int32)
    p.batches = np.zeros((nbat, 2), np.int32)
    p.steps = np.zeros(nsteps, np.dtype([("item0", "<i8"), ("ntw", "<i4"), ("pad", "<i4")]))
    p.cols = np.full(ncols, -12345, np.int32)
    p.items = np.zeros(nitems, np.uint32)
    p.items16 = np.zeros(nitems if p.it16 else 0, np.uint16)
    assert L.bnmf_test_zstep_plan(K, G, N, int(save_Z), n_cu, _ptr(M), d, _ptr(p.wgs), _ptr(p.batches), _ptr(p.steps), _ptr(p.cols), _ptr(p.items),
                                  _ptr(p.items16) if p.it16 else None) == 0
    return p


def _fragments_exact(cell, f, nfrag_of_cell, what):
    """every (cell, fragment) pair of the plan occurs once, and they are exactly fragment 0 .. F - 1 of every cell (F = 1 for a cell without counts)"""
    ncell = nfrag_of_cell.size
    fmax = int(nfrag_of_cell.max())
    assert (f < nfrag_of_cell[cell]).all(), f"{what}: a fragment index beyond its cell's last fragment"
    key = cell.astype(np.int64) * fmax + f
    want = np.repeat(np.arange(ncell, dtype=np.int64) * fmax, nfrag_of_cell) + \
        (np.arange(int(nfrag_of_cell.sum()), dtype=np.int64) - np.repeat(np.cumsum(nfrag_of_cell) - nfrag_of_cell, nfrag_of_cell))
    key = np.sort(key)
    assert key.size == want.size and np.array_equal(key, want), f"{what}: a fragment is missing or occurs twice ({key.size} items for {want.size} fragments)"


def check_zsort(M, N, save_Z, n_cu, p):
    """The contract of the sorted schedule, as k_zalloc_sort, k_zexpand and colterms read it."""
    M = np.asarray(M)
    K, G = M.shape
    nb, GBc, qmax = p.nb, p.GBc, p.qmax
    item0, ntask, col0, ncols = (p.blocks[:, i].astype(np.int64) for i in range(4))
    # ---- the tables: contiguous ranges inside the lists
    assert nb >= 1 and 1 <= GBc <= 64 and p.W in (4, 6, 8, 12, 14, 16) and p.nblk == (N + 4) // 5
    assert (ncols >= 0).all() and (ncols <= GBc).all() and (ntask >= 0).all()
    assert col0[0] == 0 and np.array_equal(col0[1:], (col0 + ncols)[:-1]), "column ranges are not contiguous"
    assert item0[0] == 0 and np.array_equal(item0[1:], (item0 + 64 * ntask)[:-1]), "item ranges are not contiguous (or not whole tasks of 64)"
    nlisted = int(ncols.sum())
    assert nlisted <= p.cols.size, "a block's column range ends beyond the column list"
    assert p.items.size == max(1, int(64 * ntask.sum()))
    assert ((p.cols >= 0) & (p.cols < G)).all(), "the uploaded column list holds something that is no column"
    # ---- what the kernel's set-up reads is inside what is allocated: cols[col0 + 0] whatever ncols is (zalloc_sort.h, block set-up)
    over = np.nonzero(col0 + np.maximum(ncols, 1) > p.cols.size)[0]
    assert over.size == 0, (f"set-up read beyond the column list: blocks {over.min()}..{over.max()} ({over.size} of {nb}) have no column and col0 = "
                            f"{int(col0[over[0]])} = the {p.cols.size} ints uploaded")
    # ---- items
    blk = np.repeat(np.arange(nb), 64 * ntask)
    it = p.items[:blk.size]
    valid = it != 0xFFFFFFFF
    if blk.size == 0:
        assert p.items.size == 1 and p.items[0] == 0xFFFFFFFF
    itv, bv = it[valid], blk[valid]
    k, gl, f = (itv & 1023).astype(np.int64), ((itv >> 10) & 63).astype(np.int64), (itv >> 16).astype(np.int64)
    assert (k < K).all() and (gl < ncols[bv]).all() and (f <= 65534).all()          # (f = 65535 with k = 1023, gl = 63 is the 4-byte sentinel)
    assert (ncols[ntask > 0] > 0).all()                                            # an empty lane reads row 0 of the block's first column
    g = p.cols[col0[bv] + gl].astype(np.int64)
    if p.it16:
        assert K <= 127 and (f < 8).all() and (k < 128).all()
        enc = (k | (gl << 7) | (f << 13)).astype(np.uint16)
        assert (enc != 0xFFFF).all(), "a real 2-byte item equals the empty-lane sentinel"
        want16 = np.full(it.size, 0xFFFF, np.uint16)
        want16[valid] = enc
        assert np.array_equal(p.items16[:blk.size], want16), "the 2-byte items do not decode to the 4-byte items"
        r = p.items16[:blk.size][valid].astype(np.int64)
        assert np.array_equal(r & 127, k) and np.array_equal((r >> 7) & 63, gl) and np.array_equal(r >> 13, f)   # (the kernel's decode)
    # ---- fragments: every cell's 0 .. F - 1 once over the whole grid; their quads add up to ceil(m / 4)
    m = M.reshape(-1, order="F").astype(np.int64)                                  # cell = k + K g
    qt = (m + 3) >> 2
    F = np.maximum(1, (qt + qmax - 1) // qmax)
    cell = k + K * g
    _fragments_exact(cell, f, F, "zsort")
    quads = np.where(qt[cell] > 0, np.minimum(qmax, qt[cell] - f * qmax), 0)       # (what the lane runs: zalloc_sort.h nq)
    assert (quads[qt[cell] > 0] >= 1).all()
    assert np.array_equal(np.bincount(cell, weights=quads, minlength=K * G).astype(np.int64), qt)
    # ---- owners: fragment 0 of every cell of a column (the lane that leaves Mhat) is in ONE block, which lists the column once
    f0 = f == 0
    owner = np.full(K * G, -1, np.int64)
    owner[cell[f0]] = bv[f0]
    owner = owner.reshape(G, K)
    assert (owner == owner[:, :1]).all(), "the first fragments of a column's cells are in different blocks"
    owner = owner[:, 0]
    lb = np.repeat(np.arange(nb), ncols)                                           # block of every listed column slot
    lg = p.cols[:nlisted].astype(np.int64)
    pair = lb * G + lg
    assert np.unique(pair).size == pair.size, "a block lists a column twice"
    own = owner[lg] == lb
    assert np.array_equal(np.sort(lg[own]), np.arange(G)), "a column is not an own column of exactly one block"
    nown = np.bincount(lb[own], minlength=nb)
    slot = np.arange(nlisted) - col0[lb]
    assert (slot[own] < nown[lb[own]]).all(), "a guest column in front of an own column"
    used = np.unique(bv * G + g)
    assert np.isin(pair[~own], used).all(), "a guest column no item of its block refers to"
    if not p.shared:
        assert own.all()
    assert int((nown == 0).sum()) == p.nempty
    # large cells: fragments beyond the first ZS_HOME may be anywhere, the others are at home
    home = owner[g] == bv
    assert home[f < ZS_HOME].all() and (home | (m[cell] > ZS_BIG)).all()
    if save_Z:
        assert not p.shared and int(M.max()) <= 65535
    # ---- two factors per word only if no half can overflow
    if p.pk:
        assert int(M.sum(0).max()) < 65536
        rows = np.zeros((nb, K), np.int64)
        np.add.at(rows, lb, M[:, lg].T.astype(np.int64))
        assert int(rows.max()) < 65536, "pk with a block row total (guests included) of 65,536 or more"
    # ---- Mblk: M's columns in column-list order
    assert p.Mblk.size >= K * nlisted
    assert np.array_equal(p.Mblk[:K * nlisted].reshape(nlisted, K), M[:, lg].T), "Mblk is not M in column-list order"
    return dict(nown=nown, ncols=ncols, guests=ncols - nown, units_at_home=int((home & (f >= ZS_HOME)).sum()), units_away=int((~home).sum()))


def check_zstep(M, N, n_cu, p):
    M = np.asarray(M)
    K, G = M.shape
    W, GBP, nch = p.W, p.GBP, p.nch
    assert p.nwg == min(G, n_cu) and nch == (K + ZP_KC - 1) // ZP_KC and GBP in (32, 40) and W == 8
    batch0, nbatch = p.wgs[:, 0].astype(np.int64), p.wgs[:, 1].astype(np.int64)
    # G >= workgroups always (nwg = min(G, n_cu)), and a column costs its counts + 64 K > 0: no workgroup is left without one
    assert (nbatch >= 1).all(), "a workgroup without a column"
    assert batch0[0] == 0 and np.array_equal(batch0[1:], (batch0 + nbatch)[:-1]) and int(nbatch.sum()) == p.batches.shape[0]
    bcol0, bn = p.batches[:, 0].astype(np.int64), p.batches[:, 1].astype(np.int64)
    assert (bn >= 1).all() and (bn <= GBP).all()
    assert bcol0[0] == 0 and np.array_equal(bcol0[1:], (bcol0 + bn)[:-1]) and int(bn.sum()) == p.cols.size == G
    assert np.array_equal(np.sort(p.cols), np.arange(G)), "a column is not in exactly one workgroup"
    nsteps = p.batches.shape[0] * nch
    assert p.steps.size == nsteps
    s_item0, ntw = p.steps["item0"], p.steps["ntw"].astype(np.int64)
    assert s_item0[0] == 0 and np.array_equal(s_item0[1:], (s_item0 + W * ntw * 64)[:-1]), "a wave's list is not padded to ntw * 64"
    assert p.items.size == max(1, int((W * ntw * 64).sum()))
    st = np.repeat(np.arange(nsteps), W * ntw * 64)
    it = p.items[:st.size]
    valid = it != 0xFFFFFFFF
    # no task that is empty in every wave: ntw is what the longest wave list needs
    pos = np.arange(st.size) - s_item0[st]
    wave = pos // (ntw[st] * 64)
    cnt = np.zeros((nsteps, W), np.int64)
    np.add.at(cnt, (st[valid], wave[valid]), 1)
    assert np.array_equal((cnt.max(1) + 63) // 64, ntw)
    assert (cnt.max(1) - cnt.min(1) <= 1).all()                                     # snake order: the waves' counts differ by one at most
    # the empty lanes are the tail of a wave's list: the kernel leaves the list at the first task without an item
    inwave = pos - wave * ntw[st] * 64
    assert (inwave[valid] < cnt[st[valid], wave[valid]]).all(), "an empty lane in front of an item of its wave's list"
    itv, sv = it[valid], st[valid]
    kl, gl, f = (itv & 31).astype(np.int64), ((itv >> 5) & 63).astype(np.int64), (itv >> 11).astype(np.int64)
    bi, ch = sv // nch, sv % nch
    k = ch * ZP_KC + kl
    assert (k < K).all() and (gl < bn[bi]).all() and (gl != 63).all() and (f < (1 << 21)).all()
    g = p.cols[bcol0[bi] + gl].astype(np.int64)
    m = M.reshape(-1, order="F").astype(np.int64)
    qt = (m + 3) >> 2
    F = np.maximum(1, (qt + ZP_QMAX - 1) // ZP_QMAX)
    _fragments_exact(k + K * g, f, F, "zstep")
    assert p.maxfrag == int(f.max())
    if p.it16:
        assert p.maxfrag <= 30
        want16 = np.full(it.size, 0xFFFF, np.uint16)
        want16[valid] = itv.astype(np.uint16)
        assert (itv < 0xFFFF).all() and np.array_equal(p.items16[:st.size], want16)
    else:
        assert p.maxfrag > 30 or os.environ.get("BNMF_ZPIT16") == "0"


# ------------------------------------------------------------------ data
def dense(K, G, seed=3):
    from bayesnmf_amd.setup import synth_counts
    return synth_counts(K, G, 4, seed)[0]


def sparse(K, G, nonempty, seed=5):
    """G columns of which `nonempty` hold counts (scattered over the column range), the others none"""
    rng = np.random.default_rng(seed)
    M = np.zeros((K, G), np.int32, order="F")
    idx = rng.choice(G, size=nonempty, replace=False) if nonempty else np.zeros(0, np.int64)
    M[:, idx] = rng.poisson(rng.gamma(0.7, 30.0, size=(K, idx.size)))
    M[0, idx] += 1                                                                  # really non-empty
    return M


def _g_sparse(n_cu):
    return n_cu + max(1, (44 * n_cu) // 256)                                        # in (n_cu, 2 n_cu]: 300 on 256 CUs


def _expect_empty(M, p):
    """Zero columns add no load: they fill the lightest block to its capacity before the next block gets one.  So blocks stay without a
    column — the last one among them — iff non-empty columns + ceil(empty columns / capacity) < blocks (plan_zsort, the dealing loop)."""
    nz = int((M.sum(0) > 0).sum())
    cap = p.GBc if not p.shared else max(1, -(-M.shape[1] // p.nb))
    return nz + -(-(M.shape[1] - nz) // cap) < p.nb


# ------------------------------------------------------------------ zsort
@pytest.mark.parametrize("n_cu", N_CUS)
@pytest.mark.parametrize("save_Z", (0, 1))
def test_zsort_dense_control(n_cu, save_Z):
    """The regime every chain-level test is in: no empty column, no block without one."""
    for K, G, N in ((96, 2 * n_cu + 3, 20), (96, max(1, n_cu // 2), 8), (33, 5 * n_cu, 24)):
        M = dense(K, G)
        p = zsort_plan(M, N, save_Z, n_cu)
        assert p.ok
        r = check_zsort(M, N, save_Z, n_cu, p)
        assert p.nempty == 0 and (r["guests"] == 0).all()
        assert p.qmax in (64, 32, 16, 8, 4)


@pytest.mark.parametrize("n_cu", N_CUS)
@pytest.mark.parametrize("save_Z", (0, 1))
@pytest.mark.parametrize("kind", ("quarter", "twentieth", "two", "one", "none"))
def test_zsort_sparse_columns_leave_blocks_without_a_column(n_cu, save_Z, kind):
    """G in (n_cu, 2 n_cu] with 25 %, 5 %, two, one and no non-empty column: the all-zero columns pile onto the lightest blocks and the last
    blocks of the grid get none.  Their set-up still reads cols[col0]: it must be inside the uploaded list."""
    K, N, G = 96, 20, _g_sparse(n_cu)
    nonempty = {"quarter": max(1, G // 4), "twentieth": max(1, G // 20), "two": 2, "one": 1, "none": 0}[kind]
    M = sparse(K, G, nonempty)
    p = zsort_plan(M, N, save_Z, n_cu)
    assert p.ok and p.nb == n_cu and p.GBc == 2
    check_zsort(M, N, save_Z, n_cu, p)
    # (on 4 CUs two non-empty columns and three empty ones fill all four blocks: G <= 4 would be needed)
    assert _expect_empty(M, p) or (n_cu == 4 and kind == "two"), "the case does not reach the regime it is meant for"
    assert (p.nempty > 0) == _expect_empty(M, p)
    if p.nempty:
        assert p.blocks[-1, 3] == 0, "expected the last block among those without a column"
        assert p.blocks[-1, 2] == p.cols.size - 1                                   # its col0 is the trailing entry
    assert p.qmax in (64, 32, 16, 8, 4)


def test_zsort_issue_example_300_columns_80_nonempty():
    """The replay of the issue: 256 blocks, G = 300, 80 non-empty columns: GBc = 2, blocks 190..255 without a column; all-zero M: 150..255."""
    M = sparse(96, 300, 80)
    p = zsort_plan(M, 20, 0, 256)
    r = check_zsort(M, 20, 0, 256, p)
    assert p.GBc == 2 and np.array_equal(np.nonzero(r["ncols"] == 0)[0], np.arange(190, 256))
    M = np.zeros((96, 300), np.int32, order="F")
    p = zsort_plan(M, 20, 0, 256)
    r = check_zsort(M, 20, 0, 256, p)
    assert np.array_equal(np.nonzero(r["ncols"] == 0)[0], np.arange(150, 256))


@pytest.mark.parametrize("n_cu", N_CUS)
def test_zsort_column_list_a_page_long(n_cu):
    """G a multiple of 1,024 with a sparse tail: the column list is exactly a page (4,096 bytes per 1,024 columns) before its trailing entry."""
    K, N = 16, 10
    G = 1024 * max(1, -(-(n_cu + 1) // 1024))                                       # > n_cu
    M = sparse(K, G, G // 16)
    M[:, G - G // 4:] = 0                                                           # the tail of the column range is empty
    for save_Z in (0, 1):
        p = zsort_plan(M, N, save_Z, n_cu)
        assert p.ok
        check_zsort(M, N, save_Z, n_cu, p)
        assert int(p.blocks[:, 3].sum()) == G                                       # the listed columns: whole pages of 1,024 ints
        assert (p.nempty > 0) == _expect_empty(M, p)


@pytest.mark.parametrize("n_cu", N_CUS)
@pytest.mark.parametrize("save_Z", (0, 1))
def test_zsort_column_counts_around_the_cu_count(n_cu, save_Z):
    """G < n_cu, = n_cu, = n_cu + 1 and 64 n_cu + 1 (a block holds 64 columns at most: twice as many blocks as CUs), dense and sparse."""
    K, N = 12, 6
    for G in (max(1, n_cu - 1), n_cu, n_cu + 1, 64 * n_cu + 1):
        for M in (dense(K, G), sparse(K, G, max(1, G // 20), seed=G)):
            p = zsort_plan(M, N, save_Z, n_cu)
            assert p.ok
            check_zsort(M, N, save_Z, n_cu, p)
            assert p.nb == (min(G, n_cu) if G <= 64 * n_cu else min(G, 2 * n_cu)) and p.nb * p.GBc >= G
            if G <= n_cu:
                assert p.nempty == 0 and p.GBc == 1                                 # one block per column: none can be empty


def _sparse_with_large_cells(n_cu, big=(300_000, 10_000_000)):
    K, G = 96, _g_sparse(n_cu)
    M = sparse(K, G, max(1, G // 8), seed=11)
    nz = np.nonzero(M.sum(0) > 0)[0]
    M[40, nz[0]] = big[0]
    if len(big) > 1:
        M[5, nz[-1]] = big[1]                                                       # (the same column where there is one only: 4 CUs)
    return M


@pytest.mark.parametrize("n_cu", N_CUS)
def test_zsort_large_cells_are_exported_into_blocks_without_a_column(n_cu):
    """Sparse data plus a cell of 300,000 and one of 10,000,000 counts: the exported units go to the lightest blocks, which are the ones
    without a column of their own — guest-only blocks."""
    M = _sparse_with_large_cells(n_cu)
    p = zsort_plan(M, 20, 0, n_cu)
    assert p.ok and p.shared and not p.it16 and p.qmax in (32, 64)
    r = check_zsort(M, 20, 0, n_cu, p)
    guest_only = (r["nown"] == 0) & (r["guests"] > 0)
    assert guest_only.any(), "no block has guests and no own column"
    assert p.nempty == int((r["nown"] == 0).sum())
    assert not p.pk
    # with save_Z a 300,000-count cell is beyond the 16-bit halves of k_zexpand's slab: declined, the register kernel takes the handle
    assert not zsort_plan(M, 20, 1, n_cu).ok


def test_zsort_large_cells_spread_off(monkeypatch):
    """BNMF_ZSSPREAD=0: every cell at home, nobody has guests; the empty blocks stay empty."""
    M = _sparse_with_large_cells(256, big=(300_000,))
    monkeypatch.setenv("BNMF_ZSSPREAD", "0")
    p = zsort_plan(M, 20, 0, 256)
    assert p.ok and not p.shared
    r = check_zsort(M, 20, 0, 256, p)
    assert (r["guests"] == 0).all() and p.nempty > 0


@pytest.mark.parametrize("n_cu", N_CUS)
def test_zsort_units_come_back_to_their_owner(n_cu):
    """A column of several 20,000-count cells whose block is the lightest (every other column is heavier than what the cells keep at home):
    the first units are dealt back to the owner, which works on them through the own column's slot, beside the cells' first fragments."""
    rng = np.random.default_rng(5)
    K = 96
    for G in (n_cu, 2 * n_cu):                                                      # (every block as many columns: the owner's is the lightest)
        M = np.asfortranarray(rng.poisson(500.0, size=(K, G)).astype(np.int32))      # ~48,000 per column, no large cell
        M[:, 3] = 0
        M[3:9, 3] = 20_000                                                          # 6 x 16 x 128 = 12,288 counts stay at home
        p = zsort_plan(M, 20, 0, n_cu)
        assert p.ok and p.shared
        r = check_zsort(M, 20, 0, n_cu, p)
        assert r["units_at_home"] > 0 and r["units_away"] > 0
    # sparse: the column with the large cells is the only one with counts
    M2 = np.zeros((K, _g_sparse(n_cu)), np.int32, order="F")
    M2[3:9, 1] = 20_000
    p = zsort_plan(M2, 20, 0, n_cu)
    assert p.ok and p.shared
    r = check_zsort(M2, 20, 0, n_cu, p)
    assert r["units_away"] > 0 and (p.nempty > 0) == _expect_empty(M2, p)


@pytest.mark.parametrize("n_cu", (4, 256))
def test_zsort_item_width_and_rank_boundaries(n_cu, monkeypatch):
    """K = 127 / 128: 2-byte items hold 7 bits of row.  K = 1,024 / 1,025: the planner declines above 1,024 rows (10 bits)."""
    G = _g_sparse(n_cu)
    monkeypatch.setenv("BNMF_ZSQMAX", "64")                                         # (8 fragments of 256 counts: a 2,048-count cell fits 2-byte items)
    for K, it16 in ((127, 1), (128, 0)):
        M = sparse(K, G, max(2, G // 4))
        M[K - 1, np.nonzero(M.sum(0))[0][0]] = 2048                                 # the last row, the largest cell 2-byte items take
        p = zsort_plan(M, 8, 0, n_cu)
        assert p.ok and p.it16 == it16
        check_zsort(M, 8, 0, n_cu, p)
        monkeypatch.setenv("BNMF_ZSIT16", "0")
        q = zsort_plan(M, 8, 0, n_cu)
        monkeypatch.delenv("BNMF_ZSIT16")
        assert q.ok and not q.it16 and q.qmax == p.qmax
        check_zsort(M, 8, 0, n_cu, q)
        assert np.array_equal(q.items, p.items) and np.array_equal(q.blocks, p.blocks) and np.array_equal(q.cols, p.cols)
    for K, ok in ((1024, 1), (1025, 0)):
        M = sparse(K, n_cu + 2, 2)
        M[K - 1, :] += 1
        p = zsort_plan(M, 5, 0, n_cu)
        assert p.ok == ok
        if ok:
            check_zsort(M, 5, 0, n_cu, p)
    assert not zsort_plan(sparse(8, 12, 3), 25, 0, n_cu).ok                          # N = 25 is the step kernel's


@pytest.mark.parametrize("n_cu", (4, 104))
@pytest.mark.parametrize("qmax", (0, 4, 8, 16, 32, 64))
def test_zsort_fragment_field_of_2_byte_items(n_cu, qmax, monkeypatch):
    """A 2-byte item has 3 bits of fragment index: cells of exactly 8 * 4 * qmax counts fit, one count more does not.  A forced BNMF_ZSQMAX
    is the plan's qmax; the default is one of the five candidates."""
    K, N, G = 40, 12, _g_sparse(n_cu)
    if qmax:
        monkeypatch.setenv("BNMF_ZSQMAX", str(qmax))
    base = sparse(K, G, max(2, G // 4))
    base = np.minimum(base, 16)
    c = np.nonzero(base.sum(0))[0][0]
    q0 = zsort_plan(base, N, 0, n_cu).qmax
    assert q0 == (qmax or q0) and q0 in (64, 32, 16, 8, 4)
    for q in ((qmax,) if qmax else (64, 32, 16, 8, 4)):
        for extra, it16 in ((0, 1), (1, 0)):
            M = base.copy(order="F")
            M[K - 1, c] = 8 * 4 * q + extra
            p = zsort_plan(M, N, 0, n_cu)
            assert p.ok
            check_zsort(M, N, 0, n_cu, p)
            if qmax:
                assert p.qmax == qmax
            if p.qmax == q:                                                         # (the default may choose another q for this data)
                assert p.it16 == it16, (q, extra)
            assert p.it16 == (int(M.max()) <= 8 * 4 * p.qmax)


@pytest.mark.parametrize("n_cu", (4, 256))
def test_zsort_pk_boundary(n_cu, monkeypatch):
    """Two factors per word (pk) only while every column total and every block row total stays below 65,536."""
    K, N, G = 24, 6, _g_sparse(n_cu)
    for tot, pk in ((65535, 1), (65536, 0)):
        M = sparse(K, G, 2, seed=2)
        c = np.nonzero(M.sum(0))[0][0]
        M[:, c] = 0
        M[:, c] = tot // K
        M[0, c] += tot - int(M[:, c].sum())
        assert int(M[:, c].sum()) == tot and int(M.max()) <= 8192
        p = zsort_plan(M, N, 0, n_cu)
        assert p.ok and p.pk == pk, tot
        check_zsort(M, N, 0, n_cu, p)
    # a block's row total: two columns of one block, 32,768 + 32,768 in the same row, each column below 65,536
    nbk = max(1, n_cu // 8)
    G2 = 16 * nbk
    M = np.ones((K, G2), np.int32, order="F")
    M[0, :] = 8000
    p = zsort_plan(M, N, 0, nbk)                                                    # 16 columns per block: 128,000 per block in row 0
    assert p.ok and p.GBc == 16 and not p.pk and int(M.sum(0).max()) < 65536
    check_zsort(M, N, 0, nbk, p)
    monkeypatch.setenv("BNMF_ZSPK", "0")
    M = dense(K, G2)
    p = zsort_plan(M, N, 0, n_cu)
    assert p.ok and not p.pk
    check_zsort(M, N, 0, n_cu, p)


@pytest.mark.parametrize("n_cu", (4, 256))
def test_zsort_save_z_largest_cell(n_cu):
    """save_Z: a cell's counts per factor meet as 16-bit halves in k_zexpand's slab — 65,535 counts are taken, 65,536 declined."""
    K, N, G = 24, 6, _g_sparse(n_cu)
    for mx, ok in ((65535, 1), (65536, 0)):
        M = sparse(K, G, 3, seed=4)
        M[K - 1, np.nonzero(M.sum(0))[0][0]] = mx
        p = zsort_plan(M, N, 1, n_cu)
        assert p.ok == ok
        if ok:
            r = check_zsort(M, N, 1, n_cu, p)
            assert not p.shared and (r["guests"] == 0).all() and not p.pk
            assert (p.nempty > 0) == _expect_empty(M, p) and (p.nempty > 0 or n_cu == 4)
        q = zsort_plan(M, N, 0, n_cu)                                               # without save_Z both are large cells, spread
        assert q.ok and q.shared
        check_zsort(M, N, 0, n_cu, q)


# ------------------------------------------------------------------ zstep
@pytest.mark.parametrize("n_cu", N_CUS)
@pytest.mark.parametrize("N", (25, 30, 100))
def test_zstep_dense_and_sparse(n_cu, N):
    K = 70                                                                          # three row chunks, the last one short
    for G in (max(1, n_cu - 1), n_cu, n_cu + 1, _g_sparse(n_cu), 3 * n_cu + 1):
        for M in (dense(K, G), sparse(K, G, max(1, G // 4)), sparse(K, G, min(2, G)), sparse(K, G, 1), np.zeros((K, G), np.int32, order="F")):
            p = zstep_plan(M, N, 0, n_cu)
            assert p.rc == 0 and p.ok
            check_zstep(M, N, n_cu, p)
            assert p.it16


@pytest.mark.parametrize("n_cu", (4, 304))
def test_zstep_batches_and_item_width(n_cu, monkeypatch):
    """More columns per workgroup than a batch holds (GBP); fragment index 30 / 31 (the 2-byte form has 5 bits, 31 with column 63 would
    be the sentinel); both batch sizes; the 4-byte form forced."""
    K, N = 40, 30
    G = 90 * n_cu + 7 if n_cu == 4 else 2 * n_cu + 1
    for mx, it16 in ((31 * 4 * ZP_QMAX, 1), (31 * 4 * ZP_QMAX + 1, 0)):               # 31 fragments: indices 0..30; one count more: index 31
        M = sparse(K, G, max(2, G // 3), seed=9)
        M[K - 1, np.nonzero(M.sum(0))[0][0]] = mx
        for gbp in ("32", "40"):
            monkeypatch.setenv("BNMF_ZPGB", gbp)
            p = zstep_plan(M, N, 0, n_cu)
            assert p.ok and p.GBP == int(gbp) and p.it16 == it16 and p.maxfrag == (30 if it16 else 31)
            check_zstep(M, N, n_cu, p)
            if n_cu == 4:
                assert (p.wgs[:, 1] > 1).any()                                      # several batches per workgroup
        monkeypatch.delenv("BNMF_ZPGB")
    monkeypatch.setenv("BNMF_ZPIT16", "0")
    p = zstep_plan(M, N, 0, n_cu)
    assert p.ok and not p.it16
    check_zstep(M, N, n_cu, p)


def test_zstep_declines():
    M = dense(40, 50)
    assert not zstep_plan(M, 24, 0, 256).ok and not zstep_plan(M, 101, 0, 256).ok     # N <= 24: the register / sorted kernels; > 100: tile
    assert not zstep_plan(M, 30, 1, 256).ok                                          # save_Z
