"""GPU parity on the schedules no other test runs: data with all-zero columns at G between one and two times the device's CU count,
where the sorted schedule leaves blocks WITHOUT A COLUMN (the last ones of the grid among them), alone and with large cells exported
into exactly those blocks; the same data through k_zalloc_step and the tile kernel; and a "second life" — a handle whose pooled device
blocks were last used by another chain of the same shape.  Engine against the oracle, bit for bit.  The contract of the schedule itself
is checked on the host (tests/test_schedule_host.py), which must pass before this file runs on a device."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
K = 96


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count                 # hipDeviceProp_t::multiProcessorCount: what bnmf_create plans for


def _sparse(G, nonempty, seed=5, big=()):
    rng = np.random.default_rng(seed)
    M = np.zeros((K, G), np.int32, order="F")
    idx = np.sort(rng.choice(G, size=nonempty, replace=False)) if nonempty else np.zeros(0, np.int64)
    M[:, idx] = rng.poisson(rng.gamma(0.7, 30.0, size=(K, idx.size)))
    for i, m in enumerate(big):
        M[40 - 7 * i, idx[i * (idx.size - 1)]] = m
    return M


def _plan(M, N, save_Z, n_cu):
    """the host's plan for this data (bnmf_test_zsort_plan): blocks, blocks without an own column, and whether the last block has none at all"""
    from bayesnmf_amd.engine import lib
    L = lib()
    L.bnmf_test_zsort_plan.argtypes = [C.c_int] * 5 + [C.c_void_p, C.POINTER(C.c_longlong)] + [C.c_void_p] * 5
    M = np.asfortranarray(M, dtype=np.int32)
    d = (C.c_longlong * 14)()
    assert L.bnmf_test_zsort_plan(K, M.shape[1], N, int(save_Z), n_cu, M.ctypes.data, d, None, None, None, None, None) == 0
    assert d[0] == 1
    blocks, items = np.zeros((int(d[3]), 4), np.int32), np.zeros(int(d[11]), np.uint32)
    assert L.bnmf_test_zsort_plan(K, M.shape[1], N, int(save_Z), n_cu, M.ctypes.data, d, blocks.ctypes.data, None, items.ctypes.data, None, None) == 0
    last = items[blocks[-1, 0]:blocks[-1, 0] + 64 * blocks[-1, 1]] if blocks[-1, 1] else np.zeros(0, np.uint32)
    # (every cell of an own column has its fragment 0 — the lane that leaves Mhat — at home: a block without one owns no column)
    last_owns_none = not ((last != 0xFFFFFFFF) & ((last >> 16) == 0)).any()
    return int(d[3]), int(d[9]), blocks, last_owns_none


def _mk(cls, M, N, prior="gamma", **kw):
    from bayesnmf_amd.setup import apply_hyperprior_params
    c = cls(M, N, prior=prior, **kw)
    # (an all-zero M has mean 0, which no default hyper-prior is defined for: the defaults of a mean of one count per cell, on both sides)
    apply_hyperprior_params(c, prior, M if np.any(M) else np.ones((1, 1)), N)
    return c


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _has_empty_blocks(e, M, N, save_Z, guest_only=False):
    """stat(6) / stat(7): the handle RAN on a schedule with blocks that own no column, the last block of the grid among them"""
    n_cu = _n_cu()
    nb, nempty, blocks, last_owns_none = _plan(M, N, save_Z, n_cu)
    assert e.stat(5) > 0, "the handle is not on the sorted schedule"
    assert e.stat(6) == nb == n_cu and e.stat(7) == nempty > 0 and last_owns_none
    if guest_only is None:
        pass
    elif guest_only:
        assert blocks[-1, 3] > 0 and blocks[-1, 1] > 0                                # the last block owns no column, but hosts guests and has tasks
    else:
        assert blocks[-1, 3] == 0 and blocks[-1, 1] == 0                              # no column at all, no task


def _parity(M, N, save_Z=False, steps=(3, 2), seed=3, empty="sorted", guest_only=False, **kw):
    import oracle as O
    from bayesnmf_amd import Engine
    o = _mk(O.Oracle, M, N, seed=seed, save_Z=save_Z, nthreads=16, **kw)
    e = _mk(Engine, M, N, seed=seed, save_Z=save_Z, window=3 if save_Z else 0, **kw)
    if empty == "sorted":
        _has_empty_blocks(e, M, N, save_Z, guest_only)
    r0, r1 = o.init(), e.init()
    assert np.array_equal(r0[:9], r1[:9], equal_nan=True)
    zhist, it = {}, 1
    for n in steps:
        mo = np.empty((n, r0.size))
        me = np.empty((n, r0.size))
        for j in range(n):                                                          # (the oracle one iteration at a time: its Z of every iteration)
            mo[j] = o.run(1)[0]
            it += 1
            if save_Z:
                zhist[it] = o.get("Z").astype(np.int32)
        me = e.run(n)
        for nm in ("ZsumK", "ZsumG"):
            assert np.array_equal(o.get(nm).astype(np.int32), e.get(nm)), nm
        assert e.get("ZsumK").sum() == M.sum() and e.get("ZsumG").sum() == M.sum()
        for nm in ("P", "E"):
            assert np.array_equal(_bits(o.get(nm)), _bits(e.get(nm))), nm
        assert np.array_equal(mo[:, :9], me[:, :9], equal_nan=True), "metric rows"
        if np.any(M):
            assert np.array_equal(_bits(mo[:, :9]), _bits(me[:, :9])), "metric rows"
        if save_Z:
            assert np.array_equal(zhist[it], e.get("Z")), "Z"
            win = e.window("Z", 3)                                                  # the records ring, expanded by k_zexpand when read
            for j, i2 in enumerate(range(it - 2, it + 1)):
                assert np.array_equal(win[j], zhist[i2]), ("window Z", i2)
    e.close()
    o.close()


def _n80(n_cu):
    return max(2, 80 * n_cu // 256)                                                 # 80 non-empty columns on 256 CUs


def _cases(n_cu):
    G = n_cu + 44
    return {"80 columns": (_sparse(G, _n80(n_cu)), 20), "2 columns": (_sparse(G, 2), 8), "no counts": (np.zeros((K, G), np.int32, order="F"), 20)}


@pytest.mark.parametrize("save_Z", [False, True])
@pytest.mark.parametrize("case", ["80 columns", "2 columns", "no counts"])
def test_blocks_without_a_column(case, save_Z):
    """K = 96, G = CUs + 44: 80 non-empty columns at N = 20, two at N = 8, none at all.  Most blocks of the sorted schedule have no column;
    with save_Z they go through k_zexpand and the records ring too."""
    M, N = _cases(_n_cu())[case]
    _parity(M, N, save_Z=save_Z)
    if not np.any(M):
        from bayesnmf_amd import Engine
        e = _mk(Engine, M, N, seed=3)
        e.init(); e.run(3)
        assert not e.get("ZsumK").any() and not e.get("ZsumG").any()
        e.close()


@pytest.mark.parametrize("gate", ["0", "1"])
@pytest.mark.parametrize("cells", [1, 3])
def test_large_cells_exported_into_blocks_without_a_column(cells, gate, monkeypatch):
    """The sparse data plus 300,000-count cells: their units go to the lightest blocks, lowest block number first.  Blocks whose own columns
    are all empty weigh as little as blocks without a column and come first: one cell's 73 units end there (the blocks behind them stay
    without any column), three cells' 219 units reach every weightless block — guest-only blocks, the last of the grid among them.  ZsumK is
    accumulated with atomics and zeroed by the draw kernel that consumed it (two run calls), in the plain and in the merged sweep."""
    monkeypatch.setenv("BNMF_GATE", gate)
    n_cu = _n_cu()
    M = _sparse(n_cu + 44, _n80(n_cu), big=(300_000,))
    if cells == 3:
        nz = np.nonzero(M.sum(0))[0]
        M[11, nz[1]] = 300_000
        M[70, nz[2]] = 300_000
    _parity(M, 20, guest_only=(cells == 3) if n_cu == 256 else None)


@pytest.mark.parametrize("switch,value", [("BNMF_ZSPK", "0"), ("BNMF_ZSPK", "1"), ("BNMF_ZSIT16", "0"), ("BNMF_ZSIT16", "1")])
def test_blocks_without_a_column_in_every_table_form(switch, value, monkeypatch):
    """One / two factors per word in the block tables, 4-byte / 2-byte items: on the first case."""
    monkeypatch.setenv(switch, value)
    monkeypatch.setenv("BNMF_ZSQMAX", "64")                                         # (2-byte items whatever the largest cell: <= 2,048 counts)
    M, N = _cases(_n_cu())["80 columns"]
    assert M.max() <= 2048
    _parity(M, N)


@pytest.mark.parametrize("N,kernel", [(30, "step"), (100, "step"), (30, "tile"), (100, "tile")])
def test_step_and_tile_kernels_on_sparse_columns(N, kernel, monkeypatch):
    """k_zalloc_step (N = 30, 100) and the tile kernel (BNMF_ZSTEP=0) on the same sparse data at G > CUs."""
    if kernel == "tile":
        monkeypatch.setenv("BNMF_ZSTEP", "0")
    n_cu = _n_cu()
    M = _sparse(n_cu + 44, _n80(n_cu))
    from bayesnmf_amd import Engine
    e = _mk(Engine, M, N, seed=3)
    assert e.stat(6) == (n_cu if kernel == "step" else 0) and e.stat(7) == 0         # a workgroup of the step schedule always has a column
    e.close()
    _parity(M, N, empty=None, steps=(3,))


def _temps():
    return np.concatenate([np.zeros(3), 10.0 ** np.linspace(-6, 0, 30), np.ones(1000)])


@pytest.mark.parametrize("model", ["sorted", "save_Z", "mh_pipe", "normal", "rank"])
def test_second_life_of_the_pooled_blocks(model):
    """A handle of the same shape but other data and another seed is run and destroyed first: every pooled device block the handle under
    test takes — the padded column list included — holds ANOTHER chain's contents.  Bit for bit the oracle's chain all the same."""
    import oracle as O
    from bayesnmf_amd import Engine
    n_cu = _n_cu()
    G = n_cu + 44
    if model in ("sorted", "save_Z"):
        N, kw, prior, steps = 20, dict(save_Z=model == "save_Z"), "gamma", (3, 2)
        Mother, M = _sparse(G, _n80(n_cu) * 3 // 2, seed=77), _sparse(G, _n80(n_cu))
    elif model == "mh_pipe":
        N, kw, prior, steps = 6, dict(MH=True), "exponential", (4, 4)
        Mother, M = _sparse(G, _n80(n_cu) * 3 // 2, seed=77), _sparse(G, _n80(n_cu))
    elif model == "normal":
        N, kw, prior, steps = 5, dict(likelihood="normal"), "exponential", (4, 3)
        rng = np.random.default_rng(11)
        mk = lambda: np.asfortranarray(rng.gamma(1.0, 1.0, size=(K, 3)) @ rng.gamma(2.0, 4.0, size=(3, G)) + rng.normal(0.0, 0.5, size=(K, G)))
        Mother, M = mk(), mk()
    else:
        N, kw, prior, steps = 6, dict(learning_rank=True, rank_method="SBFI", temperature=_temps()), "gamma", (12, 12)
        Mother, M = _sparse(G, _n80(n_cu) * 3 // 2, seed=77), _sparse(G, _n80(n_cu))
    win = dict(window=3) if model == "save_Z" else {}
    first = _mk(Engine, Mother, N, prior, seed=991, **win, **kw)
    first.init(); first.run(steps[0], converged=model == "mh_pipe")
    first.close()
    o = _mk(O.Oracle, M, N, prior, seed=3, nthreads=16, **kw)
    e = _mk(Engine, M, N, prior, seed=3, **win, **kw)
    if model in ("sorted", "save_Z"):
        _has_empty_blocks(e, M, N, model == "save_Z")
    if model == "mh_pipe":
        assert e.stat(4) == 1
    r0, r1 = o.init(), e.init()
    assert np.array_equal(_bits(r0[:9]), _bits(r1[:9]))
    for seg, n in enumerate(steps):
        conv = model == "mh_pipe" and seg > 0                                       # MH: the later segment with true accept / reject
        mo, me = o.run(n, converged=conv), e.run(n, converged=conv)
        names = ["P", "E"] + (["A"] if model == "rank" else []) + (["sigmasq"] if model == "normal" else [])
        for nm in names:
            assert np.array_equal(_bits(o.get(nm)), _bits(e.get(nm))), (nm, seg)
        if model != "normal":
            for nm in ("ZsumK", "ZsumG"):
                assert np.array_equal(o.get(nm).astype(np.int32), e.get(nm)), (nm, seg)
        if model == "save_Z":
            assert np.array_equal(o.get("Z").astype(np.int32), e.get("Z")), seg
            assert np.array_equal(e.window("Z", 1)[0], e.get("Z"))
        assert np.array_equal(_bits(mo[:, :9]), _bits(me[:, :9])), seg
    e.close()
    o.close()
