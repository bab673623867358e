"""bnmf_map / bnmf_map_at on the device (map_impl in csrc/api.hip; k_map_colsum, k_map_stats, k_map_quant, k_map_fit in csrc/kernels.h)
against their numerical spec restated in numpy float64 (tests/map_ref.py): every output of every case bit for bit, np.uint64 views, no
tolerance.  tests/test_gpu_map.py keeps the independent comparison with numpy / np.quantile; tests/test_map_host.py pins the
restatement on the CPU and records what the chains hold.

Small shapes (tests/map_cases.py): window = 16, run to iteration 40, so the ring wraps; map(end_iter = iter - 2, n_samples = 12) and
map of the last 10.  K < 64 and K N, N G no multiple of 8 (k7: the `live` tail of k_map_quant, the early return of k_map_stats), N = 1,
three 64-row passes of the column sums (pg_k130), N = 151, real-valued data with 13 negative cells under the KL clip (normal), rings of
the MH sweep (ptn_mh), rank learning (rank_n3, seed 3: 5 patterns with counts [3, 3, 3, 2, 1] / [3, 3, 2, 1, 1], n_used = 3 with gaps in
the slot list, across the wrap; sbfi: a pattern per sample, the mode all zeros), a fixed column of P (fix1: a constant series, whose
mean and bounds are the constant's bits) and an MH chain with every column fixed (fixall_mh: 20 / 19 of the 21 elements of E repeat a
value inside the range, some in every sample) — figures from the CPU oracle, asserted here from the device's window.

Routes: one K = 5, G = 3, N = 2 chain with window 2,100 at iteration 2,150, bnmf_map_at over 1 .. 2,100 samples (R = 16 up to 1,024
samples, R = 32 up to 2,048, k_map_stats above), four of the ranges across the ring's wrap, ci in {0.95, 0.5, 0.999, 0.002} (the last
makes the two chains of draws cross up to 65 samples); above 2,048 samples the ci that kt admits, kt = 160 (the whole opt-in LDS)
included, and kt = 161 refused."""
import ctypes as C

import numpy as np
import pytest

import map_cases as MC
import map_ref as R

pytestmark = pytest.mark.gpu

W, T_END = MC.W, MC.T_END
RANGES = ((T_END - 2, MC.N_RANGE), (T_END, 10))
ROUTE_RANGES = ((1, 2150), (2, 2102), (3, 2103), (63, 2120), (64, 2150), (65, 2100), (1023, 2150), (1024, 2150), (1025, 2140),
                (2047, 2149), (2048, 2150), (2049, 2150), (2100, 2150))
ROUTE_CI = (0.95, 0.5, 0.999, 0.002)
CI_KT160, CI_KT161 = 0.849, 0.848                              # over 2,100 samples
OUT = ("P", "E", "A", "top_A", "P_lower", "P_upper", "E_lower", "E_upper", "rmse", "kl")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _call(e, end, n, ci, bounds=True, means=True, at=True):
    """bnmf_map_at (or bnmf_map: end is then iter) through lib() with every output, top_A whole; the return code and the outputs"""
    from bayesnmf_amd.engine import lib, BnmfMapInfo
    K, G, N = e.K, e.G, e.N
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    Pm, Em = (np.full(K * N, np.nan), np.full(N * G, np.nan)) if means else (None, None)
    Am, top = np.full(N, np.nan), np.full(5 * N, np.nan)
    Pl, Pu, El, Eu = (np.full(K * N, np.nan), np.full(K * N, np.nan), np.full(N * G, np.nan), np.full(N * G, np.nan)) if bounds else (None,) * 4
    used = np.full(n, -1, dtype=np.int32)
    info = BnmfMapInfo()
    args = (float(ci) if ci else 0.0, dp(Pm), dp(Em), dp(Am), dp(top), dp(Pl), dp(Pu), dp(El), dp(Eu), used.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(info))
    rc = lib().bnmf_map_at(e._h, int(end), int(n), *args) if at else lib().bnmf_map(e._h, int(n), *args)
    f = lambda a, shp: None if a is None else a.reshape(shp, order="F")   # noqa: E731
    has = bool(ci) and bounds
    return rc, dict(P=f(Pm, (K, N)), E=f(Em, (N, G)), A=Am, top_A=top.reshape(5, N), used=used,
                    P_lower=f(Pl, (K, N)) if has else None, P_upper=f(Pu, (K, N)) if has else None,
                    E_lower=f(El, (N, G)) if has else None, E_upper=f(Eu, (N, G)) if has else None,
                    n_used=info.n_used, n_patterns=info.n_patterns, top_counts=[int(c) for c in info.top_counts], rmse=info.rmse, kl=info.kl)


def _map(e, end, n, ci, **kw):
    rc, out = _call(e, end, n, ci, **kw)
    assert rc == 0, rc
    return out


def _differences(tag, a, b, names=OUT):
    """the names of the outputs of a that are not b's, bit for bit (printed with the first place they differ)"""
    bad = []
    for k in names:
        if a[k] is None or b[k] is None:
            if not (a[k] is None and b[k] is None):
                print(f"map[{tag}] {k}: one of the two is missing")
                bad.append(k)
            continue
        x, y = np.atleast_1d(np.asarray(a[k], dtype=np.float64)), np.atleast_1d(np.asarray(b[k], dtype=np.float64))
        if x.shape != y.shape:
            print(f"map[{tag}] {k}: shapes {x.shape} and {y.shape}")
            bad.append(k)
            continue
        ne = _bits(x) != _bits(y)
        if ne.any():
            i = tuple(np.argwhere(ne)[0])
            print(f"map[{tag}] {k}: {int(ne.sum())} of {ne.size} differ, first at {i}: {x[i]!r} against {y[i]!r}")
            bad.append(k)
    for k in ("n_used", "n_patterns", "top_counts"):
        if a[k] != b[k]:
            print(f"map[{tag}] {k}: {a[k]!r} against {b[k]!r}")
            bad.append(k)
    if not np.array_equal(np.asarray(a["used"]), np.asarray(b["used"])):
        print(f"map[{tag}] used: {a['used']} against {b['used']}")
        bad.append("used")
    return bad


def _same(a, b, names=OUT):
    assert not _differences("equivalence", a, b, names)


def _fresh(case, window=W):
    from bayesnmf_amd import Engine
    e, M = MC.create(Engine, case, window=window)
    return e, M, e.init()


_RUNS = {}


def _run(case):
    """the chain at iteration 40 (the route chain: 2,150) and its metric rows: made once per case"""
    if case in _RUNS:
        return _RUNS[case]
    if case == "route":
        e, M, row1 = _fresh(case, MC.ROUTE_W)
        e.run(MC.ROUTE_END - 1, metrics=False)
        assert e.iter == MC.ROUTE_END
        _RUNS[case] = dict(e=e, M=M, rows=None)
        return _RUNS[case]
    MH = MC.CASES[case][5]
    e, M, row1 = _fresh(case)
    rows = np.vstack([row1[None, :], e.run(T_END - 1, converged=MH)])
    assert e.iter == T_END
    _RUNS[case] = dict(e=e, M=M, rows=rows)
    return _RUNS[case]


def _window(e, end, n):
    """P [n][K][N], E [n][N][G], A [n][N] of the n samples that end at iteration end"""
    back = e.iter - (end - n)
    return tuple(np.stack(e.window(nm, back)[:n]) for nm in ("P", "E", "A"))


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for r in _RUNS.values():
        r["e"].close()
    _RUNS.clear()


@pytest.mark.parametrize("case", MC.MAP_CASES)
def test_every_output_is_the_restatement_bit_for_bit(case, oracle_lib):
    r = _run(case)
    e, M = r["e"], r["M"]
    bad = []
    for end, n in RANGES:
        Pw, Ew, Aw = _window(e, end, n)
        Aw = Aw.reshape(n, e.N)
        ref = R.map_reference(Pw, Ew, Aw, M, 0.95)
        dev = _map(e, end, n, 0.95)
        print(f"map[{case}] {end - n + 1}..{end}: n_used {dev['n_used']} of {n}, {dev['n_patterns']} patterns {dev['top_counts']}, rmse {dev['rmse']!r} kl {dev['kl']!r}")
        bad += _differences(f"{case}, {end - n + 1}..{end}", dev, ref)
        bad += _differences(f"{case}, {end - n + 1}..{end}, no bounds", _map(e, end, n, None), R.map_reference(Pw, Ew, Aw, M, None))
        used = ref["used"] == 1
        _, x, es = R.renormalised(Pw[used], Ew[used])
        if case == "rank_n3":                                  # the chain still holds what the oracle rehearsal showed
            assert dev["n_patterns"] == 5 and dev["top_counts"] == ([3, 3, 3, 2, 1] if n == 12 else [3, 3, 2, 1, 1])
            assert 2 <= dev["n_used"] < n and (np.diff(np.where(dev["used"])[0]) > 1).any() and list(dev["A"]) == [0.0, 1.0, 0.0]
        if case == "sbfi":
            assert dev["n_patterns"] == n and dev["n_used"] == 1 and not dev["A"].any()
        if case == "normal":
            assert (np.asarray(M) < 0).sum() == 13
        if case == "fix1":                                     # ties (a): a fixed column is one value in every sample
            v = x[0][:, 1]
            assert (x[:, :, 1] == v[None, :]).all()
            for k in ("P", "P_lower", "P_upper"):
                assert np.array_equal(_bits(dev[k][:, 1]), _bits(v)), k
        if case == "fixall_mh":                                # ties (b): rejected E proposals repeat the renormalised value
            share, most = MC.repeated_values(es.reshape(n, -1))
            print(f"map[{case}] {share:.3f} of the E elements repeat a value inside the range, one holds a value {most} times")
            assert share >= 0.25 and most >= 3
            assert (x == x[0][None]).all() and np.array_equal(_bits(dev["P"]), _bits(x[0]))
    assert not bad, bad


def _admitted(n, ci):
    return n <= 2048 or R.order_stats(n, ci)[4] <= 160


def test_every_route_and_boundary_bit_for_bit(oracle_lib):
    r = _run("route")
    e, M = r["e"], r["M"]
    assert R.order_stats(2100, CI_KT160)[4] == 160 and R.order_stats(2100, CI_KT161)[4] == 161
    wraps = [(n, end) for n, end in ROUTE_RANGES if end - n + 1 <= MC.ROUTE_W + 1 < end]     # iteration 2,101 sits in the ring's last slot
    assert len(wraps) >= 2
    bad, done = [], 0
    for n, end in ROUTE_RANGES:
        Pw, Ew, Aw = _window(e, end, n)
        for ci in ROUTE_CI + ((CI_KT160,) if n == 2100 else ()):
            if not _admitted(n, ci):
                continue
            ref = R.map_reference(Pw, Ew, Aw.reshape(n, e.N), M, ci)
            bad += _differences(f"route, n = {n} ending at {end}, ci = {ci}", _map(e, end, n, ci), ref)
            done += 1
    print(f"map[route] {done} calls, ranges across the wrap {wraps}")
    assert [ci for ci in ROUTE_CI if _admitted(2049, ci)] == [0.95, 0.999] and done == 11 * 4 + 2 + 3
    assert not bad, bad


def test_kt_161_is_refused_and_the_handle_stays_usable():
    from bayesnmf_amd.engine import lib
    e = _run("route")["e"]
    before = _map(e, 2150, 2100, CI_KT160)
    rc, _ = _call(e, 2150, 2100, CI_KT161)
    msg = lib().bnmf_last_error().decode()
    assert rc == -1 and "161 order statistics" in msg and "limit 160" in msg, (rc, msg)          # BNMF_EINVAL
    _same(before, _map(e, 2150, 2100, CI_KT160))
    _same(_map(e, 2150, 64, 0.95), _map(e, 2150, 64, 0.95))


@pytest.mark.parametrize("case", ["k7", "rank_n3", "normal", "fixall_mh"])
def test_equivalent_calls_give_the_same_bits(case):
    e = _run(case)["e"]
    end, n = RANGES[0]
    a = _map(e, end, n, 0.95)
    _same(a, _map(e, end, n, 0.95))                                                                # a second call
    _same(_map(e, e.iter, 10, 0.95), _map(e, e.iter, 10, 0.95, at=False))                          # bnmf_map is bnmf_map_at(iter)
    m = e.map(n, 0.95, end_iter=end)                                                               # the wrapper gives these arrays
    for k in ("P", "E", "P_lower", "E_upper"):
        assert np.array_equal(_bits(m[k]), _bits(a[k])), k
    means = ("P", "E", "A", "top_A", "rmse", "kl")
    _same(a, _map(e, end, n, None), means)                                                         # ci = None: the means of k_map_stats
    _same(a, _map(e, end, n, 0.95, bounds=False), means)                                           # the four bound pointers NULL
    info_only = _map(e, end, n, 0.95, means=False)                                                 # no mean asked for: the same bounds and fit
    _same(a, info_only, ("A", "top_A", "P_lower", "P_upper", "E_lower", "E_upper", "rmse", "kl"))


def test_the_means_of_the_three_kernels_are_equal():
    """k_map_quant at R = 16 and R = 32 and k_map_stats (ci = None, NULL bounds, and above 2,048 samples) give one mean"""
    e = _run("route")["e"]
    means = ("P", "E", "A", "rmse", "kl")
    for n, end in ((64, 2150), (1024, 2150), (1025, 2140), (2048, 2150)):
        a = _map(e, end, n, 0.95)
        _same(a, _map(e, end, n, None), means)
        _same(a, _map(e, end, n, 0.5, bounds=False), means)
        _same(a, _map(e, end, n, 0.002), means)
    _same(_map(e, 2150, 2100, 0.95), _map(e, 2150, 2100, None), means)


@pytest.mark.parametrize("case", ["pg_k96", "ptn_mh", "rank_n3"])
def test_the_call_is_read_only_for_the_chain(case):
    """a chain that calls map mid-run continues with the bits of a twin that never did"""
    r = _run(case)
    MH = MC.CASES[case][5]
    _map(r["e"], *RANGES[0], 0.95); _map(r["e"], *RANGES[1], None)
    b, _, row1 = _fresh(case)
    rows_b = np.vstack([row1[None, :], b.run(T_END - 1, converged=MH)])
    assert np.array_equal(_bits(rows_b), _bits(r["rows"]))
    more_a, more_b = r["e"].run(10, converged=MH), b.run(10, converged=MH)
    assert np.array_equal(_bits(more_a), _bits(more_b))
    for nm in ("P", "E", "A"):
        assert np.array_equal(_bits(r["e"].get(nm)), _bits(b.get(nm))), nm
    b.close()
    _RUNS.pop(case)["e"].close()                                                 # (this case's chain has moved on)


@pytest.mark.parametrize("case", ["pg_k8", "normal"])
def test_a_reopened_chain_gives_the_same_map(case, tmp_path):
    from bayesnmf_amd import Engine
    r = _run(case)
    path = str(tmp_path / "state.bin")
    r["e"].save_state(path)
    c, _ = MC.create(Engine, case, window=W)
    assert c.load_state(path) == T_END
    for end, n in RANGES:
        _same(_map(r["e"], end, n, 0.95), _map(c, end, n, 0.95))
    c.close()
