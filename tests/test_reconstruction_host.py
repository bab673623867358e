"""Reconstruction quality per tumour over a recorded range, the parts that need no GPU: the numpy restatement of the spec
(tests/reconstruction_ref.py) against the plain matrix form in extended precision inside a derived bound, its conventions and a planted
case, the library's own finish (csrc/reduce_host.h) as a stand-alone program under the sanitizers, bayesNMF_sampler.get_reconstruction
over a stub engine, and the two new symbols."""
import os
import re
import subprocess

import numpy as np
import pytest

import reconstruction_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(_bits(x)[~np.isnan(x)], _bits(y)[~np.isnan(y)])


def _samples(S, K, G, N, seed):
    rng = np.random.default_rng(seed)
    P = rng.gamma(0.5, 1.0, size=(S, K, N))
    E = rng.gamma(2.0, 20.0, size=(S, N, G))
    A = np.ones((S, N))
    M = rng.poisson(np.einsum("kn,ng->kg", P[0], E[0]))
    return P, E, A, M


@pytest.mark.parametrize("S,K,G,N,seed", [(4, 96, 7, 5, 1), (3, 8, 70, 20, 2), (3, 150, 5, 40, 3)])
def test_restatement_agrees_with_the_matrix_form_inside_a_derived_bound(S, K, G, N, seed):
    """The independent evaluation: C = P diag(A) E, cos = (M . C) / (|M| |C|) by matrix products in extended precision, so that its own
    error (about (K + N) 2^-64) does not count.  The restatement's cosine carries, for data and factors that are not negative (every
    partial sum then has a relative error bounded by its number of roundings, u = 2^-53 each): f_n two products and c at most N
    additions, N + 2; m c one more and at most K additions, dot: K + N + 3; c c twice c's and one, then K: cc: K + 2 N + 5; mm: K + 1;
    mm cc one more, halved by the root, and the root: (2 K + 2 N + 7) / 2 + 1; the division 1: in all fewer than n = 2 K + 2 N + 9
    roundings, so |cos - exact| <= gamma_n = n u / (1 - n u) since cos <= 1.  c_-n has one factor fewer and the same bound; the drop is
    the difference of two cosines and one subtraction: 2 gamma_n + u.  The bound comes from these lengths, not from what is measured."""
    P, E, A, M = _samples(S, K, G, N, seed)
    A[1, N // 2] = 0.0
    r = R.reconstruction_reference(P, E, A, M)
    n = 2 * K + 2 * N + 9
    gam = n * U / (1.0 - n * U)
    L = np.longdouble
    Ml = M.astype(L)
    worst_c = worst_d = 0.0
    for s in range(S):
        PA = P[s].astype(L) * A[s].astype(L)[None, :]
        C = PA @ E[s].astype(L)
        nm = np.sqrt((Ml * Ml).sum(axis=0))
        cos = (Ml * C).sum(axis=0) / (nm * np.sqrt((C * C).sum(axis=0)))
        worst_c = max(worst_c, float(np.abs(r["cos"][s].astype(L) - cos).max()))
        for f in range(N):
            Cn = C - PA[:, f][:, None] * E[s, f].astype(L)[None, :]
            cosn = (Ml * Cn).sum(axis=0) / (nm * np.sqrt((Cn * Cn).sum(axis=0)))
            want = cos - cosn if A[s, f] != 0 else np.zeros(G, dtype=L)
            worst_d = max(worst_d, float(np.abs(r["drops"][s, f].astype(L) - want).max()))
            if A[s, f] == 0:
                assert (r["drops"][s, f] == 0).all() and not np.signbit(r["drops"][s, f]).any() and _same_bits(r["loo"][s, f], r["cos"][s])
    print(f"reconstruction: K {K} N {N}: largest error of cos {worst_c:.3e} (bound {gam:.3e}), of the drop {worst_d:.3e} (bound {2 * gam + U:.3e})")
    assert worst_c <= gam and worst_d <= 2 * gam + U
    # the rows are the moments of the per-sample values
    assert np.allclose(r["tumour"][0], r["cos"].mean(axis=0), rtol=1e-13) and np.allclose(r["tumour"][1], r["cos"].var(axis=0, ddof=1), rtol=1e-8, atol=1e-30)
    assert _same_bits(r["tumour"][2], r["cos"].min(axis=0)) and np.allclose(r["drop"][0], r["drops"].mean(axis=0), rtol=1e-12, atol=1e-17)
    assert np.allclose(r["drop"][2], r["loo"].mean(axis=0), rtol=1e-13) and np.allclose(r["series"], r["cos"].mean(axis=1), rtol=1e-13)
    assert np.array_equal(r["drop"][3], (r["drops"] >= 0.01).mean(axis=0)) and np.array_equal(r["tumour"][5], (r["cos"] >= 0.9).mean(axis=0))
    assert r["tumour"].shape == (6, G) and r["drop"].shape == (4, N, G) and r["series"].shape == (S,) and r["signature"].shape == (3, N)


def test_conventions_are_pinned_exactly():
    S, K, G, N = 5, 12, 6, 3
    P, E, A, M = _samples(S, K, G, N, 9)
    M = M.astype(np.float64)
    M[:, 2] = 0.0                                           # an all-zero tumour: undefined
    E[:, :, 4] = 0.0                                        # a tumour no factor reaches: an empty fit explains nothing
    A[3, :] = 0.0                                           # a sample that excludes every factor
    A[1, 0] = 0.0
    r = R.reconstruction_reference(P, E, A, M, min_cosine=0.5, min_drop=0.01)
    assert r["n_undefined"] == 1 and np.isnan(r["tumour"][[0, 1, 2, 5], 2]).all() and np.isnan(r["drop"][:, :, 2]).all()
    assert r["tumour"][3, 2] == 0.0 and np.isfinite(r["tumour"][4, 2])                      # rel_l1 of t = 0 is 0.0, the rmse is the fit's
    assert not np.isnan(np.delete(r["tumour"], 2, axis=1)).any() and not np.isnan(np.delete(r["drop"], 2, axis=2)).any()
    assert (r["cos"][:, 4] == 0).all() and (r["cos"][3, [0, 1, 3, 4, 5]] == 0).all() and np.isnan(r["cos"][:, 2]).all()
    assert (np.delete(r["drops"][3], 2, axis=1) == 0).all() and (np.delete(r["drops"][1, 0], 2) == 0).all()
    assert r["tumour"][2, 0] == 0.0 and r["tumour"][2, 4] == 0.0                            # the smallest cos: the empty sample's
    assert not np.isnan(r["series"]).any() and r["series"][3] == 0.0
    assert r["worst_at"] == 4 and r["worst_cosine"] == 0.0 and r["n_poor"] >= 1             # tumour 4 is the first with mean cos 0
    assert r["n_needed"] == int((r["drop"][3] >= 0.5).sum()) and r["signature"][0].sum() == r["n_needed"]
    # no defined tumour at all
    z = R.reconstruction_reference(P, E, A, np.zeros((K, G)))
    assert z["n_undefined"] == G and np.isnan(z["series"]).all() and np.isnan(z["signature"][1:]).all() and (z["signature"][0] == 0).all()
    assert z["worst_at"] == -1 and np.isnan(z["worst_cosine"]) and z["n_poor"] == 0 and z["n_needed"] == 0
    # real-valued data with negative cells: defined, and the cosine may be negative
    rng = np.random.default_rng(4)
    n = R.reconstruction_reference(P, E, np.ones((S, N)), rng.normal(0.0, 1.0, size=(K, G)))
    assert n["n_undefined"] == 0 and np.isfinite(n["tumour"]).all() and (n["tumour"][0] < 0.9).all() and (np.abs(n["cos"]) <= 1 + 1e-12).all()


def test_permuting_the_tumours_permutes_tumour_and_drop_bit_for_bit():
    """a tumour's rows depend on its own column of the data and of E alone: not on its place (the series and the signature means sum over
    the tumours in their order and may move in the last bits)"""
    S, K, G, N = 4, 12, 264, 5
    P, E, A, M = _samples(S, K, G, N, 6)
    M[:, [3, 200]] = 0
    A[2, 1] = 0.0
    perm = np.random.default_rng(1).permutation(G)
    a = R.reconstruction_reference(P, E, A, M)
    b = R.reconstruction_reference(P, E[:, :, perm], A, M[:, perm])
    assert _same_bits(b["tumour"], a["tumour"][:, perm]) and _same_bits(b["drop"], a["drop"][:, :, perm])
    assert np.array_equal(b["signature"][0], a["signature"][0]) and _same_bits(b["signature"][2], a["signature"][2])
    assert [b[k] for k in ("n_undefined", "n_poor", "n_needed")] == [a[k] for k in ("n_undefined", "n_poor", "n_needed")]
    assert b["worst_cosine"] == a["worst_cosine"] and perm[b["worst_at"]] == a["worst_at"]
    assert np.allclose(b["series"], a["series"], rtol=1e-14) and np.allclose(b["signature"][1], a["signature"][1], rtol=1e-12, atol=1e-18)


def test_planted_signature_is_needed_by_its_carriers_only():
    """data from 3 signatures, signature 2 active in half of the tumours only: its drop is well above min_drop in the carriers and near 0 in
    the others; an all-zero tumour column is NaN and counted"""
    rng = np.random.default_rng(7)
    K, G, N, S = 24, 9, 3, 20
    P0 = rng.dirichlet(np.full(K, 0.3), size=N).T
    E0 = rng.gamma(8.0, 60.0, size=(N, G))
    carriers = np.arange(G) % 2 == 0
    E0[2, ~carriers] = 0.5                                  # half a mutation against hundreds
    E0[2, carriers] = E0[:2, carriers].sum(axis=0)          # half of a carrier's mutations
    M = rng.poisson(P0 @ E0).astype(np.int32)
    M[:, 8] = 0                                             # (a carrier) all zero
    Ps = P0[None] * rng.uniform(0.97, 1.03, size=(S, K, N))
    Es = E0[None] * rng.uniform(0.97, 1.03, size=(S, N, G))
    r = R.reconstruction_reference(Ps, Es, np.ones((S, N)), M)
    d, p = r["drop"][0], r["drop"][3]
    print("mean cos", r["tumour"][0].round(4), "\ndrop of signature 2", d[2].round(5), "\np_needed\n", p)
    live = np.arange(G) != 8
    assert r["n_undefined"] == 1 and np.isnan(r["tumour"][0, 8]) and np.isnan(d[:, 8]).all() and r["worst_at"] != 8
    assert (r["tumour"][0][live] >= 0.9).all() and r["n_poor"] == 0
    assert (d[2][carriers & live] > 10 * r["min_drop"]).all() and (p[2][carriers & live] == 1.0).all()
    assert (np.abs(d[2][~carriers]) < 1e-3).all() and (p[2][~carriers] == 0.0).all()
    assert r["signature"][0, 2] == (carriers & live).sum() and r["signature"][2, 2] == d[2][live].max()
    assert (p[:2][:, live] == 1.0).all() and r["n_needed"] == 2 * 8 + 4


def test_finish_under_the_sanitizers_is_the_restatement(tmp_path):
    """csrc/reduce_host.h's reconstruction_reduce (the library's own code), built as a stand-alone program with
    -fsanitize=address,undefined: a clean run, and the series, the signature rows and the info fields the restatement's bit for bit;
    edge cases: no defined tumour, S = 2, one tumour, more than 64 defined tumours (a second round of the canonical sum)"""
    exe = str(tmp_path / "reconstruction_reduce_check")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tools", "reconstruction_reduce_check.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", p.stderr
    cases = []
    P, E, A, M = _samples(5, 10, 150, 4, 3)
    M[:, [0, 77, 149]] = 0
    cases.append((P, E, A, M, 0.9))
    cases.append((P[:2], E[:2], A[:2], M, 0.99))                                            # S = 2
    cases.append((P, E, A, np.zeros_like(M), 0.9))                                          # no defined tumour
    cases.append((P[:, :, :1], E[:, :1, :1], A[:, :1], M[:, 1:2], 0.5))                     # N = 1, G = 1
    for P, E, A, M, mc in cases:
        ref = R.reconstruction_reference(P, E, A, M, min_cosine=mc)
        S, N, G = P.shape[0], P.shape[2], M.shape[1]
        drop = np.stack([row.ravel(order="F") for row in ref["drop"]])                     # n + N g
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(np.array([S, N, G], dtype=np.int64).tobytes() + np.array([mc]).tobytes() + np.ascontiguousarray(ref["tumour"]).tobytes() +
                    np.ascontiguousarray(drop).tobytes() + ref["mm"].tobytes() + ref["sums"].tobytes())
        q = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert q.returncode == 0 and q.stderr == "", q.stderr
        out = np.fromfile(dst, dtype=np.float64)
        series, sig, info = np.split(out, np.cumsum([S, 3 * N]))
        assert _same_bits(series, ref["series"]) and _same_bits(sig.reshape(3, N), ref["signature"])
        assert [int(info[0]), int(info[1]), int(info[2]), int(info[4])] == [ref["n_undefined"], ref["n_poor"], ref["n_needed"], ref["worst_at"]]
        assert _same_bits(info[3:4], np.array([ref["worst_cosine"]]))


def test_get_reconstruction_ranges_idx_and_result(tmp_path):
    """bayesNMF_sampler.get_reconstruction over a stub engine: the range and idx rules of get_WAIC (_recorded_range), the defaults, the
    shapes of the result"""
    from test_waic_host import _NoWaicEngine
    from bayesnmf_amd.sampler import bayesNMF_sampler
    from bayesnmf_amd.convergence import new_convergence_control
    from bayesnmf_amd.setup import synth_counts

    class _RecEngine(_NoWaicEngine):
        calls = []

        def reconstruction(self, last_n, used=None, end_iter=None, min_cosine=0.9, min_drop=0.01, drop=True):
            type(self).calls.append(dict(last_n=last_n, used=None if used is None else np.array(used), end_iter=end_iter, min_cosine=min_cosine,
                                         min_drop=min_drop, drop=drop))
            S = last_n if used is None else int(np.sum(used))
            G, N = self.G, self.N
            return dict(n_used=S, n_undefined=1, n_poor=2, n_needed=7, min_cosine=min_cosine, min_drop=min_drop, worst_cosine=0.25, worst_at=3,
                        tumour=np.arange(6.0 * G).reshape(6, G), drop=np.arange(4.0 * N * G).reshape(4, N, G), series=np.arange(float(S)),
                        signature=np.arange(3.0 * N).reshape(3, N))

    M, _, _ = synth_counts(12, 9, 2, 3, mean_total=200)
    cc = new_convergence_control()
    cc.update(MAP_over=4, MAP_every=2, maxiters=10, miniters=2)
    s = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "r"), engine_factory=_RecEngine,
                         convergence_control=cc, save_all_samples=True, periodic_save=False)
    s.run_gibbs_sampler()
    r = s.get_reconstruction()
    c = _RecEngine.calls[-1]
    assert c["last_n"] == 4 and c["end_iter"] is None and c["min_cosine"] == 0.9 and c["min_drop"] == 0.01 and np.array_equal(c["used"], [1, 1, 1, 1])
    assert r["tumour"].shape == (6, 9) and r["drop"].shape == (4, 3, 9) and r["series"].shape == (4,) and r["signature"].shape == (3, 3)
    assert [r[k] for k in ("n_used", "n_undefined", "n_poor", "n_needed", "min_cosine", "min_drop", "worst_cosine", "worst_at")] == [4, 1, 2, 7, 0.9, 0.01, 0.25, 3]
    for i, k in enumerate(("cosine", "cosine_var", "min_cosine_sample", "rel_l1", "rmse", "p_good")):
        assert np.array_equal(r[k], r["tumour"][i]), k
    for i, k in enumerate(("drop_mean", "drop_var", "loo_cosine", "p_needed")):
        assert np.array_equal(r[k], r["drop"][i]) and r[k].shape == (3, 9), k
    r = s.get_reconstruction(end_iter=8, n_samples=5, idx=[4, 6, 8], min_cosine=0.95, min_drop=0.02)
    c = _RecEngine.calls[-1]
    assert c["end_iter"] == 8 and c["last_n"] == 5 and np.array_equal(c["used"], [1, 0, 1, 0, 1]) and c["min_cosine"] == 0.95 and c["min_drop"] == 0.02
    assert r["n_used"] == 3 and r["series"].shape == (3,)
    s.get_reconstruction(end_iter=8, n_samples=5, idx=None)
    assert _RecEngine.calls[-1]["used"] is None
    with pytest.raises(ValueError, match="not all recorded"):
        s.get_reconstruction(end_iter=12, n_samples=3)
    with pytest.raises(ValueError, match="idx must lie in"):
        s.get_reconstruction(end_iter=8, n_samples=3, idx=[2])
    with pytest.raises(ValueError, match="Parameter `idx` must be"):
        s.get_reconstruction(idx="all")
    s.close()
    t = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "one"), engine_factory=_NoWaicEngine)
    with pytest.raises(ValueError, match="get_reconstruction needs an engine"):
        t.get_reconstruction()
    t.close()


def test_new_symbols_declared_exported_and_bound():
    import ctypes as C
    from bayesnmf_amd import engine
    hdr = open(os.path.join(ROOT, "include", "bnmf.h")).read()
    assert re.search(r"#define BNMF_REC_NTUM\s+6\b", hdr) and re.search(r"#define BNMF_REC_NDROP\s+4\b", hdr) and re.search(r"#define BNMF_REC_NSIG\s+3\b", hdr)
    assert re.search(r"#define BNMF_VERSION 100\b", hdr) and "NOT refitted" in hdr and "upper bound" in hdr
    for sym in ("bnmf_reconstruction", "bnmf_reconstruction_at"):
        assert re.search(r"\bint\s+%s\s*\(\s*bnmf_handle\s*\*" % sym, hdr), f"{sym} not declared in include/bnmf.h"
        assert sym in engine.ABI_SYMBOLS
    so = os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    L = engine.lib()
    for sym, nargs in (("bnmf_reconstruction", 10), ("bnmf_reconstruction_at", 11)):
        assert re.search(r"\bT %s$" % sym, exported, re.M), f"{sym} not exported by libbnmf.so"
        assert len(getattr(L, sym).argtypes) == nargs
    assert C.sizeof(engine.BnmfReconstructionInfo) == 56
    assert hasattr(engine.Engine, "reconstruction") and hasattr(engine.Engine, "reconstruction_at")
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 23." in design and "not refitted" in design.lower()
