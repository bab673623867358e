"""bnmf_prune's numerical spec on the host: the numpy restatement (tests/prune_ref.py) on hand-built samples, the library's
host finish (csrc/reduce_host.h's prune_finish) as a stand-alone program under the sanitizers against it bit for bit, and the new symbols
in the header, the library, the ctypes binding and the R shim.  No device."""
import os
import re
import subprocess

import numpy as np
import pytest

import prune_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(_bits(x)[~np.isnan(x)], _bits(y)[~np.isnan(y)])


def _signatures(K, N, seed=2):
    """N well-separated signatures: each has its own block of mutation types and a little of every other"""
    rng = np.random.default_rng(seed)
    P = 0.002 * rng.random((K, N))
    for n in range(N):
        P[n * (K // N):(n + 1) * (K // N), n] += rng.dirichlet(np.ones(K // N))
    return P


def _planted(S=3, K=20, N=5, G=6, seed=5):
    """samples around one truth: every tumour is made of exactly signatures 1 and 3, the other three hold small exposures"""
    rng = np.random.default_rng(seed)
    P0 = _signatures(K, N)
    P0 = P0 / P0.sum(axis=0)
    Et = np.zeros((N, G))
    Et[1], Et[3] = rng.uniform(400, 900, G), rng.uniform(300, 700, G)
    M = np.rint(P0 @ Et).astype(np.int32)
    P = np.stack([P0 * rng.uniform(0.5, 2.0, N)[None, :] for _ in range(S)])       # another scale per sample: the renormalisation undoes it
    E = np.stack([(Et + rng.uniform(2.0, 6.0, (N, G))) / (P[s].sum(axis=0))[:, None] for s in range(S)])
    return P, E, np.ones((S, N)), M


def test_a_tumour_made_of_two_of_five_signatures_keeps_exactly_those_two():
    P, E, A, M = _planted()
    r = R.prune_reference(P, E, A, M, n_steps=20, max_loss=0.01)
    kept = r["exposures"] > 0
    assert (kept[:, [1, 3], :]).all() and not kept[:, [0, 2, 4], :].any()
    assert (r["tumour"][2] == 2).all() and (r["tumour"][3] == 2).all() and (r["tumour"][4] == 2).all() and r["n_single"] == 0
    assert (r["load"][3][[1, 3]] == 1).all() and (r["load"][3][[0, 2, 4]] == 0).all() and r["signature"][0].tolist() == [0, 6, 0, 6, 0]
    gone = r["exposures"][:, [0, 2, 4], :]
    assert (gone == 0).all() and not np.signbit(gone).any()                         # removed factors are exactly +0.0
    assert (r["s_cos_f"] >= r["s_cos_0"] - 0.01).all() and (r["s_n_kept"] >= 1).all()
    assert np.allclose(r["load"][0][[1, 3]].sum(axis=0), M.sum(axis=0), rtol=0.02)  # the two that stay carry the tumour
    assert r["trials"] == int(r["s_trials"].sum()) and r["max_change"] == r["tumour"][5].max()
    # a permutation of the tumours permutes the outputs bitwise
    perm = np.array([4, 0, 5, 2, 1, 3])
    q = R.prune_reference(P, E[:, :, perm], A, M[:, perm], n_steps=20, max_loss=0.01)
    assert _same_bits(q["load"], r["load"][:, :, perm]) and _same_bits(q["tumour"], r["tumour"][:, perm]) and _same_bits(q["exposures"], r["exposures"][:, :, perm])
    assert q["trials"] == r["trials"] and _same_bits(q["signature"][0], r["signature"][0])


def test_nothing_is_removed_below_any_cosine_and_everything_but_one_above():
    P, E, A, M = _planted(S=2, G=4)
    A[1, 4] = 0.0                                                                   # the second sample excludes a factor: N_in = 4
    r = R.prune_reference(P, E, A, M, n_steps=5, max_loss=-2.0)
    assert r["n_in"].tolist() == [5, 4] and (r["s_trials"] == r["n_in"][:, None]).all() and (r["s_n_kept"] == r["n_in"][:, None]).all()
    assert (r["exposures"][1, 4] == 0).all() and not np.signbit(r["exposures"][1, 4]).any() and (r["s_cos_f"] == r["s_cos_0"]).all()
    r = R.prune_reference(P, E, A, M, n_steps=5, max_loss=2.0)
    assert (r["s_n_kept"] == 1).all() and (r["s_trials"] == r["n_in"][:, None] - 1).all() and r["n_single"] == 4
    assert ((r["exposures"] > 0).sum(axis=1) == 1).all()


def test_equal_exposures_the_lower_place_goes_first_and_a_column_of_P_that_sums_to_zero_takes_no_part():
    K, N = 12, 4
    P0 = _signatures(K, N, seed=3)
    x = P0 / P0.sum(axis=0)
    x[:, 2] = x[:, 1]                                                               # two identical columns with equal starts: equal e after any step
    mv = np.rint(x @ np.array([300.0, 50.0, 50.0, 300.0]))
    order = []
    r = R.prune_problem(x, mv, np.array([90.0, 7.0, 7.0, 90.0]), 3, -2.0, order=order)   # one round, every candidate fails: the order of the trials
    assert r["e"][1] == r["e"][2] and r["n_kept"] == 4 and sorted(order) == [0, 1, 2, 3]
    assert order.index(2) == order.index(1) + 1                                     # the tie: the lower place first, the other right behind it
    assert [float(r["e"][i]) for i in order] == sorted(float(v) for v in r["e"])    # e ascending
    P = P0[None].copy()
    P[0, :, 2] = 0.0                                                                # cs == 0: the factor takes no part
    E = np.full((1, N, 3), 40.0)
    r = R.prune_reference(P, E, np.ones((1, N)), np.rint(x[:, [0, 1, 3]] @ np.full((3, 3), 100.0)).astype(np.int32), n_steps=3, max_loss=-2.0)
    assert r["n_in"].tolist() == [3] and (r["exposures"][0, 2] == 0).all() and not np.isnan(r["exposures"]).any() and (r["s_trials"] == 3).all()


def test_an_all_zero_tumour_is_nan_and_counted_and_one_factor_needs_no_trial():
    P, E, A, M = _planted(S=2, G=4)
    M = M.copy()
    M[:, 2] = 0
    inc = np.array([1, 1, 1, 0])
    r = R.prune_reference(P, E, A, M, n_steps=4, max_loss=0.01, include=inc)
    assert r["n_included"] == 3 and r["n_undefined"] == 1 and np.isnan(r["tumour"][:, [2, 3]]).all() and np.isnan(r["load"][:, :, [2, 3]]).all()
    assert np.isnan(r["exposures"][:, :, [2, 3]]).all() and not np.isnan(r["tumour"][:, [0, 1]]).any() and not np.isnan(r["series"]).any()
    assert (r["s_trials"][:, 2] == 0).all() and np.isnan(r["s_cos_0"][:, 2]).all()
    one = R.prune_reference(P[:, :, :1], E[:, :1], A[:, :1], M, n_steps=4, max_loss=0.01)
    assert one["trials"] == 0 and (one["tumour"][2][[0, 1, 3]] == 1).all() and one["n_single"] == 3
    none = R.prune_reference(P, E[:, :, :2], np.zeros_like(A), M[:, :2], n_steps=4)           # N_in = 0: the fit is nothing, its cosine +0.0
    assert (none["s_n_kept"] == 0).all() and (none["s_cos_0"] == 0).all() and (none["exposures"] == 0).all()


def test_finish_under_the_sanitizers_is_the_restatement(tmp_path):
    """csrc/reduce_host.h's prune_finish (the library's own code), built as a stand-alone program with -fsanitize=address,undefined: a clean
    run, and every output and info field the restatement's bit for bit, from the rows in member order as the device leaves them (taken
    here from the restatement): tumours left out at both ends, an undefined one, N = 1, one sample, more than 64 members"""
    exe = str(tmp_path / "prune_reduce_check")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tools", "prune_reduce_check.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", p.stderr
    for S, G, N, left, zero in ((3, 9, 5, [0, 8], [4]), (1, 3, 1, [], []), (2, 70, 3, [5], [6, 69]), (2, 4, 5, [1], [0, 2, 3])):
        rng = np.random.default_rng(S + G)
        K = 10
        P = rng.gamma(0.5, 1.0, size=(S, K, N))
        E = rng.gamma(1.0, 50.0, size=(S, N, G))
        M = rng.poisson(np.einsum("kn,ng->kg", P[0], E[0])).astype(np.int32)
        M[:, zero] = 0
        inc = np.ones(G, dtype=np.int32)
        inc[left] = 0
        ref = R.prune_reference(P, E, np.ones((S, N)), M, n_steps=2, max_loss=0.05, include=inc)
        members = np.where(inc == 1)[0].astype(np.int32)
        m = len(members)
        Md = M.astype(np.float64)
        mm = np.zeros(G)
        for k in range(K):
            mm = mm + Md[k] * Md[k]
        df = mm[members] > 0
        z = lambda a: np.where(np.isnan(a), 0.0, a)  # noqa: E731
        ld = np.ascontiguousarray(ref["load"][:, :, members].transpose(0, 2, 1)).reshape(4, N * m)      # n + N j
        tum = np.ascontiguousarray(ref["tumour"][:, members])
        tr = z(ref["s_trials"][:, members]).sum(axis=0)
        ser = np.stack([np.array([R.canon(np.where(df, z(ref[key][s, members]), 0.0), 1024) for s in range(S)]) for key in ("s_n_kept", "s_cos_f")])
        blob = (np.array([m, G, N, S], dtype=np.int64).tobytes() + members.tobytes() + mm[members].tobytes() + ld.tobytes() + tum.tobytes() + tr.tobytes() + ser.tobytes())
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(blob)
        done = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert done.returncode == 0 and done.stderr == "", done.stderr
        out = np.fromfile(dst, dtype=np.float64)
        lo, tu, se, sg, info = np.split(out, np.cumsum([4 * N * G, 7 * G, 2 * S, 3 * N]))
        assert _same_bits(lo.reshape(4, G, N).transpose(0, 2, 1), ref["load"]) and _same_bits(tu.reshape(7, G), ref["tumour"])
        assert _same_bits(se.reshape(2, S), ref["series"]) and _same_bits(sg.reshape(3, N), ref["signature"])
        names = ("n_included", "n_undefined", "n_single", "trials", "max_change")
        assert _same_bits(info, np.array([float(ref[n]) for n in names])), dict(zip(names, info))


def test_get_sparse_assignment_ranges_idx_names_and_frames(tmp_path):
    """bayesNMF_sampler.get_sparse_assignment over a stub engine: the range and idx rules of get_WAIC (_recorded_range), include as the
    sampler passes it on, the table of the kept pairs with the data's names, the ValueErrors"""
    pd = pytest.importorskip("pandas")
    from test_waic_host import _NoWaicEngine
    from bayesnmf_amd.sampler import bayesNMF_sampler
    from bayesnmf_amd.convergence import new_convergence_control
    from bayesnmf_amd.setup import synth_counts

    class _PrnEngine(_NoWaicEngine):
        calls = []

        def prune(self, last_n, include=None, n_steps=20, max_loss=0.01, used=None, end_iter=None, exposures=False):
            type(self).calls.append(dict(last_n=last_n, include=include, n_steps=n_steps, max_loss=max_loss, used=None if used is None else np.array(used),
                                         end_iter=end_iter, exposures=exposures))
            S, G, N = last_n if used is None else int(np.sum(used)), self.G, self.N
            load = np.zeros((4, N, G))
            load[0] = np.arange(N * G, dtype=np.float64).reshape(N, G)
            load[3, 0, :] = 1.0
            load[3, 2, 4] = 0.5
            load[3, 1, 4] = 0.25
            return dict(n_used=S, n_included=G, n_undefined=0, n_single=G - 1, n_steps=n_steps, trials=7, max_change=1e-3, max_loss=max_loss, load=load,
                        tumour=np.arange(7.0 * G).reshape(7, G), series=np.zeros((2, S)), signature=np.zeros((3, N)))

    M, _, _ = synth_counts(12, 9, 2, 3, mean_total=200)
    names = [f"PD{g:03d}" for g in range(9)]
    cc = new_convergence_control()
    cc.update(MAP_over=4, MAP_every=2, maxiters=10, miniters=2)
    s = bayesNMF_sampler(pd.DataFrame(M, columns=names), 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "r"), engine_factory=_PrnEngine,
                         convergence_control=cc, save_all_samples=True, periodic_save=False)
    s.run_gibbs_sampler()
    r = s.get_sparse_assignment()
    c = _PrnEngine.calls[-1]
    assert c["last_n"] == 4 and c["end_iter"] is None and c["max_loss"] == 0.01 and c["n_steps"] == 20 and c["include"] is None and not c["exposures"]
    assert np.array_equal(c["used"], [1, 1, 1, 1])
    a = r["assignment"]
    assert list(a.columns) == ["tumour", "signature", "load", "p_kept"] and len(a) == 10 and a["tumour"].tolist()[:5] == names[:4] + [names[4]]
    assert a[a["tumour"] == "PD004"]["signature"].tolist() == [0, 2] and a[a["tumour"] == "PD004"]["load"].tolist() == [4.0, 22.0]
    t = r["tumours"]
    assert list(t.columns) == ["tumour", "cos_0", "cos_f", "n_kept", "n_kept_min", "n_kept_max", "rel_change", "mean_trials", "included"]
    assert t["tumour"].tolist() == names and np.array_equal(t["n_kept"], r["tumour"][2]) and t["included"].all() and r["trials"] == 7
    inc = [1, 1, None, 1, 0, 1, float("nan"), 1, 1]
    r = s.get_sparse_assignment(max_loss=0.05, n_steps=7, include=inc, end_iter=8, n_samples=5, exposures=True, idx=[4, 6, 8])
    c = _PrnEngine.calls[-1]
    assert c["end_iter"] == 8 and c["last_n"] == 5 and np.array_equal(c["used"], [1, 0, 1, 0, 1]) and c["max_loss"] == 0.05 and c["n_steps"] == 7 and c["exposures"]
    assert np.array_equal(c["include"], [1, 1, 0, 1, 0, 1, 0, 1, 1]) and r["tumours"]["included"].tolist() == [bool(v) for v in c["include"]]
    with pytest.raises(ValueError, match="include has 3 values"):
        s.get_sparse_assignment(include=[1, 1, 1])
    with pytest.raises(ValueError, match="include holds a value other than"):
        s.get_sparse_assignment(include=[2] * 9)
    with pytest.raises(ValueError, match="max_loss"):
        s.get_sparse_assignment(max_loss=float("nan"))
    with pytest.raises(ValueError, match="n_steps"):
        s.get_sparse_assignment(n_steps=0)
    with pytest.raises(ValueError, match="not all recorded"):
        s.get_sparse_assignment(end_iter=12, n_samples=3)
    s.close()
    t = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "one"), engine_factory=_NoWaicEngine)
    with pytest.raises(ValueError, match="get_sparse_assignment needs an engine"):
        t.get_sparse_assignment()
    t.close()


def test_new_symbols_declared_exported_bound_and_refused_without_a_device():
    import ctypes as C
    from bayesnmf_amd import engine
    hdr = open(os.path.join(ROOT, "include", "bnmf.h")).read()
    for name, val in (("BNMF_PRN_NLOAD", 4), ("BNMF_PRN_NTUM", 7), ("BNMF_PRN_NSER", 2), ("BNMF_PRN_NSIG", 3), ("BNMF_PRN_MAX_N", 128)):
        assert re.search(r"#define %s\s+%d\b" % (name, val), hdr), name
    assert re.search(r"#define BNMF_VERSION 100\b", hdr) and "info (sizeof = 48)" in hdr
    for sym in ("bnmf_prune", "bnmf_prune_at"):
        assert re.search(r"\bint\s+%s\s*\(\s*bnmf_handle\s*\*" % sym, hdr), f"{sym} not declared in include/bnmf.h"
        assert sym in engine.ABI_SYMBOLS
    so = os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    L = engine.lib()
    for sym, nargs in (("bnmf_prune", 12), ("bnmf_prune_at", 13)):
        assert re.search(r"\bT %s$" % sym, exported, re.M), f"{sym} not exported by libbnmf.so"
        assert len(getattr(L, sym).argtypes) == nargs
    assert C.sizeof(engine.BnmfPruneInfo) == 48
    assert engine.PRN_LOAD_ROWS == ("load_mean", "load_var", "share", "p_kept") and len(engine.PRN_TUMOUR_ROWS) == 7 and len(engine.PRN_SERIES_ROWS) == 2
    assert len(engine.PRN_SIGNATURE_ROWS) == 3 and hasattr(engine.Engine, "prune") and hasattr(engine.Engine, "prune_at")
    shim = open(os.path.join(ROOT, "r", "bnmf_shim.c")).read()
    for sym in ("C_bnmf_prune", "C_bnmf_prune_at"):
        assert re.search(r'\{"%s", \(DL_FUNC\)&%s, \d\}' % (sym, sym), shim), sym
    # what is refused before the handle is looked at needs no device: a null handle, a null info
    info = engine.BnmfPruneInfo()
    rest = (None, None, 20, 0.01, None, None, None, None, None)
    assert L.bnmf_prune(None, 4, *rest, C.byref(info)) == -1 and b"null" in L.bnmf_last_error()
    assert L.bnmf_prune_at(None, 9, 4, *rest, None) == -1 and b"bnmf_prune_at" in L.bnmf_last_error()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 28." in design and "bnmf_prune" in design
