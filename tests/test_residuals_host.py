"""bnmf_residuals without a device: the numpy restatement of the spec (tests/residuals_ref.py) held to its own conventions bit for bit
(the symmetry of every C_s, include as the cohort cut down, flat samples, the sign and the tie rules), the library's host finish
(csrc/reduce_host.h) under the sanitizers against it, the declarations and bindings, get_residuals over a stub engine, and what the
numbers mean on chains of the CPU oracle: with data from three signatures, a rank-2 fit leaves a larger share on the leading component
than a rank-3 fit does, and the rank-2 candidate looks like the signature that was left out."""
import os
import re
import subprocess

import numpy as np
import pytest

import residuals_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(_bits(np.nan_to_num(x)), _bits(np.nan_to_num(y)))


def _samples(S, K, G, N, seed):
    rng = np.random.default_rng(seed)
    P = rng.dirichlet(0.3 * np.ones(K), size=(S, N)).transpose(0, 2, 1)
    E = rng.gamma(1.0, 30.0, size=(S, N, G))
    A = np.ones((S, N))
    A[S // 2, N - 1] = 0.0
    M = rng.poisson(np.einsum("kn,ng->kg", P[0], E[0])).astype(np.int32)
    return P, E, A, M


OUT = ("gram", "type", "component", "tumour", "series")
INFO = ("n_used", "n_flat", "n_included", "n_left_out", "n_steps", "n_biased", "n_overdispersed", "worst_type_at", "min_agreement_at", "lambda", "share", "move",
        "mean_share", "min_agreement", "worst_type", "max_dispersion")


def test_every_sample_matrix_is_bitwise_symmetric_and_include_is_the_cohort_cut_down():
    P, E, A, M = _samples(4, 7, 1100, 3, 1)
    inc = np.ones(1100, dtype=np.int32)
    inc[[0, 3, 500, 1023, 1024, 1099]] = 0
    full = R.residuals_reference(P, E, A, M, include=inc, n_steps=7)
    for C in list(full["C"]) + [full["gram"]]:
        assert np.array_equal(_bits(C), _bits(C.T))
    keep = np.where(inc == 1)[0]
    cut = R.residuals_reference(P, E[:, :, keep], A, M[:, keep], n_steps=7)
    for k in ("gram", "type", "component", "series", "C", "b", "v", "t", "chi"):
        assert _same_bits(full[k], cut[k]), k
    assert _same_bits(full["tumour"][:, keep], cut["tumour"]) and np.isnan(full["tumour"][:, inc == 0]).all()
    assert all(_same_bits(full[k], cut[k]) for k in INFO if k not in ("n_left_out",)) and full["n_left_out"] == 6 and full["n_included"] == 1094
    # q is the diagonal, tr its sum in order, chi and b as a plain sum would give them
    s = 2
    assert _same_bits(full["series"][0, s], sum(float(x) for x in np.diag(full["C"][s])))
    z, chi = R.residuals_z(P[s], E[s], A[s], M.astype(float), keep)
    assert np.allclose(chi, (z * z).sum(axis=0) / 7, rtol=1e-13) and np.allclose(full["C"][s], z @ z.T / len(keep), rtol=1e-11, atol=1e-13)
    assert np.allclose(full["b"][s], z.mean(axis=1), rtol=1e-10, atol=1e-13)


def test_flat_samples_are_left_out_and_counted():
    P, E, A, M = _samples(5, 6, 40, 2, 2)
    M = M.astype(np.float64)
    # a sample whose fit is the data in every cell: z = 0 throughout, trace 0, flat
    Pz, Ez = P.copy(), E.copy()
    Mz = np.einsum("kn,ng->kg", Pz[1], Ez[1])
    sig = np.ones((5, 40))
    ref = R.residuals_reference(Pz, Ez, A, Mz, sigmasq=sig, n_steps=5)
    assert ref["flat"].tolist() == [False, True, False, False, False] and ref["n_flat"] == 1 and ref["n_used"] == 5
    assert np.isnan(ref["series"][:, 1]).all() and not np.isnan(ref["series"][:, [0, 2, 3, 4]]).any() and ref["min_agreement_at"] != 1
    rest = R.residuals_reference(Pz[[0, 2, 3, 4]], Ez[[0, 2, 3, 4]], A[[0, 2, 3, 4]], Mz, sigmasq=sig[[0, 2, 3, 4]], n_steps=5)
    for k in ("gram", "type", "component", "tumour"):
        assert _same_bits(ref[k], rest[k]), k
    assert _same_bits(ref["series"][:, [0, 2, 3, 4]], rest["series"])
    # an infinite trace is flat too; fewer than 2 samples that are not flat: refused
    C = np.eye(3)
    assert R.lead(np.where(C > 0, np.inf, 0.0), 3)["flat"] and R.lead(np.zeros((3, 3)), 3)["flat"] and R.lead(-C, 3)["flat"] and not R.lead(C, 3)["flat"]
    big = np.full((2, 2), 1e200)                                                                     # the trace is finite, nn is not
    assert R.lead(big, 3)["flat"]
    with pytest.raises(R.Refused) as e:
        R.residuals_reference(Pz[[1, 1, 0]], Ez[[1, 1, 0]], A[[1, 1, 0]], Mz, sigmasq=sig[:3], n_steps=5)
    assert e.value.code == -2


def test_sign_and_tie_rules_of_the_component():
    # the start is the column of the largest diagonal element, the first among equals
    C = np.array([[2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 1.0]])
    ld = R.lead(C, 1)
    assert ld["v"].tolist() == [1.0, 0.0, 0.0] and ld["lam"] == 2.0 and ld["share"] == 0.4 and ld["move"] == 0.0
    assert R.lead(C[::-1, ::-1].copy(), 1)["v"].tolist() == [0.0, 1.0, 0.0]
    # the element of largest magnitude is made positive, the first among equals
    C = np.array([[1.0, -1.0], [-1.0, 1.0]])
    ld = R.lead(C, 4)
    assert ld["v"][0] > 0 and ld["v"][1] < 0 and abs(ld["v"][0]) == abs(ld["v"][1]) and abs(ld["lam"] - 2.0) < 1e-15
    C = np.array([[1.0, -2.0], [-2.0, 5.0]])                                                         # the start column [-2, 5] / . : already positive at 1
    ld = R.lead(C, 50)
    w, U = np.linalg.eigh(C)
    assert ld["v"][1] > 0 and ld["v"][0] < 0 and abs(ld["lam"] - w[-1]) < 1e-12 and ld["move"] < 1e-12 and np.allclose(np.abs(ld["v"]), np.abs(U[:, -1]))
    # move says how far one more step would go: large after one step of a slow matrix, small after many
    C = np.diag([1.0, 0.99, 0.5]) + 0.01
    assert R.lead(C, 1)["move"] > R.lead(C, 200)["move"] and R.lead(C, 2000)["move"] < 1e-9
    # alignment: a sample whose component points the other way enters the component rows flipped
    P, E, A, M = _samples(3, 5, 30, 2, 3)
    ref = R.residuals_reference(P, E, A, M, n_steps=30)
    sgn = np.where(ref["series"][4] < 0, -1.0, 1.0)
    assert _same_bits(ref["component"][3], ((ref["v"] * sgn[:, None]) > 0).sum(axis=0) / 3.0)
    assert ref["min_agreement"] == np.abs(ref["series"][4]).min() and ref["min_agreement_at"] == int(np.abs(ref["series"][4]).argmin())
    # the counts of the info fields
    assert ref["n_overdispersed"] == int((ref["type"][3] > 2.0).sum()) and ref["worst_type_at"] == int(ref["type"][3].argmax())
    assert ref["n_biased"] == int(((ref["type"][2] <= 0.025) | (ref["type"][2] >= 0.975)).sum())
    for bad in (dict(n_steps=0), dict(n_steps=10001), dict(max_dispersion=float("nan")), dict(max_dispersion=-1.0), dict(include=np.full(30, 2))):
        with pytest.raises(R.Refused) as e:
            R.residuals_reference(P, E, A, M, **bad)
        assert e.value.code == -1
    for bad in (dict(include=np.eye(30, dtype=int)[0]),):
        with pytest.raises(R.Refused) as e:
            R.residuals_reference(P, E, A, M, **bad)
        assert e.value.code == -2
    with pytest.raises(R.Refused):
        R.residuals_reference(P[:1], E[:1], A[:1], M)


def test_finish_under_the_sanitizers_is_the_restatement(tmp_path):
    """csrc/reduce_host.h's residuals_lead and residuals_finish (the library's own code), built as a stand-alone program with
    -fsanitize=address,undefined: a clean run, and every output and info field the restatement's bit for bit, on made-up residuals:
    tumours left out at both ends, a flat sample (all-zero residuals) in the middle and at the end, K = 1, more than 64 samples"""
    exe = str(tmp_path / "residuals_reduce_check")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tools", "residuals_reduce_check.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", p.stderr
    rng = np.random.default_rng(5)
    for K, G, S, steps, flat, left in ((6, 70, 5, 8, [2], [0, 33, 69]), (1, 9, 3, 1, [], []), (4, 40, 70, 3, [0, 69], [5]), (3, 2, 2, 2, [], [])):
        members = np.array([g for g in range(G) if g not in left], dtype=np.int32)
        m = len(members)
        z = rng.normal(0.0, 1.0, size=(S, K, m)) + rng.normal(0.0, 1.0, size=(S, 1, m)) * np.linspace(-1, 1, K)[None, :, None]
        z[flat] = 0.0
        Cs, bs, leads, ts, chis = np.empty((S, K, K)), np.empty((S, K)), [], np.empty((S, m)), np.empty((S, m))
        for s in range(S):
            Cs[s], bs[s] = R.second_moments(z[s])
            leads.append(R.lead(Cs[s], steps))
            with np.errstate(invalid="ignore"):
                ts[s] = R.scores(leads[s]["v"], z[s])
            c = np.zeros(m)
            for k in range(K):
                c = c + z[s, k] * z[s, k]
            chis[s] = c / float(K)
        ref = R.finish(G, members, steps, 1.5, Cs, bs, leads, ts, chis)
        blob = np.array([m, G, K, S, steps], dtype=np.int64).tobytes() + np.array([1.5]).tobytes() + members.tobytes() + Cs.tobytes() + bs.tobytes() + z.tobytes()
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(blob)
        run = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert run.returncode == 0 and run.stderr == "", run.stderr
        out = np.fromfile(dst, dtype=np.float64)
        fl, gram, typ, comp, tum, ser, info = np.split(out, np.cumsum([S, K * K, 5 * K, 4 * K, 3 * G, 5 * S]))
        assert fl.tolist() == [1.0 if s in flat else 0.0 for s in range(S)] and ref["n_flat"] == len(flat)
        assert _same_bits(gram.reshape(K, K), ref["gram"]) and _same_bits(typ.reshape(5, K), ref["type"]) and _same_bits(comp.reshape(4, K), ref["component"])
        assert _same_bits(tum.reshape(3, G), ref["tumour"]) and _same_bits(ser.reshape(5, S), ref["series"])
        names = ("n_flat", "n_included", "n_left_out", "n_biased", "n_overdispersed", "worst_type_at", "min_agreement_at", "lambda", "share", "move", "mean_share",
                 "min_agreement", "worst_type")
        assert _same_bits(info, np.array([float(ref[n]) for n in names])), dict(zip(names, info))


def _oracle_samples(oracle_lib, M, N, seed, burn, S):
    from bayesnmf_amd.setup import apply_hyperprior_params
    o = oracle_lib.Oracle(M, N, prior="gamma", seed=seed, nthreads=4)
    apply_hyperprior_params(o, "gamma", M, N)
    o.init()
    o.run(burn)
    P, E = [], []
    for _ in range(S):
        o.run(1)
        P.append(o.get("P").copy()); E.append(o.get("E").copy())
    return np.stack(P), np.stack(E), np.ones((S, N))


def test_a_rank_too_low_shows_as_a_shared_direction(oracle_lib):
    """data from three signatures (synth_counts); chains of the CPU oracle at rank 2 and at rank 3.  No absolute threshold: the rank-2
    fit's mean share is the larger one, and its candidate is nearer the true signature that neither fitted column stands for than
    either fitted column is"""
    from bayesnmf_amd.sampler import residual_candidate
    from bayesnmf_amd.setup import synth_counts
    M, Ptrue, _ = synth_counts(24, 60, 3, 5, mean_total=8000)
    r = {}
    for N in (2, 3):
        P, E, A = _oracle_samples(oracle_lib, M, N, 3, 150, 6)
        r[N] = R.residuals_reference(P, E, A, M, n_steps=100)
        r[N]["Pm"] = np.mean(P / P.sum(axis=1, keepdims=True), axis=0)
    print(f"mean share rank 2 {r[2]['mean_share']!r} rank 3 {r[3]['mean_share']!r}; dispersion rank 2 {r[2]['type'][3].mean()!r} rank 3 {r[3]['type'][3].mean()!r}")
    assert r[2]["mean_share"] > r[3]["mean_share"]
    cos = lambda a, b: float(a @ b / np.sqrt((a @ a) * (b @ b)))  # noqa: E731
    # the true signature that the rank-2 fit leaves out: the one its two columns match worst
    fit = r[2]["Pm"]
    left = int(np.argmin([max(cos(Ptrue[:, j], fit[:, n]) for n in range(2)) for j in range(3)]))
    cand = residual_candidate(r[2]["component"][0])
    assert abs(cand.sum() - 1.0) < 1e-12 and (cand >= 0).all()
    c_left = cos(cand, Ptrue[:, left])
    print(f"left-out signature {left}: candidate cosine {c_left!r}, fitted columns {[cos(fit[:, n], Ptrue[:, left]) for n in range(2)]!r}; "
          f"candidate with the fitted columns {[cos(cand, fit[:, n]) for n in range(2)]!r}")
    assert all(c_left > cos(cand, fit[:, n]) for n in range(2))


def test_get_residuals_ranges_idx_names_and_frames(tmp_path):
    """bayesNMF_sampler.get_residuals over a stub engine: the range and idx rules of get_WAIC (_recorded_range), include as the sampler
    passes it on, the candidate and its cosines, the frames with the data's column names"""
    pd = pytest.importorskip("pandas")
    from test_waic_host import _NoWaicEngine
    from bayesnmf_amd.sampler import bayesNMF_sampler, residual_candidate
    from bayesnmf_amd.convergence import new_convergence_control
    from bayesnmf_amd.setup import synth_counts

    class _ResEngine(_NoWaicEngine):
        calls = []

        def window(self, name, back):
            rng = np.random.default_rng(7)
            shp = dict(P=(self.K, self.N), E=(self.N, self.G), A=(1, self.N))[name]
            return [rng.gamma(1.0, 1.0, size=shp) if name != "A" else np.ones(shp) for _ in range(back)]

        def residuals(self, last_n, include=None, n_steps=100, max_dispersion=2.0, used=None, end_iter=None):
            type(self).calls.append(dict(last_n=last_n, include=include, n_steps=n_steps, max_dispersion=max_dispersion,
                                         used=None if used is None else np.array(used), end_iter=end_iter))
            S, G, K = last_n if used is None else int(np.sum(used)), self.G, self.K
            vbar = np.linspace(-1.0, 2.0, K)
            out = dict(n_used=S, n_flat=0, n_included=G, n_left_out=0, n_steps=n_steps, n_biased=1, n_overdispersed=2, worst_type_at=3, min_agreement_at=0,
                       share=0.5, move=1e-9, mean_share=0.4, min_agreement=0.9, worst_type=3.5, max_dispersion=max_dispersion, gram=np.eye(K),
                       type=np.full((5, K), 4.0), component=np.stack([vbar, vbar, np.full(K, 9.0), np.ones(K)]), tumour=np.arange(3.0 * G).reshape(3, G),
                       series=np.zeros((5, S)))
            out["lambda"] = 2.0
            return out

    M, _, _ = synth_counts(12, 9, 2, 3, mean_total=200)
    names = [f"PD{g:03d}" for g in range(9)]
    cc = new_convergence_control()
    cc.update(MAP_over=4, MAP_every=2, maxiters=10, miniters=2)
    s = bayesNMF_sampler(pd.DataFrame(M, columns=names), 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "r"), engine_factory=_ResEngine,
                         convergence_control=cc, save_all_samples=True, periodic_save=False)
    s.run_gibbs_sampler()
    r = s.get_residuals()
    c = _ResEngine.calls[-1]
    assert c["last_n"] == 4 and c["end_iter"] is None and c["n_steps"] == 100 and c["max_dispersion"] == 2.0 and c["include"] is None
    assert np.array_equal(c["used"], [1, 1, 1, 1])
    vbar = np.linspace(-1.0, 2.0, 12)
    cand = np.maximum(vbar, 0.0) / np.maximum(vbar, 0.0).sum()
    assert np.array_equal(r["candidate"], cand) and np.array_equal(residual_candidate(-vbar), cand) and np.isnan(residual_candidate(np.full(3, np.nan))).all()
    assert np.isnan(residual_candidate(np.zeros(4))).all() and residual_candidate([-3.0, 1.0, -1.0]).tolist() == [0.75, 0.0, 0.25]
    assert r["candidate_cosine"].shape == (3,) and ((r["candidate_cosine"] > 0) & (r["candidate_cosine"] <= 1)).all() and "reference_cosine" not in r
    t = r["types"]
    assert list(t.columns) == ["type", "bias", "bias_sd", "p_positive", "dispersion", "dispersion_sd", "component", "component_mean", "component_sd"]
    assert t.iloc[2].tolist() == [2, 4.0, 2.0, 4.0, 4.0, 2.0, vbar[2], vbar[2], 3.0]
    u = r["tumours"]
    assert list(u.columns) == ["tumour", "score", "score_sd", "chi", "included"] and u["tumour"].tolist() == names and u["included"].all()
    assert np.array_equal(u["score"], r["tumour"][0]) and np.array_equal(u["chi"], r["tumour"][2]) and r["n_overdispersed"] == 2 and r["lambda"] == 2.0
    inc = [1, 1, None, 1, 0, 1, float("nan"), 1, 1]
    ref = pd.DataFrame(np.stack([cand, np.ones(12), np.arange(12.0)], axis=1), columns=["SBS1", "SBS5", "SBS40"])
    r = s.get_residuals(include=inc, n_steps=7, max_dispersion=3.0, reference_P=ref, end_iter=8, n_samples=5, idx=[4, 6, 8])
    c = _ResEngine.calls[-1]
    assert c["end_iter"] == 8 and c["last_n"] == 5 and np.array_equal(c["used"], [1, 0, 1, 0, 1]) and c["n_steps"] == 7 and c["max_dispersion"] == 3.0
    assert np.array_equal(c["include"], [1, 1, 0, 1, 0, 1, 0, 1, 1]) and r["tumours"]["included"].tolist() == [bool(v) for v in c["include"]]
    assert r["best_reference"] == "SBS1" and abs(r["best_reference_cosine"] - 1.0) < 1e-15 and r["reference_cosine"].shape == (3,)
    s.get_residuals(end_iter=8, n_samples=5, idx=None)
    assert _ResEngine.calls[-1]["used"] is None
    with pytest.raises(ValueError, match="include has 3 values"):
        s.get_residuals(include=[1, 1, 1])
    with pytest.raises(ValueError, match="reference_P is"):
        s.get_residuals(reference_P=np.ones((5, 2)))
    with pytest.raises(ValueError, match="not all recorded"):
        s.get_residuals(end_iter=12, n_samples=3)
    s.close()
    t = bayesNMF_sampler(M, 3, likelihood="poisson", prior="gamma", output_dir=str(tmp_path / "one"), engine_factory=_NoWaicEngine)
    with pytest.raises(ValueError, match="get_residuals needs an engine"):
        t.get_residuals()
    t.close()


def test_new_symbols_declared_exported_bound_and_refused_without_a_device():
    import ctypes as C
    from bayesnmf_amd import engine
    hdr = open(os.path.join(ROOT, "include", "bnmf.h")).read()
    for name, val in (("BNMF_RES_NTYPE", 5), ("BNMF_RES_NCOMP", 4), ("BNMF_RES_NTUM", 3), ("BNMF_RES_NSER", 5), ("BNMF_RES_MAX_K", 2048), ("BNMF_RES_MAX_STEPS", 10000)):
        assert re.search(r"#define %s\s+%d\b" % (name, val), hdr), name
    assert re.search(r"#define BNMF_VERSION 100\b", hdr) and "a reporting convention" in hdr
    for sym in ("bnmf_residuals", "bnmf_residuals_at"):
        assert re.search(r"\bint\s+%s\s*\(\s*bnmf_handle\s*\*" % sym, hdr), f"{sym} not declared in include/bnmf.h"
        assert sym in engine.ABI_SYMBOLS
    so = os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    L = engine.lib()
    for sym, nargs in (("bnmf_residuals", 12), ("bnmf_residuals_at", 13)):
        assert re.search(r"\bT %s$" % sym, exported, re.M), f"{sym} not exported by libbnmf.so"
        assert len(getattr(L, sym).argtypes) == nargs
    assert C.sizeof(engine.BnmfResidualsInfo) == 96 and R.MAX_K == 2048 and R.MAX_STEPS == 10000
    assert engine.RES_TYPE_ROWS == ("bias", "bias_var", "p_positive", "dispersion", "dispersion_var") and engine.RES_TUMOUR_ROWS == ("score", "score_var", "chi")
    assert engine.RES_COMPONENT_ROWS == ("vbar", "mean", "var", "p_positive") and engine.RES_SERIES_ROWS == ("trace", "lambda", "share", "move", "agreement")
    assert hasattr(engine.Engine, "residuals") and hasattr(engine.Engine, "residuals_at")
    shim = open(os.path.join(ROOT, "r", "bnmf_shim.c")).read()
    for sym in ("C_bnmf_residuals", "C_bnmf_residuals_at"):
        assert re.search(r'\{"%s", \(DL_FUNC\)&%s, \d\}' % (sym, sym), shim), sym
    # what is refused before the handle is looked at needs no device: a null handle, a null info
    info = engine.BnmfResidualsInfo()
    rest = (None, None, 5, 2.0, None, None, None, None, None)
    assert L.bnmf_residuals(None, 4, *rest, C.byref(info)) == -1 and b"null" in L.bnmf_last_error()
    assert L.bnmf_residuals_at(None, 9, 4, *rest, None) == -1 and b"bnmf_residuals_at" in L.bnmf_last_error()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 26." in design and "bnmf_residuals" in design
