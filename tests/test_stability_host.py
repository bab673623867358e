"""Silhouette stability of recorded signatures, the parts that need no GPU: the two new symbols; the numpy restatement of the spec
(tests/stability_ref.py) against an independent evaluation — unit columns, 1 - U U^T and plain means in extended
precision (and scikit-learn's silhouette_samples where it is installed); the conventions, the tie rules and the label renumbering
pinned exactly; the library's own finish (csrc/reduce_host.h: stability_reduce), built as a stand-alone program under the address
and undefined-behaviour sanitizers and held to the restatement bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest

import stability_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53                           # the unit roundoff of float64


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(_bits(a)[~na], _bits(b)[~nb])


def _clustered(S, K, N, seed, noise=0.15):
    """S noisy copies of N well-separated non-negative signatures: P [S][K][N], A all ones"""
    rng = np.random.default_rng(seed)
    base = rng.gamma(0.3, 1.0, size=(K, N))
    P = base[None] * rng.gamma(1.0 / noise ** 2, noise ** 2, size=(S, K, N))
    return P, np.ones((S, N))


def test_new_symbols_declared_exported_and_bound():
    import ctypes as C
    from bayesnmf_amd import engine
    hdr = open(os.path.join(ROOT, "include", "bnmf.h")).read()
    assert re.search(r"typedef struct \{ int32_t n_used, n_points, n_extra, n_left_out, n_clusters, min_stability_at (?:/\*.*?\*/)?;\s*"
                     r"int64_t n_negative; double mean_silhouette, min_stability; \} bnmf_stability_info;", hdr)
    for name, v in (("NPOINT", 4), ("NFROW", 6), ("MAX_POINTS", 65536)):
        assert re.search(r"#define BNMF_STAB_%s\s+%d\b" % (name, v), hdr), name
    so = os.path.join(ROOT, "bayesnmf_amd", "libbnmf.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    L = engine.lib()
    for sym, nargs in (("bnmf_stability", 13), ("bnmf_stability_at", 14)):
        assert re.search(r"\bint\s+%s\s*\(\s*bnmf_handle\s*\*" % sym, hdr), f"{sym} not declared in include/bnmf.h"
        assert sym in engine.ABI_SYMBOLS
        assert re.search(r"\bT %s$" % sym, exported, re.M), f"{sym} not exported by libbnmf.so"
        assert len(getattr(L, sym).argtypes) == nargs
    assert C.sizeof(engine.BnmfStabilityInfo) == 6 * 4 + 8 + 2 * 8
    assert engine.STAB_POINT_ROWS == list(R.POINT_ROWS) and engine.STAB_FACTOR_ROWS == list(R.FACTOR_ROWS) and R.MAX_POINTS == 65536
    assert hasattr(engine.Engine, "stability") and hasattr(engine.Engine, "stability_at")


@pytest.mark.parametrize("S,K,N,seed", [(9, 96, 4, 1), (14, 24, 3, 2), (6, 96, 7, 3)])
def test_restatement_agrees_with_the_matrix_product_form_inside_a_derived_bound(S, K, N, seed):
    """The independent evaluation: columns scaled to unit length, 1 - U U^T, plain means, all in extended precision, so that its own
    error (about K 2^-64) does not count.  The restatement's distance carries, for non-negative columns, the K roundings of the dot
    product, those of the two norms halved by the root, the product, the root, the division and the subtraction from 1; a cosine is at
    most 1, so the absolute error is that many units.  A worst-case count gives 2 K + 5 units; the figure held here is the tighter
    (K + 4) 2^-53 per distance, and the same for a and b, which are means of distances.  The silhouette (b - a) / mx with errors e in
    a and b moves by at most 2 e / mx + |b - a| e / mx^2 + 2^-53 <= 3 e / mx + 2^-53; the inputs keep mx >= 0.05."""
    P, A = _clustered(S, K, N, seed)
    ref = R.stability_reference(P, A)
    cols, nn, lab, _ = R.points_of(P, A)
    M = cols.shape[0]
    L = cols.astype(np.longdouble)
    Un = L / np.sqrt((L * L).sum(axis=1))[:, None]
    d = 1.0 - Un @ Un.T
    d[np.arange(M), np.arange(M)] = 0.0
    e = (K + 4) * U
    assert np.abs(R.distances(cols, nn).astype(np.longdouble) - d).max() <= e
    m = np.array([(lab == j).sum() for j in range(N)])
    mean_to = np.stack([d[:, lab == j].sum(axis=1) / m[j] for j in range(N)], axis=1)               # [M][N]
    a = np.array([d[i, lab == lab[i]].sum() / (m[lab[i]] - 1) for i in range(M)])
    other = np.where(np.arange(N)[None, :] == lab[:, None], np.inf, mean_to)
    b = other.min(axis=1)
    mx = np.maximum(a, b)
    assert float(mx.min()) >= 0.05, "the inputs do not keep max(a, b) away from 0"
    sil = (b - a) / mx
    print(f"stability: largest differences a {float(np.abs(ref['point'][1] - a).max()):.3g}, b {float(np.abs(ref['point'][2] - b).max()):.3g}, "
          f"silhouette {float(np.abs(ref['point'][0] - sil).max()):.3g}; bound {e:.3g}")
    assert np.abs(ref["point"][1] - a).max() <= e and np.abs(ref["point"][2] - b).max() <= e
    assert (np.abs(ref["point"][0] - sil) <= 3 * e / mx + U).all()
    assert np.array_equal(ref["point"][3], other.argmin(axis=1).astype(np.float64))
    for j in range(N):
        assert abs(ref["factor"][1, j] - float(sil[lab == j].mean())) <= float((3 * e / mx[lab == j]).max()) + 8 * U
        assert ref["factor"][0, j] == m[j]
    try:
        from sklearn.metrics import silhouette_samples
    except ImportError:
        return
    sk = silhouette_samples(cols, lab, metric="cosine")
    print(f"stability: largest difference from silhouette_samples {float(np.abs(ref['point'][0] - sk).max()):.3g}")
    assert (np.abs(ref["point"][0] - sk) <= 3 * e / mx + U).all()                                   # the second witness, under the same bound


def test_conventions_are_pinned_exactly():
    P, A = _clustered(6, 8, 3, 5)
    S, K, N = P.shape
    ident = np.tile(np.arange(N), (S, 1))
    # a singleton cluster: silhouette +0.0, a = +0.0, b and nearest as usual
    lab = ident.copy()
    lab[:, 2] = -1
    lab[3, 2] = 2
    r = R.stability_reference(P, A, lab)
    i = 3 * N + 2
    assert r["factor"][0].tolist() == [6, 6, 1] and _bits(r["point"][0, i]) == 0 and _bits(r["point"][1, i]) == 0 and r["point"][3, i] in (0.0, 1.0)
    assert r["n_left_out"] == 5 and np.isnan(r["point"][:3, 2]).all() and r["point"][3, 2] == -1 and r["medoid_at"][2] == i
    assert _bits(r["factor"][1, 2]) == 0 and r["between"][2, 2] == 0.0 and r["n_clusters"] == 3
    # one non-empty cluster: NaN silhouettes, b NaN, nearest -1, no stability
    r = R.stability_reference(P, A, np.zeros((S, N), dtype=np.int64))
    assert np.isnan(r["point"][0]).all() and np.isnan(r["point"][2]).all() and (r["point"][3] == -1).all() and (r["point"][1] > 0).all()
    assert np.isnan(r["mean_silhouette"]) and np.isnan(r["min_stability"]) and r["min_stability_at"] == -1 and r["n_clusters"] == 1 and r["n_negative"] == 0
    assert np.isnan(r["factor"][1:3]).all() and r["factor"][0].tolist() == [S * N, 0, 0] and np.isnan(r["between"][0, 1]) and not np.isnan(r["between"][0, 0])
    assert np.isnan(r["medoid"][:, 1:]).all() and (r["medoid_at"][1:] == -1).all() and abs(r["medoid"][:, 0].sum() - 1) < 1e-12
    # identical columns: a = +0.0 exactly (1 - x / sqrt(x x) is 1 - 1), the silhouette 1
    Pi = np.repeat(P[:1], S, axis=0)
    r = R.stability_reference(Pi, A)
    assert (_bits(r["point"][1]) == 0).all() and (r["point"][0] == 1.0).all() and (r["factor"][1] == 1.0).all() and r["mean_silhouette"] == 1.0
    assert r["medoid_at"].tolist() == [0, 1, 2], "the first member wins a tie"
    # two clusters at the same mean distance: the first wins b's tie
    Pt = Pi.copy()
    Pt[:, :, 2] = Pt[:, :, 1]
    r = R.stability_reference(Pt, A)
    assert (r["point"][3].reshape(S, N)[:, 0] == 1).all() and (r["point"][3].reshape(S, N)[:, 1] == 2).all() and (r["point"][0].reshape(S, N)[:, 1:] == 0).all()
    assert r["min_stability_at"] == 1 and r["min_stability"] == 0.0
    # an extras-only cluster, a ring point excluded by A, by a zero column and by a column that is not finite
    A2, P2 = A.copy(), P.copy()
    A2[:, 2] = 0.0
    P2[1, :, 0] = 0.0
    P2[2, 3, 1] = np.inf
    ex = np.random.default_rng(9).gamma(0.5, 1.0, size=(K, 3))
    r = R.stability_reference(P2, A2, None, ex, [2, 2, 0])
    assert r["factor"][0].tolist() == [6, 5, 2] and r["n_left_out"] == S + 2 and r["n_extra"] == 3 and r["n_points"] == 13
    assert r["point"].shape == (4, S * N + 3) and not np.isnan(r["point"][0, S * N:]).any() and r["medoid_at"][2] in (S * N, S * N + 1)
    # renumbering the labels permutes the outputs
    P3, A3 = _clustered(7, 12, 4, 6, noise=0.4)
    lab3 = np.stack([np.random.default_rng(s).permutation(4) for s in range(7)])
    lab3[2, 1] = -1
    base = R.stability_reference(P3, A3, lab3)
    pi = np.array([2, 0, 3, 1])                                                      # old label j becomes pi[j]
    ren = R.stability_reference(P3, A3, np.where(lab3 >= 0, pi[np.clip(lab3, 0, None)], -1))
    assert _same_bits(ren["point"][:3], base["point"][:3]) and _same_bits(ren["factor"][:, pi], base["factor"]) and _same_bits(ren["medoid"][:, pi], base["medoid"])
    assert _same_bits(ren["between"][np.ix_(pi, pi)], base["between"]) and np.array_equal(ren["medoid_at"][pi], base["medoid_at"])
    near = base["point"][3]
    assert np.array_equal(ren["point"][3], np.where(near >= 0, pi[np.clip(near.astype(int), 0, None)], -1).astype(np.float64))
    assert _same_bits(ren["mean_silhouette"], base["mean_silhouette"]) and _same_bits(ren["min_stability"], base["min_stability"])
    assert ren["min_stability_at"] == pi[base["min_stability_at"]] and ren["n_negative"] == base["n_negative"]
    # the refusals of the restatement
    for kw, code in ((dict(labels=np.full((S, N), 3)), -1), (dict(extra_P=ex, extra_label=[0, 1, 3]), -1), (dict(extra_P=ex * 0, extra_label=[0, 1, 2]), -1),
                     (dict(labels=np.full((S, N), -1)), -2)):
        with pytest.raises(R.Refused) as err:
            R.stability_reference(P, A, **kw)
        assert err.value.code == code


def _packed(ref, P, A, labels, extra_P, extra_label):
    """the inputs of stability_reduce for the case of ref: the members in the packed order (cluster by cluster, list order)"""
    cols, nn, lab, _ = R.points_of(P, A, labels, extra_P, extra_label)
    idx = np.where(lab >= 0)[0]
    N = P.shape[2]
    order = np.concatenate([np.where(lab[idx] == j)[0] for j in range(N)])
    off = np.concatenate([[0], np.cumsum([(lab[idx] == j).sum() for j in range(N)])]).astype(np.int32)
    return off, idx[order].astype(np.int64), np.ascontiguousarray(ref["D"][order]), np.ascontiguousarray(cols[idx][order]), cols.shape[0]


def test_finish_under_the_sanitizers_is_the_restatement(tmp_path):
    """csrc/reduce_host.h's stability_reduce and stability_medoid (the library's own code), built as a stand-alone program with
    -fsanitize=address,undefined: a clean run, and every output and info field the restatement's bit for bit"""
    exe = str(tmp_path / "stability_reduce_check")
    cmd = ["c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tools", "stability_reduce_check.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", p.stderr
    cases = []
    P, A = _clustered(11, 12, 5, 7, noise=0.5)
    lab = np.stack([np.random.default_rng(s).permutation(5) for s in range(11)])
    lab[4] = -1
    lab[:, 3] = np.where(np.arange(11) == 6, 3, -1)                                  # a label used exactly once
    cases.append((P, A, lab, None, None))
    ex = np.random.default_rng(3).gamma(0.5, 1.0, size=(12, 150))
    cases.append((P, A, None, ex, np.concatenate([np.zeros(140, dtype=np.int64), np.full(10, 4)])))     # more than two wave rounds in a cluster
    cases.append((P, A, np.zeros((11, 5), dtype=np.int64), None, None))                                   # one cluster: NaN
    A0 = A.copy()
    A0[:, 1] = 0.0
    cases.append((P, A0, None, ex[:, :4], [1, 1, 1, 2]))                                                  # an extras-only cluster
    for P, A, lab, ex, el in cases:
        ref = R.stability_reference(P, A, lab, ex, el)
        off, pt, D, cols, NPT = _packed(ref, P, A, lab, ex, el)
        M, N, K = D.shape[0], P.shape[2], P.shape[1]
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(np.array([M, N, NPT, K], dtype=np.int64).tobytes() + off.tobytes() + pt.tobytes() + D.tobytes() + cols.tobytes())
        q = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert q.returncode == 0 and q.stderr == "", q.stderr
        out = np.fromfile(dst, dtype=np.float64)
        cuts = np.cumsum([4 * NPT, 6 * N, N * N, N, N * K])
        point, factor, between, at, med, info = np.split(out, cuts)
        assert _same_bits(point.reshape(4, NPT), ref["point"]) and _same_bits(factor.reshape(6, N), ref["factor"])
        assert _same_bits(between.reshape(N, N), ref["between"]) and np.array_equal(at.astype(np.int64), ref["medoid_at"])
        assert _same_bits(med.reshape(N, K).T, ref["medoid"])
        assert [int(info[0]), int(info[1]), int(info[2]), int(info[5])] == [ref["n_points"], ref["n_clusters"], ref["n_negative"], ref["min_stability_at"]]
        assert _same_bits(info[3:5], np.array([ref["mean_silhouette"], ref["min_stability"]]))


class _StubEngine:
    """an engine that answers relabel with a perm it was given and stability from the restatement over samples it was given"""

    def __init__(self, P, A, perm):
        self.P, self.A, self.perm = P, A, perm
        self.calls = []

    def get(self, name):
        return self.P[-1]

    def relabel(self, last_n, used=None, end_iter=None, pivot_P=None, max_rounds=10, aligned=False):
        self.calls.append(("relabel", dict(last_n=last_n, used=used, end_iter=end_iter)))
        K, N = self.P.shape[1:]
        return dict(perm=self.perm, P_mean=np.zeros((K, N)), E_mean=np.zeros((N, 1)), n_used=len(self.perm))

    def stability(self, last_n, labels=None, used=None, end_iter=None, extra_P=None, extra_label=None):
        self.calls.append(("stability", dict(last_n=last_n, labels=labels, used=used, end_iter=end_iter)))
        sel = slice(None) if used is None else np.asarray(used) == 1
        return R.stability_reference(self.P[-last_n:][sel], self.A[-last_n:][sel], None if labels is None else np.asarray(labels)[sel], extra_P, extra_label)


def test_get_stability_over_a_stub_engine():
    """bayesNMF_sampler.get_stability's own glue: get_relabelling's perm (a row per USED sample) scattered into the range's rows where
    used has gaps, an unmatched sample arriving as -1 and left out, the rows of the ring points reshaped to S x N and the extras cut off"""
    from bayesnmf_amd.sampler import bayesNMF_sampler
    n, K, N, G = 7, 8, 3, 5
    P, A = _clustered(n, K, N, 21, noise=0.3)
    used = np.array([1, 0, 1, 1, 0, 1, 1], dtype=np.int32)
    S = int(used.sum())
    assert S != N
    perm = np.array([[0, 1, 2], [2, 0, 1], [-1, -1, -1], [1, 0, 2], [0, 2, 1]], dtype=np.int32)     # a row per used sample; the third is unmatched
    sm = bayesNMF_sampler.__new__(bayesNMF_sampler)
    sm._chain = _StubEngine(P, A, perm)
    sm.dims = dict(K=K, G=G, N=N)
    sm.MAP = dict(P=P[-1], keep_sigs=np.arange(N))
    sm.log = lambda *a, **k: None
    sm._recorded_range = lambda end_iter, n_samples, idx: (n, used, None, dict(end_iter=40))
    ex = np.random.default_rng(5).gamma(0.5, 1.0, size=(K, 4))
    el = np.array([2, 0, 0, 1], dtype=np.int32)
    out = sm.get_stability(extra_P=ex, extra_label=el)
    want_labels = np.full((n, N), -1, dtype=np.int32)
    want_labels[[0, 2, 3, 5, 6]] = perm
    (k0, c0), (k1, c1) = sm._chain.calls
    assert (k0, k1) == ("relabel", "stability") and c0["last_n"] == c1["last_n"] == n and c0["end_iter"] == c1["end_iter"] == 40
    assert np.array_equal(c0["used"], used) and np.array_equal(c1["used"], used)
    assert c1["labels"].dtype == np.int32 and c1["labels"].shape == (n, N) and np.array_equal(c1["labels"], want_labels)
    assert np.array_equal(out["labels"], want_labels)
    want = R.stability_reference(P[used == 1], A[used == 1], perm, ex, el)
    assert out["n_used"] == S and out["n_left_out"] == N and out["n_extra"] == 4 and out["n_points"] == (S - 1) * N + 4
    for i, name in enumerate(R.POINT_ROWS):
        assert out[name].shape == (S, N) and _same_bits(out[name], want["point"][i, :S * N].reshape(S, N)), name
    assert np.isnan(out["silhouette"][2]).all() and (out["nearest"][2] == -1).all() and not np.isnan(np.delete(out["silhouette"], 2, axis=0)).any()
    assert out["extra"].shape == (4, 4) and _same_bits(out["extra"], want["point"][:, S * N:])
    for i, name in enumerate(R.FACTOR_ROWS):
        assert out[name].shape == (N,) and _same_bits(out[name], want["factor"][i]), name
    assert out["members"].tolist() == [S - 1 + 2, S - 1 + 1, S - 1 + 1]
    assert _same_bits(out["between"], want["between"]) and _same_bits(out["medoid"], want["medoid"]) and np.array_equal(out["medoid_at"], want["medoid_at"])
    for k in ("n_clusters", "n_negative", "min_stability_at"):
        assert out[k] == want[k], k
    assert _same_bits(out["mean_silhouette"], want["mean_silhouette"]) and _same_bits(out["min_stability"], want["min_stability"])
    # relabel = False: no relabel call, labels NULL (the factor); used = None: every row of the range receives its perm row
    sm._chain.calls.clear()
    plain = sm.get_stability(relabel=False)
    assert [k for k, _ in sm._chain.calls] == ["stability"] and sm._chain.calls[0][1]["labels"] is None and plain["labels"] is None
    assert plain["n_left_out"] == 0 and plain["extra"].shape == (4, 0) and plain["silhouette"].shape == (S, N)
    full = np.stack([np.random.default_rng(s).permutation(N) for s in range(n)]).astype(np.int32)
    sm._chain = _StubEngine(P, A, full)
    sm._recorded_range = lambda end_iter, n_samples, idx: (n, None, None, {})
    every = sm.get_stability()
    assert np.array_equal(sm._chain.calls[1][1]["labels"], full) and every["n_used"] == n and every["silhouette"].shape == (n, N)
    sm._chain = object()
    with pytest.raises(ValueError, match="get_stability needs an engine"):
        sm.get_stability()
