"""The CPU oracle is the only parity checker: its own tests, the law tests and a regeneration of the committed
golden chains run ONCE against a build with AddressSanitizer + UndefinedBehaviorSanitizer (`make -C oracle asan`; CPU only — GPU
sanitizers are not available on the pool).  A finding aborts the child process (-fno-sanitize-recover, ASAN halt_on_error)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _asan_env():
    cc = os.environ.get("CC", "gcc")
    if not shutil.which(cc):
        pytest.skip("no C compiler")
    libasan = subprocess.check_output([cc, "-print-file-name=libasan.so"], text=True).strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):
        pytest.skip("libasan not installed")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "asan"])
    env = dict(os.environ)
    env.update(LD_PRELOAD=libasan, ORACLE_ASAN="1", ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", OMP_NUM_THREADS="4", PYTHONPATH=ROOT)
    return env


def test_oracle_suites_under_sanitizers():
    env = _asan_env()
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "-m", "not gpu",
                        os.path.join(ROOT, "tests", "test_oracle.py"), os.path.join(ROOT, "tests", "test_oracle_laws.py")],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in tail and "runtime error:" not in tail, tail


def test_golden_chains_regenerate_identically_under_sanitizers(tmp_path):
    """tests/golden/make_golden.py's four chains (fixed rank gamma / exponential, learned rank with tempering, Normal on real data) and shapes that
    exercise every model family once — MH, Normal likelihood, N above 64, K above 64 — on the sanitizer build: no finding, and the
    regenerated golden arrays equal the committed ones bit for bit."""
    env = _asan_env()
    code = r'''
import os, sys, numpy as np
sys.path.insert(0, %r)
import importlib.util
spec = importlib.util.spec_from_file_location("mk", os.path.join(%r, "tests", "golden", "make_golden.py"))
mk = importlib.util.module_from_spec(spec); spec.loader.exec_module(mk)
import oracle as O
assert O.lib()._name.endswith("liboracle_asan.so"), O.lib()._name
out = {"pg": mk.chain("gamma", False, 8, 6, 3, 2, 11, 7, 50), "pe": mk.chain("exponential", False, 8, 6, 3, 2, 11, 7, 50)}
temp = np.concatenate([np.zeros(3), 10.0 ** np.linspace(-6, 0, 20), np.ones(40)])
out["sbfi"] = mk.chain("gamma", True, 12, 10, 4, 2, 12, 9, 40, temp=temp)
out["nreal"] = mk.normal_golden()                  # the Normal likelihood on real data: negative, fractional and edge cells
for k, d in out.items():
    np.savez(os.path.join(%r, k + ".npz"), **d)
from bayesnmf_amd.setup import synth_counts, apply_hyperprior_params
for (K, G, N, kw, prior) in [(70, 9, 3, dict(MH=True), "truncnormal"), (20, 12, 4, dict(likelihood="normal"), "exponential"),
                             (9, 7, 70, dict(), "gamma"), (130, 5, 2, dict(learning_rank=True, rank_method="BFI"), "gamma")]:
    M, _, _ = synth_counts(K, G, 2, 5)
    o = O.Oracle(M, N, prior=prior, seed=3, save_Z=(prior == "gamma"), nthreads=3, **kw)
    apply_hyperprior_params(o, prior, M, N)
    o.init(); o.run(3); o.run(2, converged=True) if kw.get("MH") else o.run(2)
    o.close()
print("ok")
''' % (ROOT, ROOT, str(tmp_path))
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0 and "ok" in r.stdout, tail
    assert "ERROR: AddressSanitizer" not in tail and "runtime error:" not in tail, tail
    gold = os.path.join(ROOT, "tests", "golden")
    for mine, ref in (("pg", "pg_k8_g6_n3"), ("pe", "pe_k8_g6_n3"), ("sbfi", "pg_sbfi_k12_g10_n4"), ("nreal", "nt_sbfi_real_k12_g10_n3")):
        a, b = np.load(os.path.join(str(tmp_path), mine + ".npz")), np.load(os.path.join(gold, ref + ".npz"))
        for nm in a.files:
            x, y = np.ascontiguousarray(a[nm], dtype=np.float64), np.ascontiguousarray(b[nm], dtype=np.float64)
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (ref, nm)
