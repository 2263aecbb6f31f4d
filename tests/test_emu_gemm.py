"""The training GEMM wrappers on their own (gemm_nt / gemm_tn / gemm_ks / colsum_launch behind cvae_selftest_gemm) on the host-fiber
emulator: every LDS tile x contraction split x edge class of tests/gemm_util.py against the float64 numpy reference, bit for bit
(integer operands: exact in any summation order), plus one N(0, 1) shape per kernel and tile against the derived bound
|d| <= 2 (depth + slices + 2) 2^-24 (sum |a||b| + |bias| + |C_old|).

test_asan_driver_runs_the_table_clean runs the same table in a stand-alone program built with -fsanitize=address whose operands are
malloc'ed at exactly the contracts' extents (tests/emu/gemm_asan_main.cpp): an over-read that lands in the NaN arena's neighbour
here, or in allocated memory on a GPU, is an error there.
"""
import os
import subprocess

import numpy as np
import pytest

import _cabi
import gemm_util as gu
from emu_util import CLANG, CSRC, EMU_DIR, ROOT, emu_lib

ASAN_EXE = os.path.join(EMU_DIR, "gemm_asan")


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


@pytest.fixture(scope="module")
def bench(lib):
    w, addr, nbytes, counters = gu.work_numpy(lib)
    return {"arena": gu.NumpyArena(), "work": w, "addr": addr, "bytes": nbytes, "counters": counters}


def run_all(lib, options, bench, cases, real=False):
    worst = 0.0
    for c in cases:
        options(**c.options())
        worst = max(worst, gu.run_case(lib, bench["arena"], c, bench["addr"], bench["bytes"], bench["counters"], real=real))
    return worst


def test_table_holds_every_class_with_every_tile():
    cases = gu.table()
    for TM, TN in gu.TILES:
        BM, BN = 32 * TM, 32 * TN
        mine = [c for c in cases if c.e_tiled and (c.e_TM, c.e_TN) == (TM, TN)]
        nt, tn = [c for c in mine if c.kind == gu.NT], [c for c in mine if c.kind == gu.TN]
        assert {c.M for c in nt} >= {1, BM - 1, BM, BM + 1, 2 * BM + 5} and {c.N for c in nt} >= {1, BN - 3, BN, BN + 1}
        assert {c.K for c in nt} >= {16, 48, 80, 272} and {c.force % 100 for c in nt} >= set(gu.SPLITS)
        assert {c.N for c in tn} >= {1, BM - 1, BM, BM + 1, 2 * BM + 5} and {c.K for c in tn} >= {1, BN - 3, BN, BN + 1}
        assert {c.M for c in tn} >= {1, 5, 16, 17, 83} and {c.force % 100 for c in tn} >= set(gu.SPLITS)
        assert any(c.N % 4 for c in tn) and any(c.K % 4 for c in tn) and {c.seglen for c in tn if c.K > 4} >= {4}
        assert any(c.K == 16 and c.force % 100 > 1 and c.e_nz == 1 for c in nt)              # one slice despite ks > 1
        assert any(c.K == 48 and 1 < c.e_nz < c.force % 100 for c in nt)                      # fewer slices than asked
        assert any(c.K == 80 and c.force % 100 == 2 and c.e_nz == 2 for c in nt)              # short last slice (48 + 32)
        assert any(c.segstride < 0 for c in nt) and any(c.segstride > 0 and c.lda == 16 for c in nt)
        assert {c.bias for c in nt} == {0, 1} and {c.acc for c in nt} == {0, 1} == {c.acc for c in tn}
        assert any(c.mB and c.mB < c.mBp for c in nt) and any(c.ldc > c.N for c in nt)
        assert any(c.e_nz == 1 and c.force % 100 > 1 and c.M <= 16 for c in tn)               # mchunk = up(nblk(M, ks), 16) covers M
        assert any(not c.split and c.e_nz == 1 for c in nt) and any(not c.split and c.e_nz == 1 for c in tn)
    simple = [c for c in cases if not c.e_tiled]
    assert {c.kind for c in simple if c.old} == {gu.NT, gu.TN, gu.COLSUM} == {c.kind for c in simple if c.lda % 4}
    assert any(c.kind == gu.NT and c.mB and c.old for c in simple) and any(c.kind == gu.NT and c.mB and c.lda % 4 for c in simple)
    assert len(cases) < 500


@pytest.mark.parametrize("kind", [gu.NT, gu.TN, gu.KS, gu.COLSUM], ids=["nt", "tn", "ks", "colsum"])
def test_integer_table_bit_for_bit(lib, options, bench, kind):
    run_all(lib, options, bench, [c for c in gu.table() if c.kind == kind])


def test_real_valued_within_derived_bound(lib, options, bench):
    worst = run_all(lib, options, bench, gu.table(real=True), real=True)
    print("largest |d| / bound over the real-valued cases: %.3f" % worst)
    assert worst <= 1.0


def test_contract_violations_are_refused(lib, options, bench):
    """A call outside a contract is refused with a message, never launched: C keeps its bits."""
    ok = gu.nt_case(33, 31, 48, form=1, force=10203)
    variants = [dict(K=40), dict(seglen=24, K=48), dict(K=80, seglen=32), dict(a_hi=ok.a_hi - 1), dict(b_hi=ok.b_hi - 1), dict(c_hi=ok.c_hi - 1),
                dict(ldc=ok.N - 1), dict(M=0)]
    neg = gu.nt_case(33, 31, 48, form=2, force=10203)
    tn = gu.tn_case(17, 33, 30, form=1, force=10203)
    ks = gu.make_case(gu.KS, 16, 16, 48, lda=48, ldb=48, ldc=16)
    cs = gu.make_case(gu.COLSUM, 33, 30, lda=32)
    todo = [(ok, v) for v in variants] + [(neg, dict(a_lo=neg.a_lo + 1)), (tn, dict(a_hi=tn.a_hi - 1)), (tn, dict(b_hi=tn.b_hi - 1)),
                                          (ks, dict(K=40)), (cs, dict(a_hi=cs.a_hi - 1)), (ok, dict(kind=7))]
    assert tn.a_hi == 16 * tn.lda + 36 and cs.a_hi == 32 * 32 + 32          # (the padded reach, not N1 = 33 / n = 30)
    for base, change in todo:
        c = gu.Case(base)
        c.update(change)
        options(**c.options())
        ops = gu.operands(base)
        with pytest.raises(_cabi.CvaeError):
            gu.launch(lib, bench["arena"], c, ops, bench["addr"], bench["bytes"])
        assert lib.lib.cvae_last_error_string().startswith(b"selftest_gemm")
    with pytest.raises(_cabi.CvaeError):                                         # a split without the work space
        gu.launch(lib, bench["arena"], ok, gu.operands(ok), None, 0)


def build_asan_driver():
    """The emulator sources and the driver as one -fsanitize=address executable, cached by mtime like emu_util.build_emu."""
    srcs = [os.path.join(CSRC, "cvae_lib.hip"), os.path.join(EMU_DIR, "emu_rt.cpp")]
    main = os.path.join(EMU_DIR, "gemm_asan_main.cpp")
    deps = srcs + [main] + [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".inc"))]
    deps += [os.path.join(EMU_DIR, "cvae_intrin.h"), os.path.join(EMU_DIR, "hip", "hip_runtime.h"), os.path.join(ROOT, "include", "cyclevae_hip.h")]
    if os.path.exists(ASAN_EXE) and all(os.path.getmtime(ASAN_EXE) >= os.path.getmtime(d) for d in deps):
        return ASAN_EXE
    if not os.path.exists(CLANG):
        return None
    cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address", "-fno-omit-frame-pointer", "-Wno-psabi", "-I", EMU_DIR,
           "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-x", "c++"] + srcs + [main, "-o", ASAN_EXE]
    subprocess.check_call(cmd)
    return ASAN_EXE


def test_asan_driver_runs_the_table_clean(tmp_path):
    exe = build_asan_driver()
    assert exe, "no clang++ with AddressSanitizer at " + CLANG
    path = str(tmp_path / "gemm_cases.txt")
    gu.write_list(path, gu.table())
    # (leak checking off: it needs ptrace, which a sandboxed test user may lack; the driver is about out-of-bounds accesses)
    p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    tail = (p.stdout[-3000:] + "\n" + "\n".join(l for l in p.stderr.splitlines() if "swapcontext" not in l)[:6000])
    assert p.returncode == 0, tail
    assert "cases %d bad 0" % len(gu.table()) in p.stdout, tail
