"""One case table for the training GEMM wrappers (gemm_nt, gemm_tn, gemm_ks, colsum_launch behind cvae_selftest_gemm), shared by
the stand-alone sanitizer driver (tests/emu/gemm_asan_main.cpp), the emulator test and the GPU test.

Operands are small integers in [-4, 4] stored as fp32 (masks: 0 or 2, the inverted-dropout values at p = 0.5): every product and
every partial sum is an integer below 2^24, exact in fp32 in ANY summation order, so the result must equal the float64 numpy
reference bit for bit at every tile, split and kernel.  The reference is written from the documented formulas only:

    nt      C[m, n] (+)= sum_k A[m*lda + seg(k)] * B[n*ldb + k] + bias[n];  seg(k) = (k // seglen)*segstride + k % seglen
            mask [B][T][N], M = T*Bp: row f*Bp + b times mask[b, f, n], rows b >= B become 0
    tn      C[i, j] (+)= sum_m A[m*lda + i] * B[m*ldb + seg(j)]
    ks      C[m, n] (+)= sum_k A[m*lda + k] * B[n*ldb + k]
    colsum  C[n] (+)= sum_m A[m*lda + n]

The operand extents [a_lo, a_hi), [b_lo, b_hi), [0, c_hi) are the kernels' contracts (include/cyclevae_hip.h), computed here a second
time: the library refuses a case whose extents are smaller than what it derives itself, and the sanitizer driver allocates exactly
these extents.

What the table leaves out (each class below still appears with every tile; combinations were dropped, never a class):
  * the full cross product M x N x K x ks x segment form x bias x accumulate per tile (7 x 5 x 4 x 4 x 5 x 3 x 2 x 2 = 33,600 nt
    cases alone): every tile sees a 12-entry list of (K, ks) pairs that holds every K, every ks and the named coincidences
    (K = 16 with ks > 1: one slice; K = 48 with ks = 5 / 16: fewer slices than asked; K = 80 with ks = 2: short last slice), and the
    M, N, segment-form, bias, accumulate and ldc classes cycle over that list with different periods;
  * tn likewise over a 10-entry list of (M, ks) pairs;
  * ks: a 5 x 5 Latin square over (M, N) with K = Ks[(i + j) % 5], so every (M, N), (M, K) and (N, K) pair appears once;
  * colsum: every (rows, n) pair, accumulate alternating;
  * a split that is lost because the PADDED tiles overflow the work space (ntile > 4096 or ks*ntile*1024*TM*TN > 2^24 floats) needs
    an output of at least 1024 tiles: too large for a quick test, not in the table.
"""

import zlib

import numpy as np

import _cabi

NT, TN, KS, COLSUM = _cabi.GEMM_NT, _cabi.GEMM_TN, _cabi.GEMM_KS, _cabi.GEMM_COLSUM
KIND_NAMES = {NT: "nt", TN: "tn", KS: "ks", COLSUM: "colsum"}
PART_FLOATS = 16 << 20        # GEMM_PART_FLOATS
CNT = _cabi.SELFTEST_GEMM_CNT
TILES = ((4, 4), (3, 4), (2, 4), (3, 2), (2, 2), (1, 2), (1, 1))
SPLITS = (1, 2, 3, 5, 16)

# one line of plain integers per case in the list the sanitizer driver reads, in this order
FIELDS = ("kind", "acc", "split", "M", "N", "K", "seglen", "mB", "mBp", "mT", "lda", "ldb", "ldc", "segstride", "a_lo", "a_hi", "b_lo",
          "b_hi", "c_hi", "bias", "force", "old", "seed", "e_tiled", "e_TM", "e_TN", "e_nz", "zero_pad")


def up(x, m):
    return (x + m - 1) // m * m


def nblk(n, per):
    return (n + per - 1) // per


def seg_index(n, seglen, segstride):
    k = np.arange(n)
    return (k // seglen) * segstride + k % seglen


class Case(dict):
    __getattr__ = dict.__getitem__

    def name(self):
        s = "%s M%d N%d K%d sl%d ss%d lda%d ldb%d ldc%d acc%d" % (KIND_NAMES[self.kind], self.M, self.N, self.K, self.seglen, self.segstride,
                                                                  self.lda, self.ldb, self.ldc, self.acc)
        s += " force%d" % self.force + (" old" if self.old else "") + (" bias" if self.bias else "") + ("" if self.split else " nows")
        return s + (" mask%d/%d" % (self.mB, self.mBp) if self.mB else "")

    def options(self):
        return {"gemm_force": self.force, "train_old_gemm": self.old}


def _aligned_paths(c):
    """(operands aligned for the LDS-tiled / two-stage kernel, that kernel runs): bases are always 16-byte aligned here."""
    if c.kind == NT:
        al = c.lda % 4 == 0 and c.ldb % 4 == 0 and c.segstride % 4 == 0
    elif c.kind == TN:
        al = c.lda % 4 == 0 and c.ldb % 4 == 0 and c.seglen % 4 == 0 and c.segstride % 4 == 0
    elif c.kind == COLSUM:
        al = c.lda % 4 == 0 and bool(c.split) and nblk(c.N, 64) <= CNT
    else:
        return True
    return al and not c.old


def _extents(c):
    """The floats around A, B, C that the contract lets the kernels touch."""
    M, N, K = c.M, c.N, c.K
    tiled = _aligned_paths(c)
    a_lo = b_lo = b_hi = 0
    if c.kind == NT:
        nseg = 1 if K <= c.seglen else K // c.seglen
        last = (nseg - 1) * c.segstride
        a_lo, a_hi = min(0, last), (M - 1) * c.lda + max(0, last) + min(K, c.seglen)
        b_hi = (N - 1) * c.ldb + K
        c_hi = M * c.ldc if (c.mB and not tiled) else (M - 1) * c.ldc + N
    elif c.kind == TN:
        q = 4 if tiled else 1
        a_hi = (M - 1) * c.lda + up(N, q)
        ends = [s * c.segstride + up(min(c.seglen, K - s * c.seglen), q) for s in range(nblk(K, c.seglen))]
        b_lo = min(0, (nblk(K, c.seglen) - 1) * c.segstride)
        b_hi = (M - 1) * c.ldb + max(ends)
        c_hi = (N - 1) * c.ldc + K
    elif c.kind == KS:
        a_hi, b_hi, c_hi = (M - 1) * c.lda + K, (N - 1) * c.ldb + K, (M - 1) * c.ldc + N
    else:
        a_hi, c_hi = (M - 1) * c.lda + (up(N, 4) if tiled else N), N
    return a_lo, a_hi, b_lo, b_hi, c_hi


def _expect(c):
    """[tiled, TM, TN, slices] the wrappers must report, from their own formulas (gemm_nt / gemm_tn / colsum_launch)."""
    if c.kind == KS:
        return 1, 0, 0, 1
    if not _aligned_paths(c):
        return 0, 0, 0, 1
    if c.kind == COLSUM:
        rs = min(64, max(1, 1024 // nblk(c.N, 64)))
        return 1, 0, 0, nblk(c.M, up(nblk(c.M, rs), 16))
    assert c.force > 0, "a tiled case needs gemm_force (the cost model's own choice is not part of the table)"
    TM, TN, k = c.force // 10000, c.force // 100 % 100, c.force % 100
    rows, cols, depth = (c.M, c.N, c.K) if c.kind == NT else (c.N, c.K, c.M)
    ks = k if (k > 1 and c.split and k * rows * cols <= PART_FLOATS) else 1
    ntile = nblk(cols, 32 * TN) * nblk(rows, 32 * TM)
    if ks > 1 and (ntile > CNT or ks * ntile * 1024 * TM * TN > PART_FLOATS):
        ks = 1
    chunk = up(nblk(depth, ks), 16) if ks > 1 else depth
    return 1, TM, TN, (nblk(depth, chunk) if ks > 1 else 1)


def make_case(kind, M, N, K=0, acc=0, split=1, seglen=0, segstride=0, lda=0, ldb=0, ldc=0, bias=0, mask=None, force=0, old=0):
    c = Case(kind=kind, acc=acc, split=split, M=M, N=N, K=K, seglen=seglen, segstride=segstride, lda=lda, ldb=ldb, ldc=ldc, bias=bias,
             force=force, old=old, mB=0, mBp=0, mT=0)
    if mask:
        c["mB"], c["mBp"], c["mT"] = mask
        assert c.mT * c.mBp == M and 1 <= c.mB <= c.mBp
    c["seed"] = zlib.crc32(repr(sorted(c.items())).encode()) & 0x7fffffff       # (operands depend on the case alone, not on its place)
    c["a_lo"], c["a_hi"], c["b_lo"], c["b_hi"], c["c_hi"] = _extents(c)
    c["e_tiled"], c["e_TM"], c["e_TN"], c["e_nz"] = _expect(c)
    c["zero_pad"] = int(bool(c.mB) and not c.e_tiled)
    return c


def nt_case(M, N, K, form, **kw):
    """form 0: one segment (segstride 0, seglen K); 1: overlapping rows as in conv0 (lda = seglen = 16, segstride = 4*lda); 2: negative
    stride as in the conv-transpose products (base pointer at the last segment); 3: one segment, lda not a multiple of 4."""
    if form == 0 or (form in (1, 2) and K == 16):
        seglen, ss, lda = K, 0, K + 4 * (M % 2)
    elif form == 1:
        seglen, lda = 16, 16
        ss = 4 * lda
    elif form == 2:
        seglen, lda = 16, 20
        ss = -3 * lda
    else:
        seglen, ss, lda = K, 0, K + 1
    pad = kw.pop("ldc_pad", 3)
    return make_case(NT, M, N, K, seglen=seglen, segstride=ss, lda=lda, ldb=K + 4 * (N % 2), ldc=N + pad, **kw)


def tn_case(M, N1, N2, form, **kw):
    """form 0: seglen = up(N2, 4) (one segment; the non-zero segstride must not matter); 1: seglen 4, segments 8 floats apart;
    2: one segment, lda not a multiple of 4."""
    if form == 1:
        seglen, ss = 4, 8
        ldb = nblk(N2, 4) * 8 + 4
    else:
        seglen = up(N2, 4)
        ss, ldb = 4 * seglen, seglen + 4 * (M % 2)
    lda = up(N1, 4) + 4 * (N2 % 2) if form != 2 else N1 + 1
    return make_case(TN, M, N1, N2, seglen=seglen, segstride=ss, lda=lda, ldb=ldb, ldc=N2 + kw.pop("ldc_pad", 1), **kw)


NT_K_KS = ((16, 1), (16, 2), (48, 5), (48, 16), (80, 2), (80, 3), (272, 1), (272, 2), (272, 3), (272, 5), (272, 16), (48, 1))
TN_M_KS = ((1, 1), (5, 2), (16, 3), (17, 2), (17, 16), (83, 1), (83, 2), (83, 3), (83, 5), (83, 16))


def build_table():
    cases = []
    for TM, TN_ in TILES:
        BM, BN = 32 * TM, 32 * TN_
        Ms, Ns = (1, BM - 1, BM, BM + 1, 2 * BM + 5), (1, BN - 3, BN, BN + 1)
        for i, (K, ks) in enumerate(NT_K_KS):
            cases.append(nt_case(Ms[i % 5], Ns[(i + i // 4) % 4], K, form=i % 3, bias=(i // 2) % 2, acc=(i // 3 + i) % 2,
                                 ldc_pad=(0 if i % 6 == 5 else 3), force=TM * 10000 + TN_ * 100 + ks))
        # mask epilogue with B < Bp (M = T*Bp one row past the tile; split and unsplit)
        for ks in (1, 3):
            Bp, T = (BM + 1, 1) if TM % 2 else ((BM + 2) // 2, 2)
            cases.append(nt_case(T * Bp, BN + 1, 80, form=0, bias=1, acc=ks // 3, mask=(Bp - 2, Bp, T), force=TM * 10000 + TN_ * 100 + ks))
        for i, (M, ks) in enumerate(TN_M_KS):
            cases.append(tn_case(M, Ms[(i + 1) % 5], Ns[(i + i // 4) % 4], form=i % 2, acc=(i // 2) % 2, force=TM * 10000 + TN_ * 100 + ks))
        # no work space: the forced split must be dropped
        cases.append(nt_case(BM + 1, BN - 3, 272, form=0, split=0, force=TM * 10000 + TN_ * 100 + 3))
        cases.append(tn_case(83, BM + 1, BN - 3, form=0, split=0, force=TM * 10000 + TN_ * 100 + 3))
    # ---- the simple kernels: train_old_gemm, and an lda that is not a multiple of 4
    for old, form in ((1, 0), (1, 1), (1, 2), (0, 3)):
        cases.append(nt_case(129, 125, 80, form=form, bias=1, acc=old, old=old, force=20203))
        cases.append(nt_case(1, 129, 16, form=form, acc=1 - old, old=old, force=20203))
    cases.append(nt_case(2 * 35, 67, 48, form=0, bias=1, mask=(33, 35, 2), old=1))          # the mask through k_mul_mask_tm
    cases.append(nt_case(2 * 35, 67, 48, form=3, acc=1, mask=(33, 35, 2)))
    for old, form in ((1, 0), (1, 1), (0, 2)):
        cases.append(tn_case(83, 65, 61, form=form, acc=old, old=old, force=20203))
        cases.append(tn_case(17, 1, 129, form=form, acc=1 - old, old=old, force=20203))
    # ---- gemm_ks
    Mk, Nk, Kk = (1, 15, 16, 17, 33), (1, 15, 16, 17, 50), (16, 48, 64, 80, 272)
    for i, M in enumerate(Mk):
        for j, N in enumerate(Nk):
            K = Kk[(i + j) % 5]
            cases.append(make_case(KS, M, N, K, acc=(i + 2 * j) % 2, lda=K + 4 * (j % 2), ldb=K + 4 * (i % 2), ldc=N + 2))
    # ---- colsum_launch
    for i, rows in enumerate((1, 15, 16, 17, 31, 32, 33, 100, 1030)):
        for j, n in enumerate((1, 3, 4, 63, 64, 65, 130)):
            cases.append(make_case(COLSUM, rows, n, acc=(i + j) % 2, lda=up(n, 4) + 4 * (i % 2)))
    for rows, n in ((1, 3), (33, 65), (100, 130)):
        cases.append(make_case(COLSUM, rows, n, acc=rows % 2, lda=up(n, 4), old=1))
        cases.append(make_case(COLSUM, rows, n, acc=1 - rows % 2, lda=n + 1))
        cases.append(make_case(COLSUM, rows, n, acc=rows % 2, lda=up(n, 4), split=0))
    return cases


def build_real_table():
    """One shape per kernel and tile for the N(0, 1) run (a change of precision class is invisible to integer operands)."""
    cases = []
    for TM, TN_ in TILES:
        BM, BN = 32 * TM, 32 * TN_
        cases.append(nt_case(BM + 1, BN + 1, 272, form=1, bias=1, acc=1, force=TM * 10000 + TN_ * 100 + 3))
        cases.append(tn_case(83, BM + 1, BN + 1, form=1, acc=1, force=TM * 10000 + TN_ * 100 + 3))
    cases.append(nt_case(2 * 35, 67, 272, form=0, bias=1, acc=1, mask=(33, 35, 2), force=20202))
    cases.append(nt_case(129, 125, 272, form=1, bias=1, acc=1, old=1))
    cases.append(tn_case(83, 65, 61, form=1, acc=1, old=1))
    cases.append(make_case(KS, 17, 50, 272, acc=1, lda=272, ldb=276, ldc=52))
    cases.append(make_case(COLSUM, 1030, 130, acc=1, lda=136))
    cases.append(make_case(COLSUM, 1030, 130, acc=1, lda=136, old=1))
    return cases


_TABLE = {}


def table(real=False):
    if real not in _TABLE:
        _TABLE[real] = build_real_table() if real else build_table()
    return _TABLE[real]


def write_list(path, cases):
    with open(path, "w") as f:
        f.write("%d %d\n" % (len(cases), len(FIELDS)))
        for c in cases:
            f.write(" ".join(str(int(c[k])) for k in FIELDS) + "\n")


# ---------------------------------------------------------------------------------------------------------------
# operands and the float64 reference
# ---------------------------------------------------------------------------------------------------------------
def operands(c, real=False):
    rng = np.random.RandomState(c.seed)

    def draw(n):
        return (rng.standard_normal(n) if real else rng.randint(-4, 5, n)).astype(np.float32)
    ops = {"A": draw(c.a_hi - c.a_lo), "C": draw(c.c_hi)}
    if c.kind != COLSUM:
        ops["B"] = draw(c.b_hi - c.b_lo)
    if c.bias:
        ops["bias"] = draw(c.N)
    if c.mB:
        ops["mask"] = (2 * rng.randint(0, 2, c.mB * c.mT * c.N)).astype(np.float32)
    return ops


def reference(c, ops):
    """(expected C as float64 [c_hi], untouched floats included; sum of the absolute terms per float, 0 where nothing is summed)."""
    A, C0 = ops["A"].astype(np.float64), ops["C"].astype(np.float64)
    M, N, K = c.M, c.N, c.K
    rows = np.arange(M)[:, None]
    if c.kind == COLSUM:
        A2 = A[rows * c.lda + np.arange(N)[None, :]]
        P, S = A2.sum(0)[None, :], np.abs(A2).sum(0)[None, :]
        out_rows, out_cols, ldc = 1, N, N
    else:
        B = ops["B"].astype(np.float64)
        if c.kind == TN:
            A2 = A[rows * c.lda + np.arange(N)[None, :]]                                           # [M][N1]
            B2 = B[rows * c.ldb + seg_index(K, c.seglen, c.segstride)[None, :] - c.b_lo]           # [M][N2]
            P, S = A2.T @ B2, np.abs(A2).T @ np.abs(B2)
            out_rows, out_cols = N, K
        else:
            kk = seg_index(K, c.seglen, c.segstride) if c.kind == NT else np.arange(K)
            A2 = A[rows * c.lda + kk[None, :] - c.a_lo]                                            # [M][K]
            B2 = B[np.arange(N)[:, None] * c.ldb + np.arange(K)[None, :]]                          # [N][K]
            P, S = A2 @ B2.T, np.abs(A2) @ np.abs(B2).T
            out_rows, out_cols = M, N
        ldc = c.ldc
    idx = np.arange(out_rows)[:, None] * ldc + np.arange(out_cols)[None, :]
    if c.bias:
        P, S = P + ops["bias"].astype(np.float64)[None, :], S + np.abs(ops["bias"].astype(np.float64))[None, :]
    if c.acc:
        P, S = P + C0[idx], S + np.abs(C0[idx])
    E, SA = C0.copy(), np.zeros_like(C0)
    if c.mB:
        mk = ops["mask"].astype(np.float64).reshape(c.mB, c.mT, N)
        full = np.zeros((c.mT, c.mBp, N))
        full[:, :c.mB] = mk.transpose(1, 0, 2)
        full = full.reshape(M, N)
        P, S = P * full, S * full
        if c.zero_pad:
            E[:M * ldc] = 0.0
    E[idx], SA[idx] = P, S
    return E, SA


def slices_depth(c):
    return c.e_nz, (c.M if c.kind in (TN, COLSUM) else c.K)


# ---------------------------------------------------------------------------------------------------------------
# running a case on a library whose "device" memory is behind an arena (numpy for the emulator, one torch tensor on the GPU)
# ---------------------------------------------------------------------------------------------------------------
class NumpyArena(object):
    """Operands as views inside one larger NaN-filled array: a read outside a view gives NaN (a wrong result), a write outside it
    shows up in check_guards()."""
    GAP = 64

    def __init__(self, floats=1 << 20):
        self.buf = np.full(floats, np.nan, np.float32)
        assert self.buf.ctypes.data % 16 == 0
        self.reset()

    def reset(self):
        self.buf[:getattr(self, "top", None)] = np.nan
        self.top = self.GAP
        self.used = []

    def put(self, a):
        off = self.top
        assert off + a.size + self.GAP <= len(self.buf)
        self.write(off, a)
        self.top = up(off + a.size + self.GAP, 4)
        self.used.append((off, a.size))
        return off

    def write(self, off, a):
        self.buf[off:off + a.size] = a

    def read(self, off, n):
        return self.buf[off:off + n].copy()

    def address(self, off):
        return self.buf.ctypes.data + 4 * off

    def sync(self):
        pass

    def guards_intact(self):
        whole = self.read(0, self.top)
        keep = np.ones(whole.size, bool)
        for off, n in self.used:
            keep[off:off + n] = False
        return bool(np.all(np.isnan(whole[keep])))


def launch(lib, arena, c, ops, work_addr, work_bytes, stream=None):
    """Places the operands, runs the case once; returns (ran, offset of C in the arena)."""
    arena.reset()
    oA = arena.put(ops["A"])
    oB = arena.put(ops["B"]) if "B" in ops else None
    ob = arena.put(ops["bias"]) if "bias" in ops else None
    om = arena.put(ops["mask"]) if "mask" in ops else None
    oC = arena.put(ops["C"])
    gc = _cabi.GemmCase(kind=c.kind, accumulate=c.acc, use_split=c.split, M=c.M, N=c.N, K=c.K, seglen=c.seglen, mask_B=c.mB, mask_Bp=c.mBp,
                        mask_T=c.mT, lda=c.lda, ldb=c.ldb, ldc=c.ldc, segstride=c.segstride, a_lo=c.a_lo, a_hi=c.a_hi, b_lo=c.b_lo,
                        b_hi=c.b_hi, c_hi=c.c_hi, A=arena.address(oA - c.a_lo), B=None if oB is None else arena.address(oB - c.b_lo),
                        bias=None if ob is None else arena.address(ob), mask=None if om is None else arena.address(om),
                        C=arena.address(oC))
    ran = lib.selftest_gemm(gc, work_addr, work_bytes, stream)
    return ran, oC, gc


def run_case(lib, arena, c, work_addr, work_bytes, read_counters, real=False, stream=None):
    """Runs one case and checks it; returns the largest |d| / bound of a real-valued case (0.0 for an integer case).
    The caller has set c.options() on `lib`."""
    ops = operands(c, real)
    E, SA = reference(c, ops)
    ran, oC, gc = launch(lib, arena, c, ops, work_addr, work_bytes, stream)
    arena.sync()
    got = arena.read(oC, c.c_hi)
    assert ran == [c.e_tiled, c.e_TM, c.e_TN, c.e_nz], (c.name(), ran)
    assert arena.guards_intact(), "write outside the operands: " + c.name()
    assert not np.any(read_counters()), "arrival counters not back at zero: " + c.name()
    ratio = 0.0
    if real:
        nz, depth = slices_depth(c)
        bound = 2.0 * (depth + nz + 2) * 2.0 ** -24 * SA
        d = np.abs(got.astype(np.float64) - E)
        assert np.all(np.isfinite(got)), c.name()
        assert np.all(d <= bound), (c.name(), float(np.max(d - bound)))
        pos = bound > 0
        ratio = float(np.max(d[pos] / bound[pos])) if pos.any() else 0.0
    else:
        bad = np.flatnonzero(~(got.astype(np.float64) == E))
        assert bad.size == 0, (c.name(), "first wrong floats of C", bad[:8].tolist(), got[bad[:8]].tolist(), E[bad[:8]].tolist())
    if c.e_nz > 1:      # the same call again: identical bits whichever block arrives last
        arena.write(oC, ops["C"])
        ran2 = lib.selftest_gemm(gc, work_addr, work_bytes, stream)
        arena.sync()
        again = arena.read(oC, c.c_hi)
        assert ran2 == ran and again.tobytes() == got.tobytes(), "not reproducible: " + c.name()
        assert not np.any(read_counters()), c.name()
    return ratio


def work_numpy(lib):
    """Zeroed work space in host memory (emulator): (array, address, bytes, counter reader)."""
    nbytes = lib.selftest_gemm_work_bytes()
    w = np.zeros(nbytes // 4, np.uint32)
    assert w.ctypes.data % 16 == 0
    return w, w.ctypes.data, nbytes, (lambda: w[-CNT:])
