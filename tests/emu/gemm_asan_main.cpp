// Stand-alone driver of cvae_selftest_gemm for a -fsanitize=address build of the host-fiber emulation (tests/test_emu_gemm.py
// builds and runs it; nothing of it is loaded into python).  Reads the case list tests/gemm_util.py writes (plain integers, one
// case per line), allocates every operand with malloc at EXACTLY the contract's extent -- no margin, so a read or write outside a
// contract is a sanitizer report --, fills it with small integers (exact in fp32 in any summation order), runs the case through the
// library and compares with a double-precision sum of the documented formulas, bit for bit.  Exit status 0 only when every case
// matched, reported the expected kernel / tile / slices and left the arrival counters at zero.
#include <cyclevae_hip.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

enum { F_KIND, F_ACC, F_SPLIT, F_M, F_N, F_K, F_SEGLEN, F_MB, F_MBP, F_MT, F_LDA, F_LDB, F_LDC, F_SS, F_ALO, F_AHI, F_BLO, F_BHI, F_CHI,
       F_BIAS, F_FORCE, F_OLD, F_SEED, F_ETILED, F_ETM, F_ETN, F_ENZ, F_ZEROPAD, F_COUNT };

unsigned rs = 1;
float small_int() { rs = rs * 1664525u + 1013904223u; return (float)((int)((rs >> 16) % 9) - 4); }
float* fill(long n, bool mask = false) {
    float* p = (float*)malloc((size_t)(n > 0 ? n : 1) * sizeof(float));
    for (long i = 0; i < n; ++i) p[i] = mask ? (small_int() > 0.f ? 2.f : 0.f) : small_int();
    return p;
}
long seg(long k, long seglen, long ss) { return (k / seglen) * ss + k % seglen; }

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s case-list\n", argv[0]); return 2; }
    setvbuf(stdout, nullptr, _IOLBF, 0);      // (a sanitizer abort must not lose the lines printed so far)
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    long ncase = 0, nfield = 0;
    if (fscanf(f, "%ld %ld", &ncase, &nfield) != 2 || nfield != F_COUNT) { fprintf(stderr, "bad case list header\n"); return 2; }
    cvae_ctx* ctx = cvae_ctx_create();
    const size_t work_bytes = cvae_selftest_gemm_work_bytes(ctx);
    unsigned char* work = (unsigned char*)calloc(work_bytes, 1);
    const unsigned* cnt = (const unsigned*)(work + work_bytes) - CVAE_SELFTEST_GEMM_CNT;
    long bad = 0, done = 0;
    for (long ci = 0; ci < ncase; ++ci) {
        long long v[F_COUNT];
        for (int i = 0; i < F_COUNT; ++i)
            if (fscanf(f, "%lld", &v[i]) != 1) { fprintf(stderr, "case %ld: short line\n", ci); return 2; }
        const long M = v[F_M], N = v[F_N], K = v[F_K], lda = v[F_LDA], ldb = v[F_LDB], ldc = v[F_LDC], ss = v[F_SS], sl = v[F_SEGLEN];
        const int kind = (int)v[F_KIND];
        rs = (unsigned)v[F_SEED] * 2654435761u + 12345u;
        float* Ab = fill(v[F_AHI] - v[F_ALO]);
        float* Bb = kind == CVAE_GEMM_COLSUM ? nullptr : fill(v[F_BHI] - v[F_BLO]);
        float* bias = v[F_BIAS] ? fill(N) : nullptr;
        float* mask = v[F_MB] ? fill(v[F_MB] * v[F_MT] * N, true) : nullptr;
        float* C = fill(v[F_CHI]);
        std::vector<float> C0(C, C + v[F_CHI]);
        const float* A = Ab - v[F_ALO];
        const float* B = Bb ? Bb - v[F_BLO] : nullptr;
        // the expected C in double: untouched floats keep their bits
        std::vector<double> E(C0.begin(), C0.end());
        const long orows = kind == CVAE_GEMM_TN ? N : (kind == CVAE_GEMM_COLSUM ? 1 : M), ocols = kind == CVAE_GEMM_TN ? K : N;
        const long oldc = kind == CVAE_GEMM_COLSUM ? N : ldc;
        if (v[F_ZEROPAD])
            for (long i = 0; i < M * ldc; ++i) E[i] = 0.0;
        for (long r = 0; r < orows; ++r)
            for (long q = 0; q < ocols; ++q) {
                double s = 0.0;
                if (kind == CVAE_GEMM_NT) for (long k = 0; k < K; ++k) s += (double)A[r * lda + seg(k, sl, ss)] * B[q * ldb + k];
                else if (kind == CVAE_GEMM_TN) for (long m = 0; m < M; ++m) s += (double)A[m * lda + r] * B[m * ldb + seg(q, sl, ss)];
                else if (kind == CVAE_GEMM_KS) for (long k = 0; k < K; ++k) s += (double)A[r * lda + k] * B[q * ldb + k];
                else for (long m = 0; m < M; ++m) s += A[m * lda + q];
                if (bias) s += bias[q];
                if (v[F_ACC]) s += C0[r * oldc + q];
                if (mask) {
                    const long b = r % v[F_MBP], fr = r / v[F_MBP];
                    s = b < v[F_MB] ? s * mask[(b * v[F_MT] + fr) * N + q] : 0.0;
                }
                E[r * oldc + q] = s;
            }
        cvae_set_option(ctx, "gemm_force", v[F_FORCE]);
        cvae_set_option(ctx, "train_old_gemm", v[F_OLD]);
        cvae_gemm_case gc;
        memset(&gc, 0, sizeof gc);
        gc.kind = kind; gc.accumulate = (int32_t)v[F_ACC]; gc.use_split = (int32_t)v[F_SPLIT];
        gc.M = (int32_t)M; gc.N = (int32_t)N; gc.K = (int32_t)K; gc.seglen = (int32_t)sl;
        gc.mask_B = (int32_t)v[F_MB]; gc.mask_Bp = (int32_t)v[F_MBP]; gc.mask_T = (int32_t)v[F_MT];
        gc.lda = lda; gc.ldb = ldb; gc.ldc = ldc; gc.segstride = ss;
        gc.a_lo = v[F_ALO]; gc.a_hi = v[F_AHI]; gc.b_lo = v[F_BLO]; gc.b_hi = v[F_BHI]; gc.c_hi = v[F_CHI];
        gc.A = A; gc.B = B; gc.bias = bias; gc.mask = mask; gc.C = C;
        int32_t ran[4];
        const int rc = cvae_selftest_gemm(ctx, &gc, work, work_bytes, ran, nullptr);
        long wrong = -1;
        for (long i = 0; rc == 0 && i < v[F_CHI]; ++i)
            if (!((double)C[i] == E[i])) { wrong = i; break; }
        bool ok = rc == 0 && wrong < 0;
        if (rc != 0) printf("case %ld: refused (%d): %s\n", ci, rc, cvae_last_error_string());
        if (wrong >= 0) printf("case %ld (kind %d M %ld N %ld K %ld force %lld): C[%ld] = %g, expected %g\n", ci, kind, M, N, K, v[F_FORCE], wrong, C[wrong], E[wrong]);
        if (rc == 0 && (ran[0] != v[F_ETILED] || ran[1] != v[F_ETM] || ran[2] != v[F_ETN] || ran[3] != v[F_ENZ])) {
            printf("case %ld: ran {%d, %d, %d, %d}, expected {%lld, %lld, %lld, %lld}\n", ci, ran[0], ran[1], ran[2], ran[3], v[F_ETILED], v[F_ETM], v[F_ETN], v[F_ENZ]);
            ok = false;
        }
        for (int i = 0; i < CVAE_SELFTEST_GEMM_CNT; ++i)
            if (cnt[i]) { printf("case %ld: arrival counter %d left at %u\n", ci, i, cnt[i]); ok = false; break; }
        if (!ok) { ++bad; memset(work + work_bytes - 4 * CVAE_SELFTEST_GEMM_CNT, 0, 4 * CVAE_SELFTEST_GEMM_CNT); }
        ++done;
        free(Ab); free(Bb); free(bias); free(mask); free(C);
    }
    fclose(f);
    cvae_ctx_destroy(ctx);
    free(work);
    printf("cases %ld bad %ld\n", done, bad);
    fflush(stdout);
    return bad != 0;
}
