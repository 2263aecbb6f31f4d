// Stage 6 (decode_gru-cyclevae_gauss.py:328-475) of libcyclevae_hip.so (included by cvae_lib.hip): what the script does between the
// network trajectories and the vocoder, over host job lists.
//   cvae_mc2e_batch   the impulse-response energies mod_pow needs, for every frame of every job in one launch sequence
//   cvae_decode_jobs  mod_pow's coefficient-0 correction, the GV post-filter with its variance, the differential cepstrum, and the
//                     f64 speech-frame gathers, one block per job
// mc2e = freqt + c2ir + energy per frame (cvae_stage6.inc: k_mc2e runs freqt's recurrence on one lane per frame and pays an LDS tree
// per impulse-response sample).  Here
//   freqt  is linear in the frame: c'[j] = sum_i F[i][j] mc[i], and row i of F is the recurrence's zero-input step applied i times
//          to e_0, for any D.  k_freqt_rows builds the rows once per call (anti-diagonal wavefront: thread k owns step k and reads
//          step k-1's last two values); a frame's freqt is then D FMAs per output coefficient, lanes over j.
//   c2ir   h[n] = (1/n) sum_{k=1..n} k c'[k] h[n-k] in blocks of 64 samples: lane l owns n = 64 B + l, sums the contributions of every
//          earlier block on its own (no cross-lane reduction), and the 64 samples of the block itself are closed one after the other,
//          each broadcast through LDS.
// One wave per frame, f64, plain FMAs, every sum in a fixed order: a frame's energy does not depend on the call it is in.
namespace {

struct Mc2eTask {
    cvae_mc2e_job j;
    long long frame0;      // first block of this job
};

// F[0] = e_0; F[k] = A F[k-1] with A the zero-input step of SPTK's freqt at -alpha (k_mc2e's statements with c1[-i] = 0):
//   g[0] = a d[0];  g[1] = b d[0] + a d[1];  g[j] = d[j-1] + a (d[j] - g[j-1])
// Steps are taken blockDim.x at a time: thread t owns step k0 + 1 + t and is at coefficient j = s - t in iteration s, so d[j] is what
// thread t-1 made one iteration earlier (LDS slot, two buffers by the parity of s; thread 0 reads row k0 of F) and d[j-1], g[j-1]
// are the thread's own previous iteration.
__global__ __launch_bounds__(256) void k_freqt_rows(double* F, int Dmax, int irlen, double alpha) {
    double* slot = (double*)CVAE_SMEM;      // [2][blockDim.x]
    const int tid = threadIdx.x, NT = blockDim.x;
    const double a = -alpha, b = 1.0 - a * a;
    for (int j = tid; j < irlen; j += NT) F[j] = j == 0 ? 1.0 : 0.0;
    __syncthreads();
    for (int k0 = 0; k0 + 1 < Dmax; k0 += NT) {
        const int k = k0 + 1 + tid;
        const int nt = Dmax - 1 - k0 < NT ? Dmax - 1 - k0 : NT;
        double dprev = 0.0, gprev = 0.0;
        for (int s = 0; s < irlen + nt - 1; ++s) {
            const int j = s - tid;
            if (tid < nt && j >= 0 && j < irlen) {
                const double dj = tid == 0 ? F[(long)k0 * irlen + j] : slot[((s + 1) & 1) * NT + tid - 1];
                double g;
                if (j == 0) g = a * dj;
                else if (j == 1) g = b * dprev + a * dj;
                else g = dprev + a * (dj - gprev);
                slot[(s & 1) * NT + tid] = g;
                F[(long)k * irlen + j] = g;
                dprev = dj;
                gprev = g;
            }
            __syncthreads();
        }
    }
}

// One 64-lane block per frame.  LDS: kc [irlen] (k c'[k]), h [irlen], mc [Dmax], red [64].
__global__ __launch_bounds__(64) void k_mc2e_batch(const Mc2eTask* tasks, int n_tasks, const double* F, int irlen, int Dmax) {
    double* kc = (double*)CVAE_SMEM;
    double* h = kc + irlen;
    double* mc = h + irlen;
    double* red = mc + Dmax;
    const int lane = threadIdx.x;
    const long long frame = blockIdx.x;
    int lo = 0, hi = n_tasks - 1;
    while (lo < hi) {      // the last task that starts at or before this block
        const int mid = (lo + hi + 1) >> 1;
        if (tasks[mid].frame0 <= frame) lo = mid;
        else hi = mid - 1;
    }
    const cvae_mc2e_job& jb = tasks[lo].j;
    const long long r = frame - tasks[lo].frame0;
    const int D = jb.D;
    for (int i = lane; i < D; i += 64)
        mc[i] = jb.is_f64 ? ((const double*)jb.mc)[r * jb.ld + i] : (double)((const float*)jb.mc)[r * jb.ld + i];
    __syncthreads();
    for (int j = lane; j < irlen; j += 64) {
        double acc = 0.0;
        for (int i = 0; i < D; ++i) acc += F[(long)i * irlen + j] * mc[i];
        if (j == 0) h[0] = exp(acc);
        kc[j] = (double)j * acc;
    }
    __syncthreads();
    for (int base = 0; base < irlen; base += 64) {
        const int n = base + lane;
        double s = 0.0;
        if (n < irlen) {
            // the samples of every earlier block, four interleaved partial sums (base is a multiple of 64) added in a fixed order
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            const double* kn = kc + n;
#pragma unroll 2
            for (int m = 0; m < base; m += 4) {
                s0 += kn[-m] * h[m];
                s1 += kn[-m - 1] * h[m + 1];
                s2 += kn[-m - 2] * h[m + 2];
                s3 += kn[-m - 3] * h[m + 3];
            }
            s = (s0 + s1) + (s2 + s3);
        }
        const int cnt = irlen - base < 64 ? irlen - base : 64;
        for (int t = 0; t < cnt; ++t) {      // sample base + t is complete: its lane publishes it, the lanes behind add its term
            if (lane == t && n > 0) h[n] = s / (double)n;
            cvae_wave_barrier();
            if (lane > t && n < irlen) s += kc[lane - t] * h[base + t];
        }
    }
    __syncthreads();
    double e = 0.0;
    for (int n = lane; n < irlen; n += 64) e += h[n] * h[n];
    red[lane] = e;
    __syncthreads();
    for (int w = 32; w > 0; w >>= 1) {
        if (lane < w) red[lane] += red[lane + w];
        __syncthreads();
    }
    if (lane == 0) jb.e_out[r] = red[0];
}

__device__ __forceinline__ double dec_load(const void* p, long long at, int is_f64) {
    return is_f64 ? ((const double*)p)[at] : (double)((const float*)p)[at];
}

// One block per job; every column statistic is block_sum256's fixed-order tree (cvae_validation.inc).
__global__ __launch_bounds__(256) void k_decode_jobs(const cvae_decode_job* jobs) {
    double* red = (double*)CVAE_SMEM;      // [256]
    const cvae_decode_job& jb = jobs[blockIdx.x];
    const int tid = threadIdx.x, T = jb.T, D = jb.D;
    if (jb.kind == CVAE_DEC_GATHER) {
        const int w = jb.c1 - jb.c0;
        for (long e = tid; e < (long)T * w; e += 256) {
            const long long t = jb.idx[e / w];
            jb.x[e] = t < 0 || t >= jb.src_rows ? nan("") : dec_load(jb.c, t * jb.ldc + jb.c0 + e % w, jb.c_f64);
        }
        return;
    }
    // mod_pow (feature_extract_vc.py:131-138): coefficient 0 moves by log(e_ref / e_c) / 2, the others are copied
    const bool corr = jb.e_ref && jb.e_c;
    for (long e = tid; e < (long)T * D; e += 256) {
        const long t = e / D;
        const int d = (int)(e - t * D);
        double v = dec_load(jb.c, t * jb.ldc + d, jb.c_f64);
        if (d == 0 && corr) {
            const double dp = log(jb.e_ref[t] / jb.e_c[t]) / 2.0;
            v += dp;
            if (jb.dpow) jb.dpow[t] = dp;
        }
        jb.x[e] = v;
        if (jb.diff) jb.diff[e] = v - dec_load(jb.ref, t * jb.ldref + d, jb.ref_f64);
    }
    if (!jb.gv) return;      // (the whole block)
    __syncthreads();
    // decode...:419-422 on x: g = sqrt(gv / cvgv) (x - mean_t x) + mean_t x per column d >= 1, var = np.var(g[:, 1:], 0)
    const double* x = jb.x;
    double* g = jb.g;
    for (int t = tid; t < T; t += 256) g[(long)t * D] = x[(long)t * D];
    for (int d = 1; d < D; ++d) {
        double s = 0.0;
        for (int t = tid; t < T; t += 256) s += x[(long)t * D + d];
        const double m = block_sum256(s, red) / (double)T;
        const double f = sqrt(jb.gv[d - 1] / jb.cvgv[d - 1]);
        double sg = 0.0;
        for (int t = tid; t < T; t += 256) {
            const double v = f * (x[(long)t * D + d] - m) + m;
            g[(long)t * D + d] = v;
            sg += v;
        }
        const double mg = block_sum256(sg, red) / (double)T;
        double q = 0.0;
        for (int t = tid; t < T; t += 256) {
            const double c = g[(long)t * D + d] - mg;      // (this thread's own store)
            q += c * c;
        }
        const double var = block_sum256(q, red) / (double)T;
        if (tid == 0) jb.var[d - 1] = var;
    }
}

inline size_t mc2e_batch_lds(int irlen, int Dmax) { return ((size_t)2 * irlen + Dmax + 64) * sizeof(double); }

}  // namespace

extern "C" {

size_t cvae_mc2e_batch_work_bytes(cvae_ctx* ctx, int n_jobs, int Dmax, int irlen) {
    CVAE_ENTER_SZ(ctx);
    if (n_jobs < 1 || Dmax < 2 || irlen < 2 || irlen > 4000) return 0;
    return (size_t)up256((long long)n_jobs * (long long)sizeof(Mc2eTask)) + (size_t)Dmax * irlen * sizeof(double);
}

int cvae_mc2e_batch(cvae_ctx* ctx, const cvae_mc2e_job* jobs, int n_jobs, double alpha, int irlen, void* work, size_t work_bytes,
                    void* stream) {
    CVAE_ENTER(ctx);
    if (!jobs || !work || n_jobs < 1) return fail(-1, "cvae_mc2e_batch: bad argument (n_jobs=%d)", n_jobs);
    if (irlen < 2 || irlen > 4000) return fail(-1, "cvae_mc2e_batch: irlen=%d outside 2 .. 4000", irlen);
    int Dmax = 0;
    long long frames = 0;
    std::vector<Mc2eTask> tasks((size_t)n_jobs);
    for (int q = 0; q < n_jobs; ++q) {
        const cvae_mc2e_job& j = jobs[q];
        if (!j.mc || !j.e_out || j.T < 1 || j.D < 2 || j.ld < j.D)
            return fail(-1, "cvae_mc2e_batch: bad job %d (T=%d D=%d ld=%lld)", q, j.T, j.D, (long long)j.ld);
        tasks[q].j = j;
        tasks[q].frame0 = frames;
        frames += j.T;
        if (j.D > Dmax) Dmax = j.D;
    }
    if (frames > 0x7fffffffLL) return fail(-1, "cvae_mc2e_batch: %lld frames in one call", frames);
    const size_t lds = mc2e_batch_lds(irlen, Dmax);
    if (lds > 65536) return fail(-1, "cvae_mc2e_batch: irlen=%d with D=%d needs %zu bytes of LDS (64 KiB at most)", irlen, Dmax, lds);
    if (work_bytes < cvae_mc2e_batch_work_bytes(ctx, n_jobs, Dmax, irlen)) return fail(-2, "cvae_mc2e_batch: work buffer too small");
    hipStream_t st = (hipStream_t)stream;
    unsigned char* W = (unsigned char*)work;
    double* F = (double*)(W + up256((long long)n_jobs * (long long)sizeof(Mc2eTask)));
    // (pageable source: the runtime has taken its copy of `tasks` when the call returns)
    CVAE_HIP_OK(hipMemcpyAsync(W, tasks.data(), (size_t)n_jobs * sizeof(Mc2eTask), hipMemcpyHostToDevice, st));
    const int nt = Dmax - 1 >= 256 ? 256 : (Dmax - 1 + 63) / 64 * 64;
    hipLaunchKernelGGL((k_freqt_rows), dim3(1), dim3(nt), (size_t)2 * nt * sizeof(double), st, F, Dmax, irlen, alpha);
    hipLaunchKernelGGL((k_mc2e_batch), dim3((unsigned)frames), dim3(64), lds, st, (const Mc2eTask*)W, n_jobs, (const double*)F, irlen, Dmax);
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

int cvae_decode_jobs(cvae_ctx* ctx, const cvae_decode_job* jobs, int n_jobs, void* work, size_t work_bytes, void* stream) {
    CVAE_ENTER(ctx);
    if (!jobs || !work || n_jobs < 1) return fail(-1, "cvae_decode_jobs: bad argument (n_jobs=%d)", n_jobs);
    if (work_bytes < (size_t)n_jobs * sizeof(cvae_decode_job)) return fail(-2, "cvae_decode_jobs: work buffer too small");
    for (int q = 0; q < n_jobs; ++q) {
        const cvae_decode_job& j = jobs[q];
        bool ok = j.c && j.x && j.T >= 1;
        if (j.kind == CVAE_DEC_GATHER) ok = ok && j.idx && j.c0 >= 0 && j.c0 < j.c1 && j.ldc >= j.c1 && j.src_rows >= 1;
        else if (j.kind == CVAE_DEC_MODPOW)
            ok = ok && j.D >= 2 && j.ldc >= j.D && (!j.gv || (j.cvgv && j.g && j.var)) && (!j.diff || (j.ref && j.ldref >= j.D));
        else ok = false;
        if (!ok) return fail(-1, "cvae_decode_jobs: bad job %d (kind=%d T=%d D=%d)", q, j.kind, j.T, j.D);
    }
    hipStream_t st = (hipStream_t)stream;
    CVAE_HIP_OK(hipMemcpyAsync(work, jobs, (size_t)n_jobs * sizeof(cvae_decode_job), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL((k_decode_jobs), dim3(n_jobs), dim3(256), 256 * sizeof(double), st, (const cvae_decode_job*)work);
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

}  // extern "C"
