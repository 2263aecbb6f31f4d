// The metric half of the per-epoch validation pass (train_gru_cyclevae_gauss_batch.py:887-1019) in batched form: P alignments per
// call (cvae_dtw_batch) and a list of small f64 reductions per launch (cvae_eval_stats).  One validation batch of 8 utterance
// pairs is 96 alignments and ~250 reductions; through the one-problem entry points of cvae_stage6.inc that is several hundred
// launches and ~100 serial single-block kernels.  Here: one block per problem / job, all of them in flight at once.
namespace {

// k_dtw_cost's expression in k_dtw_cost's summation order (cvae_stage6.inc): the batched costs are its bits
__device__ __forceinline__ double dtw_local_cost(const double* x, const double* y, int D, int mcd) {
    if (mcd != 0) {
        double s = 0.0;
        for (int d = 0; d < D; ++d) s += (x[d] - y[d]) * (x[d] - y[d]);
        return (10.0 / 2.3025850929940456840179914546844) * sqrt(2.0 * s);
    }
    double xy = 0.0, xx = 0.0, yy = 0.0;
    for (int d = 0; d < D; ++d) {
        xy += x[d] * y[d];
        xx += x[d] * x[d];
        yy += y[d] * y[d];
    }
    return 1.0 - xy / (sqrt(xx) * sqrt(yy));
}

// a problem as the kernels see it: the caller's descriptor plus where its pieces of the work buffer are (byte offsets)
struct DtwTask {
    cvae_dtw_problem p;
    long long bp;        // [T1][T2] back-pointer bytes: 0 (i-1,j-1), 1 (i-1,j), 2 (i,j-1), 3 the origin
    long long path;      // [T1+T2] int2 (i, j) of the path points, from the end backwards
    long long pcost;     // [T1+T2] their local costs
    long long diag;      // 3 x [T1] doubles when T1 > CVAE_DTW_LDS_ROWS, else -1 (the rows live in LDS)
    long long cost;      // [T1][T2] doubles (dtw_batch_cost = 1), else -1
};

enum { DTW_THREADS = 256, DTW_COST_BLOCKS = 64 };

// the local costs of every problem of a chunk: grid (DTW_COST_BLOCKS, problems), grid-stride over a problem's cells
__global__ __launch_bounds__(256) void k_dtw_batch_cost(const DtwTask* tasks, unsigned char* work) {
    const DtwTask& t = tasks[blockIdx.y];
    const int T2 = t.p.T2, D = t.p.D, mcd = t.p.mcd;
    const long n = (long)t.p.T1 * T2;
    double* cost = (double*)(work + t.cost);
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256) {
        const int i = (int)(idx / T2), j = (int)(idx % T2);
        cost[idx] = dtw_local_cost(t.p.org + (long)i * t.p.ld_org, t.p.trg + (long)j * t.p.ld_trg, D, mcd);
    }
}

// One block per problem.  Forward: anti-diagonal dg holds the cells (i, dg - i); a row of the rotating triple is indexed by i, so
// (i-1, j) and (i, j-1) are entries i-1 and i of the previous row and (i-1, j-1) is entry i-1 of the one before; one barrier
// per diagonal.  Then thread 0 follows the back-pointers and lists the path, all threads fetch the path's local costs, thread 0
// picks per target frame (the path's points of one j are consecutive) and sums, all threads gather.
template <bool SLAB>
__global__ __launch_bounds__(DTW_THREADS) void k_dtw_batch_path(const DtwTask* tasks, unsigned char* work) {
    const DtwTask& t = tasks[blockIdx.x];
    const int T1 = t.p.T1, T2 = t.p.T2, D = t.p.D, mcd = t.p.mcd, tid = threadIdx.x;
    const double* org = t.p.org;
    const double* trg = t.p.trg;
    const long lo = t.p.ld_org, lt = t.p.ld_trg;
    const double* cost = SLAB ? (const double*)(work + t.cost) : nullptr;
    unsigned char* bp = work + t.bp;
    double* row = t.diag >= 0 ? (double*)(work + t.diag) : (double*)CVAE_SMEM;
    double* cur = row;
    double* prev = row + T1;
    double* prev2 = row + 2 * (long)T1;
    const double INF = 1e300;
    for (int dg = 0; dg < T1 + T2 - 1; ++dg) {
        const int i_lo = dg - (T2 - 1) > 0 ? dg - (T2 - 1) : 0, i_hi = dg < T1 - 1 ? dg : T1 - 1;
        for (int i = i_lo + tid; i <= i_hi; i += DTW_THREADS) {
            const int j = dg - i;
            double best = INF;
            unsigned char code = 3;
            if (i == 0 && j == 0) best = 0.0;
            if (i > 0 && j > 0) { best = prev2[i - 1]; code = 0; }
            if (i > 0 && prev[i - 1] < best) { best = prev[i - 1]; code = 1; }
            if (j > 0 && prev[i] < best) { best = prev[i]; code = 2; }
            const double c = SLAB ? cost[(long)i * T2 + j] : dtw_local_cost(org + (long)i * lo, trg + (long)j * lt, D, mcd);
            cur[i] = c + best;
            bp[(long)i * T2 + j] = code;
        }
        __syncthreads();
        double* r = prev2;
        prev2 = prev;
        prev = cur;
        cur = r;
    }
    int* path = (int*)(work + t.path);
    double* pcost = (double*)(work + t.pcost);
    int* npath = (int*)CVAE_SMEM;      // (the LDS rows are dead: every thread is past the last diagonal's barrier)
    if (tid == 0) {
        int i = T1 - 1, j = T2 - 1, n = 0;
        for (;;) {
            path[2 * n] = i;
            path[2 * n + 1] = j;
            ++n;
            const unsigned char code = bp[(long)i * T2 + j];
            if (code == 3 || n >= T1 + T2) break;      // (n < T1 + T2 always: every step lowers i + j)
            if (code != 2) --i;
            if (code != 1) --j;
        }
        npath[0] = n;
    }
    __syncthreads();
    const int n = npath[0];
    for (int k = tid; k < n; k += DTW_THREADS) {
        const int i = path[2 * k], j = path[2 * k + 1];
        pcost[k] = SLAB ? cost[(long)i * T2 + j] : dtw_local_cost(org + (long)i * lo, trg + (long)j * lt, D, mcd);
    }
    __syncthreads();
    if (tid == 0) {
        // walking backwards with "<=": the smallest i among equal costs wins
        int k = 0;
        for (int j = T2 - 1; j >= 0; --j) {
            double fb = INF;
            long long ib = -1;
            while (k < n && path[2 * k + 1] == j) {
                if (pcost[k] <= fb) {
                    fb = pcost[k];
                    ib = path[2 * k];
                }
                ++k;
            }
            t.p.frames[j] = fb;
            t.p.twf[j] = ib;
        }
        double s = 0.0;
        for (int q = 0; q < T2; ++q) s += t.p.frames[q];
        t.p.mean_out[0] = s / (double)T2;
    }
    if (!t.p.aligned) return;
    __syncthreads();
    for (long idx = tid; idx < (long)T2 * D; idx += DTW_THREADS) {
        const long long i = t.p.twf[idx / D];
        t.p.aligned[idx] = i >= 0 ? org[i * lo + idx % D] : nan("");
    }
}

inline long long up256(long long v) { return (v + 255) / 256 * 256; }

// bytes of work one problem takes behind the task list, and its offsets (relative to `at`)
long long dtw_task_layout(int T1, int T2, bool slab, long long at, DtwTask* t) {
    long long o = at;
    const long long cells = (long long)T1 * T2, pts = (long long)T1 + T2;
    if (t) t->bp = o;
    o = up256(o + cells);
    if (t) t->path = o;
    o = up256(o + pts * 2 * (long long)sizeof(int));
    if (t) t->pcost = o;
    o = up256(o + pts * (long long)sizeof(double));
    if (t) t->diag = T1 > CVAE_DTW_LDS_ROWS ? o : -1;
    if (T1 > CVAE_DTW_LDS_ROWS) o = up256(o + 3LL * T1 * (long long)sizeof(double));
    if (t) t->cost = slab ? o : -1;
    if (slab) o = up256(o + cells * (long long)sizeof(double));
    return o - at;
}

// ---- statistics jobs ----

// sum of v over the block's 256 threads, to every thread; fixed-order tree
__device__ __forceinline__ double block_sum256(double v, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    return red[0];
}

// sum over columns c0 .. c1-1 of (x - y)^2, in column order
__device__ __forceinline__ double sqdist64(const double* x, const double* y, int c0, int c1) {
    double s = 0.0;
    for (int c = c0; c < c1; ++c) s += (x[c] - y[c]) * (x[c] - y[c]);
    return s;
}

__global__ __launch_bounds__(256) void k_eval_stats(const cvae_stat_job* jobs, double* out) {
    double* red = (double*)CVAE_SMEM;     // [256]
    const cvae_stat_job& jb = jobs[blockIdx.x];
    const int tid = threadIdx.x, rows = jb.rows, c0 = jb.c0, c1 = jb.c1, kind = jb.kind;
    const long lda = jb.lda, ldb = jb.ldb;
    const double K = 10.0 / 2.3025850929940456840179914546844;
    const double NaN = nan("");
    double* o = out + jb.out_off;
    if (kind == CVAE_STAT_GV) {
        const float* a = (const float*)jb.a;
        for (int c = c0; c < c1; ++c) {
            double s = 0.0;
            for (int r = tid; r < rows; r += 256) s += (double)a[(long)r * lda + c];
            const double m = block_sum256(s, red) / (double)rows;
            double q = 0.0;
            for (int r = tid; r < rows; r += 256) {
                const double d = (double)a[(long)r * lda + c] - m;
                q += d * d;
            }
            const double v = block_sum256(q, red) / (double)rows;
            if (tid == 0) o[c - c0] = v;
        }
    } else if (kind == CVAE_STAT_MCD_SPC) {
        const float* a = (const float*)jb.a;
        const float* b = (const float*)jb.b;
        double acc = 0.0;
        for (int k = tid; k < rows; k += 256) {
            const long long t = jb.idx[k];
            if (t < 0 || t >= jb.src_rows) {
                acc = NaN;
                continue;
            }
            double s = 0.0;
            for (int c = c0; c < c1; ++c) {
                const double e = (double)a[t * lda + c] - (double)b[t * ldb + c];
                s += e * e;
            }
            acc += K * sqrt(2.0 * s);
        }
        const double tot = block_sum256(acc, red);
        if (tid == 0) o[0] = tot / (double)rows;
    } else if (kind == CVAE_STAT_MCD_L1) {
        const float* a = (const float*)jb.a;
        const float* b = (const float*)jb.b;
        double acc = 0.0;
        for (int t = tid; t < rows; t += 256) {
            double s = 0.0;
            for (int c = 0; c < c1; ++c) s += fabs((double)a[(long)t * lda + c] - (double)b[(long)t * ldb + c]);
            acc += K * 1.4142135623730950488016887242097 * s;
        }
        const double tot = block_sum256(acc, red);
        if (tid == 0) o[0] = tot / (double)rows;
    } else if (kind == CVAE_STAT_KL) {
        const float* a = (const float*)jb.a;
        double acc = 0.0;
        for (int t = tid; t < rows; t += 256) {
            double s = 0.0;
            for (int l = 0; l < c1; ++l) {
                const double mu = (double)a[(long)t * lda + l], sg = (double)a[(long)t * lda + c1 + l];
                s += exp(sg) + mu * mu - sg - 1.0;
            }
            acc += 0.5 * s;
        }
        const double tot = block_sum256(acc, red);
        if (tid == 0) o[0] = tot / (double)rows;
    } else if (kind == CVAE_STAT_KL_LAPLACE) {
        // loss_vae_laplace (gru_vae.py:130-139) in CVAE_STAT_KL's summation order: a[t] = [mu | log-scale], b = exp(s)
        const float* a = (const float*)jb.a;
        double acc = 0.0;
        for (int t = tid; t < rows; t += 256) {
            double s = 0.0;
            for (int l = 0; l < c1; ++l) {
                const double ma = fabs((double)a[(long)t * lda + l]), sg = (double)a[(long)t * lda + c1 + l];
                const double b = exp(sg);
                s += -sg + b * exp(-ma / b) + ma - 1.0;
            }
            acc += s;
        }
        const double tot = block_sum256(acc, red);
        if (tid == 0) o[0] = tot / (double)rows;
    } else if (kind == CVAE_STAT_GATHER64) {
        const float* a = (const float*)jb.a;
        const int w = c1 - c0;
        for (long e = tid; e < (long)rows * w; e += 256) {
            const long long t = jb.idx[e / w];
            jb.dst[e] = t < 0 || t >= jb.src_rows ? NaN : (double)a[t * lda + c0 + e % w];
        }
    } else if (kind == CVAE_STAT_LATDIST) {
        const double* a = (const double*)jb.a;
        const double* b = (const double*)jb.b;
        // one thread per column, rows in order; then the columns in order
        double acc = 0.0;
        for (int c = tid; c < c1; c += 256) {
            double s = 0.0;
            for (int t = 0; t < rows; ++t) {
                const double e = a[(long)t * lda + c] - b[(long)t * ldb + c];
                s += e * e;
            }
            acc += sqrt(s / (double)rows);
        }
        const double tot = block_sum256(acc, red);
        if (tid == 0) o[0] = tot / (double)c1;
    } else if (kind == CVAE_STAT_MEANSTD64 || kind == CVAE_STAT_MCD64) {
        // mean and population standard deviation of a per-frame array (stage 5): np.std's two passes
        const double* a = (const double*)jb.a;
        const double* b = (const double*)jb.b;
        const bool mcd = kind == CVAE_STAT_MCD64;
        if (rows < 1 || rows > jb.src_rows) {      // (the whole block: nobody reaches a barrier)
            if (tid == 0) o[0] = o[1] = NaN;
            return;
        }
        double s = 0.0;
        for (int t = tid; t < rows; t += 256) s += mcd ? K * sqrt(2.0 * sqdist64(a + t * lda, b + t * ldb, c0, c1)) : a[t * lda];
        const double m = block_sum256(s, red) / (double)rows;
        double q = 0.0;
        for (int t = tid; t < rows; t += 256) {
            const double d = (mcd ? K * sqrt(2.0 * sqdist64(a + t * lda, b + t * ldb, c0, c1)) : a[t * lda]) - m;
            q += d * d;
        }
        const double v = block_sum256(q, red) / (double)rows;
        if (tid == 0) {
            o[0] = m;
            o[1] = sqrt(v);
        }
    } else if (tid == 0) {
        o[0] = NaN;
    }
}

}  // namespace

extern "C" {

size_t cvae_dtw_batch_work_bytes(cvae_ctx* ctx, int P, int T1max, int T2max) {
    CVAE_ENTER_SZ(ctx);
    if (P < 1 || T1max < 1 || T2max < 1) return 0;
    const bool slab = opt(OPT_DTW_BATCH_COST) != 0;
    const long long one = up256((long long)sizeof(DtwTask)) + dtw_task_layout(T1max, T2max, slab, 0, nullptr);
    const long long all = up256((long long)P * (long long)sizeof(DtwTask)) + (long long)P * dtw_task_layout(T1max, T2max, slab, 0, nullptr);
    const long long cap = (long long)CVAE_DTW_BATCH_WORK_CAP;
    return (size_t)(all <= cap ? all : (one > cap ? one : cap));
}

int cvae_dtw_batch(cvae_ctx* ctx, const cvae_dtw_problem* probs, int P, void* work, size_t work_bytes, void* stream) {
    CVAE_ENTER(ctx);
    if (!probs || !work || P < 1) return fail(-1, "cvae_dtw_batch: bad argument");
    for (int q = 0; q < P; ++q) {
        const cvae_dtw_problem& p = probs[q];
        if (!p.org || !p.trg || !p.twf || !p.frames || !p.mean_out || p.T1 < 1 || p.T2 < 1 || p.D < 1 || p.ld_org < p.D || p.ld_trg < p.D)
            return fail(-1, "cvae_dtw_batch: bad problem %d (T1=%d T2=%d D=%d)", q, p.T1, p.T2, p.D);
    }
    const bool slab = opt(OPT_DTW_BATCH_COST) != 0;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* W = (unsigned char*)work;
    std::vector<DtwTask> tasks;
    int q0 = 0;
    while (q0 < P) {
        // the longest run of problems from q0 whose task list and pieces fit the buffer
        int q1 = q0;
        long long used = 0;
        while (q1 < P) {
            const long long need = dtw_task_layout(probs[q1].T1, probs[q1].T2, slab, 0, nullptr);
            if (up256((long long)(q1 + 1 - q0) * (long long)sizeof(DtwTask)) + used + need > (long long)work_bytes) break;
            used += need;
            ++q1;
        }
        if (q1 == q0) return fail(-2, "cvae_dtw_batch: work buffer too small for problem %d (T1=%d T2=%d)", q0, probs[q0].T1, probs[q0].T2);
        const int n = q1 - q0;
        tasks.resize(n);
        long long at = up256((long long)n * (long long)sizeof(DtwTask));
        size_t lds = sizeof(int);
        for (int k = 0; k < n; ++k) {
            tasks[k].p = probs[q0 + k];
            at += dtw_task_layout(tasks[k].p.T1, tasks[k].p.T2, slab, at, &tasks[k]);
            if (tasks[k].diag < 0 && 3 * (size_t)tasks[k].p.T1 * sizeof(double) > lds) lds = 3 * (size_t)tasks[k].p.T1 * sizeof(double);
        }
        // (pageable source: the runtime has taken its copy of `tasks` when the call returns, so the vector may be reused for the next chunk)
        CVAE_HIP_OK(hipMemcpyAsync(W, tasks.data(), (size_t)n * sizeof(DtwTask), hipMemcpyHostToDevice, st));
        if (slab) {
            hipLaunchKernelGGL((k_dtw_batch_cost), dim3(DTW_COST_BLOCKS, n), dim3(256), 0, st, (const DtwTask*)W, W);
            hipLaunchKernelGGL((k_dtw_batch_path<true>), dim3(n), dim3(DTW_THREADS), lds, st, (const DtwTask*)W, W);
        } else {
            hipLaunchKernelGGL((k_dtw_batch_path<false>), dim3(n), dim3(DTW_THREADS), lds, st, (const DtwTask*)W, W);
        }
        CVAE_HIP_OK(hipGetLastError());
        q0 = q1;
    }
    return 0;
}

int cvae_eval_stats(cvae_ctx* ctx, const cvae_stat_job* jobs, int n, double* out, void* stream) {
    CVAE_ENTER(ctx);
    if (!jobs || !out || n < 1) return fail(-1, "cvae_eval_stats: bad argument");
    hipLaunchKernelGGL((k_eval_stats), dim3(n), dim3(256), 256 * sizeof(double), (hipStream_t)stream, jobs, out);
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

}  // extern "C"
