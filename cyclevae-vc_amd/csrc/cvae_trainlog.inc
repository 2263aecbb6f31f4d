// The per-window half of the stage-4 training log (train_gru_cyclevae_gauss_batch.py:1312-1316, :1349-1353, :1364-1371, :1431-1439)
// as ONE launch per frame window: the script takes five .item() read-backs and four dtw_c.calc_mcd calls (two index_select(...).cpu()
// copies each) per utterance and cycle, and three .cpu() copies for its GV buffers -- a device synchronisation each.  Here a block
// per (cycle, utterance) forms the nine figures in f64 from the fp32 trajectories and leaves them in a record the host copies
// behind an event; the blocks of cycle 0 also append the window's rows to the utterance-long accumulators.  The per-utterance
// bookkeeping of the generator travels as kernel arguments: no descriptor list, no upload, nothing the host waits for.
namespace {

enum { TLW_THREADS = 256, TLW_LANES = 16 };      // TLW_LANES lanes share a speech frame's row: 64-B pieces of consecutive columns

struct TlwParams {
    const float* traj[CVAE_TRAINLOG_MAX_CYC][5];
    const float* x;                  // batch_src[j0][src_idx_s][0]
    long long ldx, sx;               // its row and utterance strides in floats
    const long long* spc;            // spcidx_src[j0][0]
    long long spc_ld;
    float* acc[4];                   // rows of utterance j0 on; NULL: no copy
    double* out;                     // rec[0][j0][0]
    int B, nb, T, D, L, stdim, s0, acc_rows;      // B: utterances of the trajectories' row stride; nb: of this launch
    int laplace;                     // non-zero: entries [3], [4] are loss_vae_laplace's KL (the caller's L | CVAE_DRAW_LAPLACE)
    int flen_acc[CVAE_TRAINLOG_MAX_UTT], s_idx[CVAE_TRAINLOG_MAX_UTT], e_idx[CVAE_TRAINLOG_MAX_UTT];
    unsigned char sel[CVAE_TRAINLOG_MAX_UTT];
};

// sums of N values over the block's 256 threads, to every thread; fixed-order trees (block_sum256's, N at a time)
template <int N>
__device__ __forceinline__ void block_sums256(double (&v)[N], double* red) {
    const int tid = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < N; ++q) red[q * TLW_THREADS + tid] = v[q];
    __syncthreads();
    for (int w = TLW_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int q = 0; q < N; ++q) red[q * TLW_THREADS + tid] += red[q * TLW_THREADS + tid + w];
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = red[q * TLW_THREADS];
}

// n floats from src to dst, consecutive lanes on consecutive addresses; 16 bytes per lane where both sides allow it
__device__ __forceinline__ void tlw_copy(float* dst, const float* src, long n) {
    const int tid = threadIdx.x;
    if (((((size_t)dst) | ((size_t)src)) & 15) == 0) {
        const long n4 = n >> 2;
        const float4* s4 = (const float4*)src;
        float4* d4 = (float4*)dst;
        for (long e = tid; e < n4; e += TLW_THREADS) d4[e] = s4[e];
        for (long e = (n4 << 2) + tid; e < n; e += TLW_THREADS) dst[e] = src[e];
    } else {
        for (long e = tid; e < n; e += TLW_THREADS) dst[e] = src[e];
    }
}

__global__ __launch_bounds__(TLW_THREADS) void k_trainlog_window(const TlwParams p) {
    double* red = (double*)CVAE_SMEM;     // [5][256]
    const int tid = threadIdx.x, j = blockIdx.x, i = blockIdx.y;
    const int T = p.T, D = p.D, L = p.L;
    const double K = 10.0 / 2.3025850929940456840179914546844;
    const double NaN = nan("");
    const long rowsD = (long)j * T * D, rowsL = (long)j * T * 2 * L;
    const float* lat = p.traj[i][0] + rowsL;
    const float* rec = p.traj[i][1] + rowsD;
    const float* cv = p.traj[i][2] + rowsD;
    const float* latcv = p.traj[i][3] + rowsL;
    const float* cyc = p.traj[i][4] + rowsD;
    const float* x = p.x + (long)j * p.sx + p.stdim;       // the window's target rows, from their first compared column
    double* o = p.out + ((long)i * p.B + j) * 9;
    const bool sel = p.sel[j] != 0;

    // :1312-1316, :1349-1353 -- the window's rows behind the utterance's earlier ones (whole rows; every utterance, selected or not)
    if (i == 0 && p.acc[0]) {
        const long atD = ((long)j * p.acc_rows + p.s0) * D, atL = ((long)j * p.acc_rows + p.s0) * 2 * L;
        tlw_copy(p.acc[0] + atD, rec, (long)T * D);
        tlw_copy(p.acc[1] + atD, cv, (long)T * D);
        tlw_copy(p.acc[2] + atD, cyc, (long)T * D);
        tlw_copy(p.acc[3] + atL, lat, (long)T * 2 * L);
    }

    // :1366-1371 -- means over the utterance's first n frames of the window.  Both are sums over (frame, column), taken element by
    // element in memory order: consecutive lanes read consecutive addresses
    const int n = p.flen_acc[j] < T ? p.flen_acc[j] : T;
    if (sel && n > 0) {                                     // (the whole block takes the same side: j is the block's)
        double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (long e = tid; e < (long)n * D; e += TLW_THREADS) {
            const long t = e / D;
            const double y = (double)x[t * p.ldx + (e - t * D)];
            v[0] += fabs((double)rec[e] - y);
            v[1] += fabs((double)cyc[e] - y);
            v[2] += fabs((double)cv[e] - y);
        }
        if (p.laplace) {      // loss_vae_laplace (gru_vae.py:130-139): sum_l (-s + b exp(-|mu|/b) + |mu| - 1), b = exp(s)
            for (long e = tid; e < (long)n * L; e += TLW_THREADS) {
                const long t = e / L, at = t * 2 * L + (e - t * L);
                const double ma = fabs((double)lat[at]), sg = (double)lat[at + L];
                const double ma2 = fabs((double)latcv[at]), sg2 = (double)latcv[at + L];
                const double b = exp(sg), b2 = exp(sg2);
                v[3] += -sg + b * exp(-ma / b) + ma - 1.0;
                v[4] += -sg2 + b2 * exp(-ma2 / b2) + ma2 - 1.0;
            }
        } else {
            for (long e = tid; e < (long)n * L; e += TLW_THREADS) {
                const long t = e / L, at = t * 2 * L + (e - t * L);
                const double mu = (double)lat[at], sg = (double)lat[at + L];
                const double mu2 = (double)latcv[at], sg2 = (double)latcv[at + L];
                v[3] += exp(sg) + mu * mu - sg - 1.0;
                v[4] += exp(sg2) + mu2 * mu2 - sg2 - 1.0;
            }
        }
        block_sums256<5>(v, red);
        if (tid == 0) {
            const double km = K * 1.4142135623730950488016887242097 / (double)n, kk = p.laplace ? 1.0 : 0.5;
            o[0] = km * v[0];
            o[1] = km * v[1];
            o[2] = km * v[2];
            o[3] = kk * v[3] / (double)n;
            o[4] = kk * v[4] / (double)n;
        }
    } else if (tid == 0) {
        o[0] = o[1] = o[2] = o[3] = o[4] = NaN;
    }

    // :1431-1439 -- calc_mcd on the window's speech frames f_k = spcidx[j][s_idx + k], k <= e_idx - s_idx: the target row is the
    // window's row f_k - src_idx_s, and so is the trajectories'.  TLW_LANES lanes per frame, a lane's columns TLW_LANES apart; one
    // thread adds a frame's partial sums in lane order.  Coefficient 0 is kept apart, so a row is read once for both figures
    const int s_idx = p.s_idx[j], e_idx = p.e_idx[j];
    const long m = (long)e_idx - s_idx + 1;
    if (sel && s_idx >= 0 && m > 0 && e_idx < p.spc_ld) {
        const long long* idx = p.spc + (long)j * p.spc_ld + s_idx;
        const int lane = tid & (TLW_LANES - 1), slot = tid / TLW_LANES;
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        for (long k0 = 0; k0 < m; k0 += TLW_THREADS / TLW_LANES) {
            const long k = k0 + slot;
            double s_rec = 0.0, s_cyc = 0.0, p_rec = 0.0, p_cyc = 0.0;
            long long r = -1;
            if (k < m) r = idx[k] - p.s0;
            const bool ok = r >= 0 && r < T;
            if (ok) {
                const float* xr = x + r * p.ldx;
                const float* a = rec + r * D;
                const float* b = cyc + r * D;
                for (int c = lane; c < D; c += TLW_LANES) {
                    const double y = (double)xr[c];
                    const double da = y - (double)a[c], db = y - (double)b[c];
                    if (c == 0) {
                        p_rec = da * da;
                        p_cyc = db * db;
                    } else {
                        s_rec += da * da;
                        s_cyc += db * db;
                    }
                }
            }
            __syncthreads();
            red[tid] = s_rec;
            red[TLW_THREADS + tid] = s_cyc;
            __syncthreads();
            if (lane == 0 && k < m) {
                if (ok) {
                    double a1 = 0.0, b1 = 0.0;
                    for (int q = 0; q < TLW_LANES; ++q) {
                        a1 += red[tid + q];
                        b1 += red[TLW_THREADS + tid + q];
                    }
                    v[0] += K * sqrt(2.0 * (p_rec + a1));
                    v[1] += K * sqrt(2.0 * a1);
                    v[2] += K * sqrt(2.0 * (p_cyc + b1));
                    v[3] += K * sqrt(2.0 * b1);
                } else {
                    v[0] = v[1] = v[2] = v[3] = NaN;       // a frame outside the window: the four figures, instead of a read there
                }
            }
        }
        block_sums256<4>(v, red);
        if (tid == 0) {
            o[5] = v[0] / (double)m;
            o[6] = v[1] / (double)m;
            o[7] = v[2] / (double)m;
            o[8] = v[3] / (double)m;
        }
    } else if (tid == 0) {
        o[5] = o[6] = o[7] = o[8] = NaN;
    }
}

}  // namespace

extern "C" {

int cvae_trainlog_window(cvae_ctx* ctx, const cvae_trainlog_window_args* a, void* stream) {
    CVAE_ENTER(ctx);
    if (!a || !a->x_win || !a->spcidx || !a->flen_acc || !a->s_idx || !a->e_idx || !a->selected || !a->rec_out)
        return fail(-1, "cvae_trainlog_window: bad argument");
    // L, or L | CVAE_DRAW_LAPLACE: the flag is taken off before anything is checked or addressed with it
    const int L = draw_dim(a->L);
    const bool laplace = draw_laplace(a->L);
    if (a->n_cyc < 1 || a->n_cyc > CVAE_TRAINLOG_MAX_CYC || a->B < 1 || a->T < 1 || a->D < 1 || L < 1 || a->stdim < 0 || a->spc_ld < 1 ||
        a->x_row_stride < (int64_t)a->stdim + a->D)
        return fail(-1, "cvae_trainlog_window: bad shape (n_cyc=%d B=%d T=%d D=%d L=%d stdim=%d)", a->n_cyc, a->B, a->T, a->D, L, a->stdim);
    for (int i = 0; i < a->n_cyc; ++i)
        for (int k = 0; k < 5; ++k)
            if (!a->traj[i][k]) return fail(-1, "cvae_trainlog_window: trajectory %d of cycle %d is NULL", k, i);
    const bool copy = a->acc[0] || a->acc[1] || a->acc[2] || a->acc[3];
    if (copy && !(a->acc[0] && a->acc[1] && a->acc[2] && a->acc[3])) return fail(-1, "cvae_trainlog_window: four accumulators, or none");
    if (copy && (a->src_idx_s < 0 || (int64_t)a->src_idx_s + a->T > (int64_t)a->acc_rows))
        return fail(-1, "cvae_trainlog_window: rows %d .. %d do not fit accumulators of %d rows", a->src_idx_s, a->src_idx_s + a->T - 1,
                    a->acc_rows);
    TlwParams p;
    for (int j0 = 0; j0 < a->B; j0 += CVAE_TRAINLOG_MAX_UTT) {
        const int nb = a->B - j0 < CVAE_TRAINLOG_MAX_UTT ? a->B - j0 : CVAE_TRAINLOG_MAX_UTT;
        memset(&p, 0, sizeof(p));
        for (int i = 0; i < a->n_cyc; ++i)
            for (int k = 0; k < 5; ++k) p.traj[i][k] = a->traj[i][k] + (size_t)j0 * a->T * (k == 0 || k == 3 ? 2 * L : a->D);
        p.x = a->x_win + (size_t)j0 * a->x_utt_stride;
        p.ldx = a->x_row_stride;
        p.sx = a->x_utt_stride;
        p.spc = (const long long*)a->spcidx + (size_t)j0 * a->spc_ld;
        p.spc_ld = a->spc_ld;
        for (int q = 0; q < 4; ++q) p.acc[q] = copy ? a->acc[q] + (size_t)j0 * a->acc_rows * (q == 3 ? 2 * L : a->D) : nullptr;
        p.out = a->rec_out + (size_t)j0 * 9;
        p.B = a->B;
        p.nb = nb;
        p.T = a->T;
        p.D = a->D;
        p.L = L;
        p.laplace = laplace ? 1 : 0;
        p.stdim = a->stdim;
        p.s0 = a->src_idx_s;
        p.acc_rows = a->acc_rows;
        for (int j = 0; j < nb; ++j) {
            p.flen_acc[j] = a->flen_acc[j0 + j];
            p.s_idx[j] = a->s_idx[j0 + j];
            p.e_idx[j] = a->e_idx[j0 + j];
            p.sel[j] = a->selected[j0 + j];
        }
        hipLaunchKernelGGL((k_trainlog_window), dim3(nb, a->n_cyc), dim3(TLW_THREADS), 5 * TLW_THREADS * sizeof(double), (hipStream_t)stream, p);
        CVAE_HIP_OK(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
