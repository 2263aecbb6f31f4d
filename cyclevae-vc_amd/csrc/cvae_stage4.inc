// Stage-4 glue of libcyclevae_hip.so (included by cvae_lib.hip): what sits BETWEEN the GRU_RNN passes of a training step in
// the reference's script -- the reparameterised draw + torch.cat that builds a decoder input (train...:1335-1338 through
// gru_vae.py:85-98), and the per-utterance loss with its gradients (train...:1363-1410 through gru_vae.py:117-123, 525-527) --
// as one launch each instead of a dozen element-wise torch kernels.
namespace {

// out[p*B + b][t] = [ code_p[b][t][:ncode] ; mu + exp(s/2) * eps_p ]   for p < parts (rec || cv stacked along the batch axis)
// laplace: [ code ; mu + exp(s) * u(eps_p) ] with eps_p the uniform of sampling_vae_laplace (cvae_laplace_u, cvae_kernels.h)
struct SampleCatParams {
    const float* lat;          // [B][T][2L]
    const float* code[2];      // [B][T][ncode]
    const float* eps_in[2];    // [B][T][L] or null (Philox: seed, draw[p], global frame, dim)
    uint64_t seed, draw[2], frame0;
    float* out;                // [parts*B][T][ncode + L]
    float* eps_out;            // [parts][B][T][L]: the eps used (the backward needs them)
    int B, T, L, ncode, parts, laplace;
};

__global__ void k_sample_cat(SampleCatParams p) {
    const int W = p.ncode + p.L;
    const long n = (long)p.parts * p.B * p.T * W;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int c = (int)(idx % W);
    const long row = idx / W;                       // (part, b, t)
    const long bt = row % ((long)p.B * p.T);
    const int part = (int)(row / ((long)p.B * p.T));
    if (c < p.ncode) {
        p.out[idx] = p.code[part][bt * p.ncode + c];
        return;
    }
    const int l = c - p.ncode;
    if (p.laplace) {
        const float e = p.eps_in[part] ? p.eps_in[part][bt * p.L + l]
                                       : cvae_laplace_eps(p.seed, p.draw[part], (uint64_t)bt + p.frame0, (uint32_t)l);
        p.eps_out[((long)part * p.B * p.T + bt) * p.L + l] = e;
        p.out[idx] = p.lat[bt * 2 * p.L + l] + expf(p.lat[bt * 2 * p.L + p.L + l]) * cvae_laplace_u(e);
        return;
    }
    const float e = p.eps_in[part] ? p.eps_in[part][bt * p.L + l] : cvae_randn(p.seed, p.draw[part], (uint64_t)bt + p.frame0, (uint32_t)l);
    p.eps_out[((long)part * p.B * p.T + bt) * p.L + l] = e;
    p.out[idx] = p.lat[bt * 2 * p.L + l] + expf(p.lat[bt * 2 * p.L + p.L + l] * 0.5f) * e;
}

// d lat[b][t][l] = sum_p dout[p][b][t][ncode + l];   d lat[b][t][L + l] = sum_p dout[..] * eps_p * 0.5 * exp(s/2)
// laplace: d lat[b][t][L + l] = sum_p dout[..] * u(eps_p) * exp(s)
__global__ void k_sample_cat_bwd(const float* dout, const float* lat, const float* eps, float* dlat, int B, int T, int L, int ncode,
                                 int parts, int laplace) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)B * T * L) return;
    const int l = (int)(idx % L);
    const long bt = idx / L;
    const int W = ncode + L;
    const float sv = lat[bt * 2 * L + L + l];
    const float hs = laplace ? expf(sv) : 0.5f * expf(sv * 0.5f);
    float dm = 0.f, ds = 0.f;
    for (int part = 0; part < parts; ++part) {
        const float g = dout[((long)part * B * T + bt) * W + ncode + l];
        const float e = eps[((long)part * B * T + bt) * L + l];
        dm += g;
        ds += g * (laplace ? cvae_laplace_u(e) : e) * hs;
    }
    dlat[bt * 2 * L + l] = dm;
    dlat[bt * 2 * L + L + l] = ds;
}

// One wave per frame (b, t): the frame's share of the cycle's loss and the gradients of the four trajectories.
//   w[b][t]      = 1/n_j for the first n_j frames of a selected utterance, else 0   (mean over frames, sum over utterances)
//   loss(b,t)    = w * ( K * (|rec - tgt|_1 + |reccyc - tgt|_1) + kl_scale * KL(lat) + latcv_w[b] * KL(latcv) )
//   K = 10/ln10 * sqrt2 (gru_vae.py:525), KL = 0.5 sum (exp(s) + mu^2 - s - 1) (gru_vae.py:123)
//   laplace: KL = sum (-s + b exp(-|mu|/b) + |mu| - 1), b = exp(s) (loss_vae_laplace, gru_vae.py:130-139);
//            d/d mu = sign(mu) (1 - exp(-|mu|/b)) with sign(0) = 0 as torch.abs differentiates, d/d s = -1 + exp(-|mu|/b) (b + |mu|)
struct Stage4LossParams {
    const float *rec, *reccyc, *lat, *latcv;   // reccyc / latcv null: half cycle (train...:283-287)
    const float* x;                            // target = x[b][t][stdim : stdim + D]
    int x_stride, stdim;
    const float* w;                            // [B][T]
    const float* latcv_w;                      // [B]
    float kl_scale;
    int B, T, D, L, laplace;
    float *d_rec, *d_reccyc, *d_lat, *d_latcv;
    float* frame_loss;                         // [B*T]
};

__device__ __forceinline__ float cvae_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += cvae_shfl(v, (int)((threadIdx.x & 63) ^ o));
    return v;
}

// one latent dim's Laplace KL term and its two derivatives
__device__ __forceinline__ float cvae_kl_laplace(float mu, float s, float& dmu, float& dsc) {
    const float b = expf(s), am = fabsf(mu), ex = expf(-am / b);
    dmu = mu > 0.f ? 1.0f - ex : (mu < 0.f ? ex - 1.0f : 0.0f);
    dsc = -1.0f + ex * (b + am);
    return -s + b * ex + am - 1.0f;
}

__global__ __launch_bounds__(64) void k_stage4_loss(Stage4LossParams p) {
    const long bt = blockIdx.x;
    const int b = (int)(bt / p.T), lane = threadIdx.x;
    const float K = (10.0f / 2.3025850929940456840179914546844f) * 1.4142135623730950488016887242097f;
    const float wt = p.w[bt], wc = p.latcv ? p.latcv_w[b] : 0.0f;
    float acc = 0.f;
    for (int d = lane; d < p.D; d += 64) {
        const float tg = p.x[bt * p.x_stride + p.stdim + d];
        const float a = p.rec[bt * p.D + d] - tg;
        acc += K * fabsf(a);
        p.d_rec[bt * p.D + d] = a > 0.f ? K * wt : (a < 0.f ? -K * wt : 0.f);
        if (p.reccyc) {
            const float c = p.reccyc[bt * p.D + d] - tg;
            acc += K * fabsf(c);
            p.d_reccyc[bt * p.D + d] = c > 0.f ? K * wt : (c < 0.f ? -K * wt : 0.f);
        }
    }
    for (int l = lane; l < p.L; l += 64) {
        if (p.laplace) {
            float dmu, dsc;
            acc += p.kl_scale * cvae_kl_laplace(p.lat[bt * 2 * p.L + l], p.lat[bt * 2 * p.L + p.L + l], dmu, dsc);
            p.d_lat[bt * 2 * p.L + l] = wt * p.kl_scale * dmu;
            p.d_lat[bt * 2 * p.L + p.L + l] = wt * p.kl_scale * dsc;
            if (p.latcv) {
                acc += wc * cvae_kl_laplace(p.latcv[bt * 2 * p.L + l], p.latcv[bt * 2 * p.L + p.L + l], dmu, dsc);
                p.d_latcv[bt * 2 * p.L + l] = wt * wc * dmu;
                p.d_latcv[bt * 2 * p.L + p.L + l] = wt * wc * dsc;
            }
            continue;
        }
        {
            const float mu = p.lat[bt * 2 * p.L + l], s = p.lat[bt * 2 * p.L + p.L + l], es = expf(s);
            acc += p.kl_scale * 0.5f * (es + mu * mu - s - 1.0f);
            p.d_lat[bt * 2 * p.L + l] = wt * p.kl_scale * mu;
            p.d_lat[bt * 2 * p.L + p.L + l] = wt * p.kl_scale * 0.5f * (es - 1.0f);
        }
        if (p.latcv) {
            const float mu = p.latcv[bt * 2 * p.L + l], s = p.latcv[bt * 2 * p.L + p.L + l], es = expf(s);
            acc += wc * 0.5f * (es + mu * mu - s - 1.0f);
            p.d_latcv[bt * 2 * p.L + l] = wt * wc * mu;
            p.d_latcv[bt * 2 * p.L + p.L + l] = wt * wc * 0.5f * (es - 1.0f);
        }
    }
    acc = cvae_wave_sum(acc);
    if (lane == 0) p.frame_loss[bt] = wt * acc;
}

// loss[0] (+)= sum of v[0..n) in a fixed order (one block; every run adds the same numbers in the same tree)
__global__ __launch_bounds__(256) void k_sum_fixed(const float* v, long n, float* out, int accumulate) {
    float* sh = (float*)CVAE_SMEM;
    float a = 0.f;
    for (long i = threadIdx.x; i < n; i += 256) a += v[i];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sh[0] + (accumulate ? out[0] : 0.0f);
}

// ---- the script's own per-utterance loss calls as one launch each (gru_vae.py:117-123, :525-533 with twf = None, GV = False, L2 = False) ----
// TWFSEloss L1 branch: mcd_i = K sqrt2 sum_d |x_id - y_id| per frame; out = (sum_i mcd_i, mean, unbiased std); frame[i] = mcd_i is kept
// for the backward.  One block: per-thread partial sums in double, fixed-order tree (deterministic).
__global__ __launch_bounds__(256) void k_mcd_l1(const float* x, long sx, const float* y, long sy, int n, int D, float* frame, float* out) {
    double* sh = (double*)CVAE_SMEM;     // [256]
    const double K = (10.0 / 2.3025850929940456840179914546844) * 1.4142135623730950488016887242097;
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        float s = 0.f;
        for (int d = 0; d < D; ++d) s += fabsf(x[(long)i * sx + d] - y[(long)i * sy + d]);
        const float m = (float)K * s;
        frame[i] = m;
        a += (double)m;
    }
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
        __syncthreads();
    }
    const double sum = sh[0], mean = sum / n;
    __syncthreads();
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double dlt = (double)frame[i] - mean;
        v += dlt * dlt;
    }
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = (float)sum;
        out[1] = (float)mean;
        out[2] = n > 1 ? (float)sqrt(sh[0] / (n - 1)) : __builtin_nanf("");      // (torch.std of one element is nan)
    }
}

// dx[i][d] = K sqrt2 sign(x - y) (g_sum + g_mean / n + g_std (mcd_i - mean) / ((n - 1) std));  g = (g_sum, g_mean, g_std) on the device
__global__ void k_mcd_l1_bwd(const float* x, long sx, const float* y, long sy, int n, int D, const float* frame, const float* out,
                             const float* g, float* dx) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)n * D) return;
    const int i = (int)(idx / D), d = (int)(idx % D);
    const float K = (float)((10.0 / 2.3025850929940456840179914546844) * 1.4142135623730950488016887242097);
    float w = g[0] + g[1] / (float)n;
    if (n > 1 && g[2] != 0.0f) w += g[2] * (frame[i] - out[1]) / ((float)(n - 1) * out[2]);
    const float df = x[(long)i * sx + d] - y[(long)i * sy + d];
    dx[idx] = df > 0.f ? K * w : (df < 0.f ? -K * w : 0.0f);
}

// loss_vae: mean over the T frames of 0.5 sum_l (exp(s) + mu^2 - s - 1), param [T][2L] with row stride sp
__global__ __launch_bounds__(256) void k_kl_gauss(const float* prm, long sp, int T, int L, float* out) {
    double* sh = (double*)CVAE_SMEM;     // [256]
    double a = 0.0;
    for (long e = threadIdx.x; e < (long)T * L; e += 256) {
        const int t = (int)(e / L), l = (int)(e % L);
        const float mu = prm[(long)t * sp + l], sg = prm[(long)t * sp + L + l];
        a += (double)(expf(sg) + mu * mu - sg - 1.0f);
    }
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)(0.5 * sh[0] / T);
}

__global__ void k_kl_gauss_bwd(const float* prm, long sp, int T, int L, const float* g, float* dprm) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)T * 2 * L) return;
    const int t = (int)(idx / (2 * L)), c = (int)(idx % (2 * L));
    const float v = prm[(long)t * sp + c], s = g[0] / (float)T;
    dprm[idx] = c < L ? s * v : s * 0.5f * (expf(v) - 1.0f);
}

}  // namespace

extern "C" {

int cvae_mcd_l1(cvae_ctx* ctx, const float* x, long x_stride, const float* y, long y_stride, int frames, int D, float* frame_mcd, float* out3, void* stream) {
    CVAE_ENTER(ctx);
    if (!x || !y || !frame_mcd || !out3 || frames < 1 || D < 1 || x_stride < D || y_stride < D) return fail(-1, "cvae_mcd_l1: bad argument");
    hipLaunchKernelGGL((k_mcd_l1), dim3(1), dim3(256), 256 * sizeof(double), (hipStream_t)stream, x, x_stride, y, y_stride, frames, D, frame_mcd, out3);
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

int cvae_mcd_l1_backward(cvae_ctx* ctx, const float* x, long x_stride, const float* y, long y_stride, int frames, int D, const float* frame_mcd,
                         const float* out3, const float* g3, float* dx, void* stream) {
    CVAE_ENTER(ctx);
    if (!x || !y || !frame_mcd || !out3 || !g3 || !dx || frames < 1 || D < 1) return fail(-1, "cvae_mcd_l1_backward: bad argument");
    hipLaunchKernelGGL((k_mcd_l1_bwd), dim3(nblk((long)frames * D, 256)), dim3(256), 0, (hipStream_t)stream, x, x_stride, y, y_stride, frames,
                       D, frame_mcd, out3, g3, dx);
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

int cvae_kl_gauss(cvae_ctx* ctx, const float* param, long stride, int frames, int lat_dim, float* out1, void* stream) {
    CVAE_ENTER(ctx);
    if (!param || !out1 || frames < 1 || lat_dim < 1 || stride < 2 * lat_dim) return fail(-1, "cvae_kl_gauss: bad argument");
    hipLaunchKernelGGL((k_kl_gauss), dim3(1), dim3(256), 256 * sizeof(double), (hipStream_t)stream, param, stride, frames, lat_dim, out1);
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

int cvae_kl_gauss_backward(cvae_ctx* ctx, const float* param, long stride, int frames, int lat_dim, const float* g1, float* dparam, void* stream) {
    CVAE_ENTER(ctx);
    if (!param || !g1 || !dparam || frames < 1 || lat_dim < 1) return fail(-1, "cvae_kl_gauss_backward: bad argument");
    hipLaunchKernelGGL((k_kl_gauss_bwd), dim3(nblk((long)frames * 2 * lat_dim, 256)), dim3(256), 0, (hipStream_t)stream, param, stride,
                       frames, lat_dim, g1, dparam);
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

int cvae_sample_cat(cvae_ctx* ctx, const float* lat, const float* code0, const float* code1, const float* eps0, const float* eps1, uint64_t seed,
                    uint64_t draw0, uint64_t draw1, int B, int T, int lat_dim, int ncode, int parts, float* out, float* eps_out,
                    void* stream) {
    CVAE_ENTER(ctx);
    const int laplace = draw_laplace(lat_dim);
    lat_dim = draw_dim(lat_dim);
    if (!lat || !code0 || !out || !eps_out || B < 1 || T < 1 || lat_dim < 1 || ncode < 0 || parts < 1 || parts > 2 ||
        (parts == 2 && !code1))
        return fail(-1, "cvae_sample_cat: bad argument");
    SampleCatParams p;
    p.lat = lat; p.code[0] = code0; p.code[1] = code1; p.eps_in[0] = eps0; p.eps_in[1] = eps1;
    p.seed = seed; p.draw[0] = draw0; p.draw[1] = draw1;
    p.frame0 = (uint64_t)cx().draw_row0 * (uint64_t)T;     // Philox keyed by the GLOBAL frame (cvae_set_draw_origin)
    p.out = out; p.eps_out = eps_out; p.B = B; p.T = T; p.L = lat_dim; p.ncode = ncode; p.parts = parts; p.laplace = laplace;
    const long n = (long)parts * B * T * (ncode + lat_dim);
    hipLaunchKernelGGL((k_sample_cat), dim3(nblk(n, 256)), dim3(256), 0, (hipStream_t)stream, p);
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

int cvae_sample_cat_backward(cvae_ctx* ctx, const float* dout, const float* lat, const float* eps, int B, int T, int lat_dim, int ncode, int parts,
                             float* dlat, void* stream) {
    CVAE_ENTER(ctx);
    const int laplace = draw_laplace(lat_dim);
    lat_dim = draw_dim(lat_dim);
    if (!dout || !lat || !eps || !dlat || B < 1 || T < 1 || lat_dim < 1 || ncode < 0 || parts < 1 || parts > 2)
        return fail(-1, "cvae_sample_cat_backward: bad argument");
    hipLaunchKernelGGL((k_sample_cat_bwd), dim3(nblk((long)B * T * lat_dim, 256)), dim3(256), 0, (hipStream_t)stream, dout, lat, eps, dlat,
                       B, T, lat_dim, ncode, parts, laplace);
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

int cvae_stage4_loss(cvae_ctx* ctx, const float* rec, const float* reccyc, const float* lat, const float* latcv, const float* x, int x_stride, int stdim,
                     const float* w, const float* latcv_w, float kl_scale, int B, int T, int D, int lat_dim, float* d_rec,
                     float* d_reccyc, float* d_lat, float* d_latcv, float* frame_loss, float* loss, int accumulate, void* stream) {
    CVAE_ENTER(ctx);
    const int laplace = draw_laplace(lat_dim);
    lat_dim = draw_dim(lat_dim);
    if (!rec || !lat || !x || !w || !d_rec || !d_lat || !frame_loss || !loss || B < 1 || T < 1 || D < 1 || lat_dim < 1)
        return fail(-1, "cvae_stage4_loss: bad argument");
    if ((reccyc && !d_reccyc) || (latcv && (!d_latcv || !latcv_w))) return fail(-1, "cvae_stage4_loss: missing gradient / weight pointer");
    if (x_stride < stdim + D) return fail(-1, "cvae_stage4_loss: x_stride %d < stdim + D = %d", x_stride, stdim + D);
    Stage4LossParams p;
    p.rec = rec; p.reccyc = reccyc; p.lat = lat; p.latcv = latcv; p.x = x; p.x_stride = x_stride; p.stdim = stdim; p.w = w;
    p.latcv_w = latcv_w; p.kl_scale = kl_scale; p.B = B; p.T = T; p.D = D; p.L = lat_dim; p.laplace = laplace;
    p.d_rec = d_rec; p.d_reccyc = d_reccyc; p.d_lat = d_lat; p.d_latcv = d_latcv; p.frame_loss = frame_loss;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL((k_stage4_loss), dim3((unsigned)((long)B * T)), dim3(64), 0, st, p);
    hipLaunchKernelGGL((k_sum_fixed), dim3(1), dim3(256), 256 * sizeof(float), st, (const float*)frame_loss, (long)B * T, loss, accumulate);
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

}  // extern "C"
