// Stage 5 (calc_cvgv_gru-cyclevae_gauss.py) of libcyclevae_hip.so (included by cvae_lib.hip): the n_draws-draw latent mean
// lat_feat of :180-184 as an array of its own.  The pass prologue (cvae_kernels.h: cvae_input_value / cvae_mean_draws) forms the
// same mean on the way into a decoder pass and never writes it out; stage 5 both decodes it (:194-198) and aligns it (:270-277).
// Its two statistics kinds (CVAE_STAT_MEANSTD64 / CVAE_STAT_MCD64) live in k_eval_stats, cvae_validation.inc.
namespace {

enum { LATMEAN_MAX_JOBS = 32 };      // jobs per launch: one row tile's worth of cells, like CVAE_MAX_CELLS
struct LatMeanParams {
    cvae_latmean_job job[LATMEAN_MAX_JOBS];
    int L, n_draws, laplace;      // laplace: out = mu + exp(s) * mean_k u(eps_k) (CVAE_DRAW_LAPLACE in lat_dim)
    uint64_t seed;
};
static_assert(sizeof(LatMeanParams) <= 4096, "LatMeanParams is a kernel argument: 4 KiB at most");

// grid (blocks, jobs); one thread per (frame, four latent dims) adds that item's draws in the order k = 0, 1, ...: a Philox block
// gives the four normals at once (cvae_randn4), injected eps are read in the same order.  The last quad of a lat_dim that is no
// multiple of 4 draws four and keeps lat_dim - 4 * quad of them.
__global__ __launch_bounds__(256) void k_latent_mean(LatMeanParams p) {
    const cvae_latmean_job& jb = p.job[blockIdx.y];
    const int L = p.L, nq = (L + 3) >> 2;
    const long items = (long)jb.frames * nq;
    const float inv = 1.0f / (float)p.n_draws;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long)gridDim.x * 256) {
        const long t = it / nq;
        const int qd = (int)(it - t * nq), l0 = 4 * qd, w = L - l0 < 4 ? L - l0 : 4;
        float e[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < p.n_draws; ++k) {
            float z[4] = {0.f, 0.f, 0.f, 0.f};
            if (jb.eps) {
                const float* ep = jb.eps + ((long)k * jb.frames + t) * L + l0;
                for (int j = 0; j < w; ++j) z[j] = p.laplace ? cvae_laplace_u(ep[j]) : ep[j];
            } else if (p.laplace) {
                cvae_laplace4(p.seed, jb.draw_id + (uint64_t)k, (uint64_t)t, (uint32_t)qd, z);
            } else {
                cvae_randn4(p.seed, jb.draw_id + (uint64_t)k, (uint64_t)t, (uint32_t)qd, z);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] += z[j];
        }
        const float* row = jb.lat + t * 2 * L;
        for (int j = 0; j < w; ++j) {
            const float s = row[L + l0 + j];
            jb.out[t * L + l0 + j] = row[l0 + j] + expf(p.laplace ? s : s * 0.5f) * (e[j] * inv);
        }
    }
}

}  // namespace

extern "C" {

int cvae_latent_mean(cvae_ctx* ctx, const cvae_latmean_job* jobs, int n_jobs, int lat_dim, int n_draws, uint64_t seed, void* stream) {
    CVAE_ENTER(ctx);
    const int laplace = draw_laplace(lat_dim);
    lat_dim = draw_dim(lat_dim);
    if (!jobs || n_jobs < 1 || lat_dim < 1 || n_draws < 1)
        return fail(-1, "cvae_latent_mean: bad argument (n_jobs=%d lat_dim=%d n_draws=%d)", n_jobs, lat_dim, n_draws);
    for (int q = 0; q < n_jobs; ++q)
        if (!jobs[q].lat || !jobs[q].out || jobs[q].frames < 1) return fail(-1, "cvae_latent_mean: bad job %d (frames=%d)", q, jobs[q].frames);
    const int nq = (lat_dim + 3) >> 2;
    for (int q0 = 0; q0 < n_jobs; q0 += LATMEAN_MAX_JOBS) {
        const int n = n_jobs - q0 < LATMEAN_MAX_JOBS ? n_jobs - q0 : LATMEAN_MAX_JOBS;
        LatMeanParams p;
        memset(&p, 0, sizeof(p));
        long items = 0;
        for (int k = 0; k < n; ++k) {
            p.job[k] = jobs[q0 + k];
            if ((long)p.job[k].frames * nq > items) items = (long)p.job[k].frames * nq;
        }
        p.L = lat_dim;
        p.n_draws = n_draws;
        p.laplace = laplace;
        p.seed = seed;
        const unsigned bx = nblk(items, 256) < 1024u ? nblk(items, 256) : 1024u;      // (grid-stride beyond: 32 jobs already fill the chip)
        hipLaunchKernelGGL((k_latent_mean), dim3(bx, n), dim3(256), 0, (hipStream_t)stream, p);
        CVAE_HIP_OK(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
