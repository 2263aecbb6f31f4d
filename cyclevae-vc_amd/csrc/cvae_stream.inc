// Live streams (stream.py: StreamConverter) of libcyclevae_hip.so (included by cvae_lib.hip): the one data movement a stream step
// needs besides its two passes.
//   cvae_stream_move  a LIST of strided row copies (append pushed frames to the sessions' input buffers, compact input and latent
//                     buffers into their other half, pack the converted frames of all sessions) as ONE launch, whatever the
//                     number of sessions: the job table travels by value in the kernel arguments, as ProParams does.
// A job is at most a few KiB (hop frames of one session), so the launch is latency, not bandwidth: one block column per job, 16-byte
// accesses where a job's rows allow them.
namespace {

#define CVAE_MOVE_MAX_JOBS 96      // per launch: 32 sessions x 3 jobs; more are split over several launches inside the call
struct MoveParams {
    cvae_move_job job[CVAE_MOVE_MAX_JOBS];
    int njobs;
};
static_assert(sizeof(cvae_move_job) == 40, "cvae_move_job is laid out for 96 jobs per launch");
static_assert(sizeof(MoveParams) <= 4096, "MoveParams is a kernel argument: 4 KiB at most");

// every row of the job starts on a 16-byte boundary on both sides: whole float4 columns first, then width % 4 single floats
__host__ __device__ __forceinline__ bool move_rows_aligned(const cvae_move_job& j) {
    return (((uintptr_t)j.dst | (uintptr_t)j.src) & 15) == 0 && ((j.dst_stride | j.src_stride) & 3) == 0;
}

// blockIdx.y = job, the blocks along x stride over its items: item = (row, float4 column | tail float)
__global__ __launch_bounds__(256) void k_stream_move(MoveParams p) {
    const cvae_move_job& j = p.job[blockIdx.y];
    const int w4 = move_rows_aligned(j) ? j.width >> 2 : 0;
    const int per = w4 + (j.width - 4 * w4);
    const long long total = (long long)j.rows * per;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / per;
        const int k = (int)(i - r * per);
        const float* s = j.src + r * j.src_stride;
        float* d = j.dst + r * j.dst_stride;
        if (k < w4) {
            ((float4*)d)[k] = ((const float4*)s)[k];
        } else {
            const int c = 4 * w4 + (k - w4);
            d[c] = s[c];
        }
    }
}

}  // namespace

extern "C" {

int cvae_stream_move(cvae_ctx* ctx, const cvae_move_job* jobs, int njobs, void* stream) {
    CVAE_ENTER(ctx);
    if (njobs < 0 || (njobs > 0 && !jobs)) return fail(-1, "cvae_stream_move: bad argument (njobs=%d)", njobs);
    // everything is checked before anything is enqueued
    for (int q = 0; q < njobs; ++q) {
        const cvae_move_job& j = jobs[q];
        if (j.rows < 0 || j.width < 0 || j.dst_stride < 0 || j.src_stride < 0)
            return fail(-1, "cvae_stream_move: job %d has a negative field (rows=%d width=%d dst_stride=%lld src_stride=%lld)", q, j.rows,
                        j.width, (long long)j.dst_stride, (long long)j.src_stride);
        if (j.width > j.dst_stride || j.width > j.src_stride)
            return fail(-1, "cvae_stream_move: job %d: width %d exceeds a row stride (dst %lld, src %lld)", q, j.width,
                        (long long)j.dst_stride, (long long)j.src_stride);
        if (j.rows == 0) continue;
        if (!j.dst || !j.src) return fail(-1, "cvae_stream_move: job %d has a null pointer with rows=%d", q, j.rows);
        if (j.width == 0) continue;
        const uintptr_t s0 = (uintptr_t)j.src, s1 = s0 + ((uintptr_t)(j.rows - 1) * (uintptr_t)j.src_stride + (uintptr_t)j.width) * sizeof(float);
        const uintptr_t d0 = (uintptr_t)j.dst, d1 = d0 + ((uintptr_t)(j.rows - 1) * (uintptr_t)j.dst_stride + (uintptr_t)j.width) * sizeof(float);
        if (s0 < d1 && d0 < s1)
            return fail(-1, "cvae_stream_move: job %d: source and destination ranges overlap (blocks run in no order)", q);
    }
    hipStream_t st = (hipStream_t)stream;
    for (int q0 = 0; q0 < njobs; q0 += CVAE_MOVE_MAX_JOBS) {
        MoveParams mp;
        memset(&mp, 0, sizeof(mp));
        mp.njobs = njobs - q0 < CVAE_MOVE_MAX_JOBS ? njobs - q0 : CVAE_MOVE_MAX_JOBS;
        long long most = 0;
        for (int q = 0; q < mp.njobs; ++q) {
            const cvae_move_job& j = mp.job[q] = jobs[q0 + q];
            const int w4 = move_rows_aligned(j) ? j.width >> 2 : 0;
            const long long items = (long long)j.rows * (w4 + (j.width - 4 * w4));
            if (items > most) most = items;
        }
        if (most == 0) continue;
        // (a stream step moves a few hundred to a few thousand floats per job: one or two blocks each)
        const long long bx = (most + 1023) / 1024;
        hipLaunchKernelGGL((k_stream_move), dim3((unsigned)(bx < 64 ? bx : 64), (unsigned)mp.njobs), dim3(256), 0, st, mp);
    }
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

}  // extern "C"
