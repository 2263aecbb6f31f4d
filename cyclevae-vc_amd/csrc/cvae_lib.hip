// libcyclevae_hip.so -- C ABI (include/cyclevae_hip.h) over the kernels in cvae_kernels.h.
// Host orchestration only: carves the caller's buffers, enqueues kernels on the caller's stream.
#include <cvae_intrin.h>

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <map>
#include <mutex>
#include <new>
#include <utility>
#include <vector>

#include "cvae_kernels.h"
#include "cvae_train_kernels.h"
#include "cvae_deep.h"
#include "cyclevae_hip.h"

namespace {

thread_local char g_err[512] = "";
// The library keeps NO process-wide mutable state (ABI 6): what used to be process-wide settings -- where a timed-out hand-off spin is
// reported, this rank's place in a data-parallel job's batch for the Philox streams, the named options, the side stream and its
// events, the profiling brackets, the record of which MFMA-order images a train image holds -- lives in the caller's cvae_ctx
// (cvae_ctx_create: one per (device, stream) user; not thread-safe per handle, independent across handles).  Every entry point
// takes the handle and installs it for the duration of the call (tl_ctx below, thread-local plumbing: never read outside a call).

// Tuning / diagnostic switches (cvae_set_option): the library reads NO environment variable.
enum OptId {
    OPT_V6_LIMBS_H64, OPT_NO_LL, OPT_MAX_RT, OPT_LL_BACKOFF, OPT_EXP, OPT_GEMM_FORCE, OPT_GEMM_LOG, OPT_TRAIN_OLD_GEMM,
    OPT_GEMM_TRACE, OPT_TRAIN_PER_STEP, OPT_TRAIN_PROF, OPT_TRAIN_BACKOFF, OPT_TRAIN_FP32_MFMA, OPT_TRAIN_BWD_PER_STEP, OPT_TRAIN_KERNEL, OPT_X3_TILE, OPT_BWD_OVERFLOW_AT, OPT_GEMM_MAX_SPLIT, OPT_BWD_KS, OPT_COOP_LAUNCH, OPT_V6_LIMBS_H2048, OPT_V6_W2S_H64, OPT_STEP_COL_TILES, OPT_TRAIN_PROFILE, OPT_TRAIN_XMAP, OPT_MASKS_ON_SIDE, OPT_V6_BACKOFF, OPT_TRAIN_BWD_BACKOFF, OPT_LL_ROW_PAD, OPT_GEMM_MIN_DEPTH, OPT_TRAIN_BWD_GEOM, OPT_BWD_W3_L1_H64, OPT_TRAIN_FWD_GEOM, OPT_TRAIN_FWD_BACKOFF, OPT_EXACT_RANGE_AT, OPT_DTW_BATCH_COST, OPT_V6_SKIP_T0, OPT_COUNT
};
struct OptEntry { const char* name; long dflt; };
const OptEntry g_opt[OPT_COUNT] = {      // names and DEFAULTS (immutable); the values live in the context
    {"v6_limbs_h64", 3},          // 2: the two-limb code path of k_gru_steps_v6 at H = 64 (what runs at H = 2048), for the emulator tests
    {"no_ll", 0},                 // 1: passes of <= 3 rows take the dataflow kernel instead of k_gru_steps_ll
    {"max_rt", 0},                // > 0: cap on the row tiles handled concurrently (tests: several row tiles per block on small problems)
    {"ll_backoff", -1},          // >= 0: s_sleep units before the first poll of a step in k_gru_steps_ll (-1: the swept default)
    {"exp", 0},                   // measurement switches of the dataflow kernels (Step6Params::exp)
    {"gemm_force", 0},            // measurement: TM*10000 + TN*100 + ks forces the tile / split of every training GEMM
    {"gemm_log", 0},              // measurement: every training GEMM bracketed by HIP events and printed to stderr
    {"train_old_gemm", 0},        // 1: the simple GEMM kernels kept as unaligned-operand fallbacks, everywhere
    {"gemm_trace", 0},            // 1: print when a GEMM takes a fallback kernel
    {"train_per_step", 0},        // 1: forward training recurrence as T launches
    {"train_prof", 0},            // 1: phase cycle sums of block 0 of the training recurrences (cvae_train_debug_counters)
    {"train_backoff", 32},       // s_sleep units before the first poll of a step, pair-form forward training recurrence
    {"train_fp32_mfma", 0},       // 1: forward training recurrence on v_mfma_f32_16x16x4_f32
    {"train_bwd_per_step", 0},    // 1: reverse training recurrence as 2T launches (fp32 products)
    {"train_kernel", 0},          // training recurrences: 0 exact fp32 operands (fp16 triples), non-zero fp16 pairs (fp32-input MFMA: train_fp32_mfma)
    {"x3_tile", 0},               // exact-operand forward training recurrence: 0 pick by tiles per block, 16 / 32 force that row tile
    {"bwd_overflow_at", 60000},   // |gate gradient * 2^8| that raises status 5 in the persistent reverse recurrences (tests lower it)
    {"gemm_max_split", 16},      // cap on the contraction split of the training GEMMs (1: never split)
    {"bwd_ks", 8},                // K slices of the per-step backward product k_bwd_step_gemm (1..32)
    {"coop_launch", 0},           // 1: the all-resident recurrent kernels go through hipLaunchCooperativeKernel (cvae_launch_coop)
    {"v6_limbs_h2048", 3},        // 2: k_gru_steps_v6 at H = 2048 on fp16 PAIRS (faster, 22-23 bit operands) instead of exact triples
    {"v6_w2s_h64", 0},            // 1: the streamed-third-limb form of k_gru_steps_v6 (what runs at H = 2048) at H = 64, for the emulator tests
    {"step_col_tiles", 0},        // per-step forward training kernel: 0 pick (two 16-column tiles per block when every CU still gets a block), 1 / 2 force
    {"train_profile", 0},         // 1: HIP events around the training recurrences and GEMMs, summed per class (cvae_train_profile_collect)
    {"train_xmap", 0},            // bit 0 / 1: XCD-aware block placement in the exact forward / reverse training recurrences
    {"masks_on_side", 1},         // train-mode forward with a side stream set: the recurrence's dropout mask is drawn on it, beside the front-end GEMMs (0: on the launch stream)
    {"v6_backoff", -1},           // >= 0: x 64 cycles before the first flag poll of a step in k_gru_steps_v6 blocks with one row tile (-1: swept per front-end width)
    {"train_bwd_backoff", -1},    // x 64 cycles before the first flag poll of a task of the exact reverse training recurrences; -1: 32 when a block has ONE tile (B = 8: reverse recurrences 5.3 -> 4.35 ms per step, round 6), 0 with two or more (swept in round 5: slower)
    {"ll_row_pad", 0},            // rows per frame of the time-major buffers of a word-exchange training pass (<= 3 rows): 0 = exactly B (every GEMM of a one-utterance pass over T rows; round 5: 5.28 -> 4.87 ms per step), 4 = round 4's layout
    {"gemm_min_depth", 128},      // a split contraction keeps at least this many k per slice (256 until round 5: one utterance 4.86 -> 4.76 ms)
    {"train_bwd_geom", -1},       // exact reverse training recurrence: 1 = 16 units x 16-row tiles, zero rows of [W_hh^T | F^T] dropped (k_train_bwd_steps_w3, round 6), 0 = 8 units x 16-row tiles (k_train_bwd_steps_x3); -1: the 16-unit form for passes of at least four 16-row tiles (two tiles per block: 128 rows at hu1024 29.0K instead of 2 x 23.3K cycles per step; 64 rows on half the chip, two tiles per block), else the 8-unit form (ONE tile per 16-unit block leaves the hand-off exposed: 22.1K vs 23.2K cycles per 64 rows alone, and no room for a co-resident GEMM)
    {"bwd_w3_l1_h64", 0},         // 1: k_train_bwd_steps_w3 at H = 64 keeps the second limbs of two fragments per wave in LDS (what runs at H = 1024), for the emulator tests
    {"train_fwd_geom", -1},       // exact forward training recurrence: 1 = 16 units x 16-row tiles with the zero column tiles of [W_hh | F] dropped (k_train_fwd_steps_w3, round 6), 0 = the 8-unit kernels (k_train_fwd_steps_x3 / x3h); -1: the 16-unit form for passes of at least four 16-row tiles (64 rows: one tile per block behind a first-poll back-off, 128 rows: two tiles per block), else the 8-unit form
    {"train_fwd_backoff", -1},    // x 64 cycles before the first flag poll of a task of the exact forward training recurrences (16-row-tile kernels); -1: 24 when a block has ONE tile (nothing else covers the hand-off and early polls slow the publishes they wait for), 0 with two or more
    {"exact_range_at", 65504},    // |x| from which an exchanged value (normalised input, carried-in state) of the limb-operand eval kernels raises CVAE_STATUS_RANGE: 65504 = the first limb overflows; 2048 = the third limb (a bf8 byte) stops being exact
    {"dtw_batch_cost", 1},        // cvae_dtw_batch: 1 = local costs of a chunk written first by one grid-wide kernel (f64 slab per problem), 0 = computed cell by cell inside the path kernel; same bits (profiles/validation_notes.md)
    {"v6_skip_t0", 1},            // k_gru_steps_v6 in a pass no cell of which carries a state in: 1 = the tasks of frame 0 leave out the recurrent product of the all-zero slot 0 (no operand request, no MFMA; same bits), 0 = they run it (profiles/v6_launch_ramp_notes.md)
};

// hipEvent pairs recorded around the recurrent kernel when CVAE_FLAG_PROFILE is set
struct ProfEvents {
    std::vector<hipEvent_t> start, stop;
    std::vector<int> rows, cin;      // of the bracketed launch: stacked batch rows and input channels (which instantiation / geometry)
    size_t used = 0;
};
// the same for the training step, per kernel class (option train_profile; cvae_train_profile_collect): 0 forward recurrence,
// 1 reverse recurrence, 2 forward / data-gradient GEMMs (gemm_nt), 3 weight-gradient contractions (gemm_tn)
enum { TPROF_FWD = 0, TPROF_BWD = 1, TPROF_GEMM = 2, TPROF_WGRAD = 3, TPROF_CLASSES = 4 };
struct TrainProfEvents {
    std::vector<hipEvent_t> start, stop;
    std::vector<int> cls;
    std::vector<double> flop;
    size_t used = 0;
};
struct SideDone { const void* scratch; hipEvent_t ev; };

}  // namespace

// The handle behind every entry point (include/cyclevae_hip.h: cvae_ctx_create / cvae_ctx_destroy).
struct cvae_ctx {
    int32_t* status_sink = nullptr;                                  // cvae_set_status_sink
    long draw_row0 = 0, draw_rows = 0, draw_frames = 0, draw_parts = 1;   // cvae_set_draw_origin / cvae_set_draw_parts
    long opt[OPT_COUNT];                                             // cvae_set_option
    ProfEvents prof;
    TrainProfEvents tprof;
    hipStream_t side = nullptr;                                      // cvae_set_side_stream
    SideDone side_done[8] = {};
    hipEvent_t side_ready = nullptr, side_join = nullptr, side_last = nullptr;   // side_last: behind ALL side work enqueued so far
    int side_cap = 0;                                                // tile cap of the side-stream GEMMs being launched (launch_wgrad_side)
    hipEvent_t mask_fork = nullptr, mask_join = nullptr;                         // train-mode forward: the feedback mask drawn on the side stream
    unsigned side_evict = 0;
    int32_t* gemm_ran = nullptr;                                     // cvae_selftest_gemm: where the GEMM wrappers report what they launched
    // which MFMA-order weight images a train image of THIS context holds (cvae_net_prepare_train_v), by address; an address the
    // context has not prepared holds none (the old process-wide registry assumed "all" for unknown addresses and grew
    // without bound); the oldest entries go when the table is full
    std::map<const void*, std::pair<int, unsigned long>> train_var;
    unsigned long train_var_tick = 0;
    // Range guard of the eval passes: images cvae_net_prepared_in_range found unfit for the limb kernels (by address; their passes
    // run the fp32-operand kernels), and the serial number an entry point's passes raise workspace word 20 with (ProParams)
    std::map<const void*, bool> image_unfit;
    int range_serial = 0;
    std::atomic<unsigned> ll_train_launch{1u};                       // tag nonce of the word-exchange training kernels (cvae_train_ll.h)
};

namespace {

thread_local cvae_ctx* tl_ctx = nullptr;       // the context of the entry point running on this thread (installed by CVAE_ENTER)
inline cvae_ctx& cx() { return *tl_ctx; }
inline long opt(OptId i) { return tl_ctx->opt[i]; }
struct CtxScope {
    cvae_ctx* prev;
    explicit CtxScope(cvae_ctx* c) : prev(tl_ctx) {
        tl_ctx = c;
        g_cvae_coop_launch = (int)c->opt[OPT_COOP_LAUNCH];
    }
    ~CtxScope() { tl_ctx = prev; }
};

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// first statement of every entry point that takes the handle
#define CVAE_ENTER(c)                                                          \
    if (!(c)) return fail(-1, "null context (cvae_ctx_create)");               \
    CtxScope cvae_scope_(c)
#define CVAE_ENTER_SZ(c)                                                       \
    if (!(c)) {                                                                \
        (void)fail(-1, "null context (cvae_ctx_create)");                      \
        return 0;                                                              \
    }                                                                          \
    CtxScope cvae_scope_(c)

#define CVAE_HIP_OK(expr)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return fail(-3, "%s failed: %s", #expr, hipGetErrorString(e_));     \
    } while (0)

inline long up(long x, long m) { return (x + m - 1) / m * m; }
// clamp_lat_dim argument of the passes: -1 none; L: out[..., L:] >= ln(1e-6) (clamp_vae, gru_vae.py:412); L | CVAE_CLAMP_LAPLACE: the
// log-scale floor of the Laplace variant (clamp_vae_laplace, gru_vae.py:417)
inline int clamp_dim(int v) { return v < 0 ? -1 : (v & ~CVAE_CLAMP_LAPLACE); }
inline float clamp_floor(int v) { return v >= 0 && (v & CVAE_CLAMP_LAPLACE) ? -7.2543288692621097f : -13.815510557964274f; }
// lat_dim argument of the draws and of the stage-4 loss: L, or L | CVAE_DRAW_LAPLACE for the Laplace posterior (sampling_vae_laplace /
// loss_vae_laplace, gru_vae.py:101-112, :130-139)
inline int draw_dim(int v) { return v < 0 ? v : (v & ~CVAE_DRAW_LAPLACE); }
inline bool draw_laplace(int v) { return v >= 0 && (v & CVAE_DRAW_LAPLACE) != 0; }
inline unsigned nblk(long n, int per) { return (unsigned)((n + per - 1) / per); }

struct Dims {
    int C, Cp, Co, Cop, H, H3, ks, layers, R, pad, cl[3], cw, tot, Kfe, nch, KFW;      // cl[i] = ks^(i+1) * C: output channels of conv i; cw = the last of them (what W_ih sees)
};

int make_dims(const cvae_net_desc* d, Dims* o) {
    if (!d) return fail(-1, "null net descriptor");
    if (d->layers < 1 || d->layers > 3) return fail(-1, "layers (reference dilation_size) must be 1, 2 or 3, got %d", d->layers);
    if (d->kernel_size < 1 || d->kernel_size % 2 == 0) return fail(-1, "kernel_size must be odd, got %d", d->kernel_size);
    if (d->hidden < 16 || d->hidden % 16) return fail(-1, "hidden must be a positive multiple of 16, got %d", d->hidden);
    if (d->in_dim < 1 || d->out_dim < 1) return fail(-1, "bad in_dim/out_dim %d/%d", d->in_dim, d->out_dim);
    if (d->layers == 3 && d->kernel_size != 3)
        return fail(-1, "layers == 3 needs kernel_size == 3: a front-end of kernel_size^3 >= 125 frames is not supported, got kernel_size %d",
                    d->kernel_size);
    // Depth 3 is taken where the recurrences it was built for exist (k_gru_steps_ll and the hoisted exact-operand kernel want
    // H % 64 == 0).  Narrower three-layer networks stay refused, as before ABI 10: tests/test_emu_library.py pins the refusal of
    // (hidden 32, layers 3), and lifting it belongs with a change that may touch that test.
    if (d->layers == 3 && d->hidden % 64)
        return fail(-1, "layers == 3 needs hidden to be a multiple of 64, got %d", d->hidden);
    o->C = d->in_dim;
    o->Cp = (int)up(d->in_dim, 8);   // multiple of 8: eight consecutive fp16 halves of a window are one 16-byte MFMA operand
    o->Co = d->out_dim;
    o->Cop = (int)up(d->out_dim, 16);
    o->H = d->hidden;
    o->H3 = 3 * d->hidden;
    o->ks = d->kernel_size;
    o->layers = d->layers;
    o->R = 1;
    o->cl[0] = o->cl[1] = o->cl[2] = 0;
    for (int i = 0; i < o->layers; ++i) {
        o->R *= o->ks;
        o->cl[i] = o->R * o->C;
    }
    o->pad = (o->R - 1) / 2;
    o->cw = o->R * o->C;
    o->tot = o->cw + o->Co;
    o->Kfe = (int)up((long)o->R * o->Cp, 16);
    o->nch = o->H / 16;
    o->KFW = (o->Kfe / 16 + 3) / 4;   // front-end 16-k chunks per wave in the fused recurrent kernel
    return 0;
}

// the training and backward entry points: their tape, segmented-row GEMMs and gradient chains are written for two conv layers
int make_train_dims(const cvae_net_desc* d, Dims* o) {
    if (int rc = make_dims(d, o)) return rc;
    if (o->layers != 2)
        return fail(-1, "training is implemented for layers (reference dilation_size) == 2 only, got %d (eval and conversion run 1..3)", o->layers);
    return 0;
}

// Scratch of cvae_net_prepare (doubles): the fold walks the conv layers M_0 -> M_1 -> .., each from the one before, so two areas
// alternate -- `a` holds M_{layers-1} (the final one, and M_{layers-3}), `b` M_{layers-2} -- and likewise the bias folds b'_n.
struct FoldScratch { long ma, mb, ba, bb, total; };
inline long fold_m_size(const Dims& m, int n) { return (long)m.cl[n] * (m.cl[n] / m.C) * m.C; }      // M_n [cl[n]][ks^(n+1)][C]
inline FoldScratch fold_scratch(const Dims& m) {
    FoldScratch f;
    f.ma = 0;
    f.mb = fold_m_size(m, m.layers - 1);
    f.ba = f.mb + (m.layers > 1 ? fold_m_size(m, m.layers - 2) : 0);
    f.bb = f.ba + m.cw;
    f.total = f.bb + (m.layers > 1 ? m.cl[m.layers - 2] : 0) + 64;
    return f;
}

// ---- Kernel instances of the eval recurrences: what is built, by geometry.  The layouts (is there a limb image to lay out?), the
// plan (plan_eval_pass) and the launches all look up THESE tables; a geometry without a row has no such kernel.
//
// k_gru_steps_v6 (exact fp32 operands): H = 1024 (16 16-k steps per wave, three limbs), H = 2048 (32 steps: three limbs with the
// third weight limb streamed from L2, or fp16 PAIRS, option v6_limbs_h2048 -- the hu2048 stress configuration, BASELINE configs[4])
// and H = 64 (one step; every form, picked by the options v6_limbs_h64 / v6_w2s_h64: tests at a size the host-fiber emulator runs)
// (fn_prof: the same instance with the phase counters of cvae_step_timing compiled in -- what a CVAE_FLAG_STEP_TIMING pass launches; the
// streamed-third-limb forms have none)
struct V6Inst { int H, KFW, limbs; bool w2s; void (*fn)(Step6Params); void (*fn_prof)(Step6Params); };
#define V6_PAIR(KPW, KFW, LIMBS) k_gru_steps_v6<KPW, KFW, LIMBS>, k_gru_steps_v6<KPW, KFW, LIMBS, false, true>      // resident weights: plain, profiling
#define V6_W2S(KPW, KFW) k_gru_steps_v6<KPW, KFW, 3, true>, nullptr                                                  // streamed third limb
const V6Inst g_v6_inst[] = {
    {1024, 8, 3, false, V6_PAIR(16, 8, 3)},  {1024, 6, 3, false, V6_PAIR(16, 6, 3)},
    {1024, 3, 3, false, V6_PAIR(16, 3, 3)},  {1024, 2, 3, false, V6_PAIR(16, 2, 3)},       // a one-layer front-end (dilation_size 1): encoder in_dim 54, decoder 34
    // many-to-many decoders ([n_spk-wide code ; z], kernel_size 3, depth 2): in_dim 25..32 (KFW 5), 41..48 (7), 57..64 (9), 65..72 (11)
    {1024, 5, 3, false, V6_PAIR(16, 5, 3)},  {1024, 7, 3, false, V6_PAIR(16, 7, 3)},
    {1024, 9, 3, false, V6_PAIR(16, 9, 3)},  {1024, 11, 3, false, V6_PAIR(16, 11, 3)},
    {2048, 8, 3, true, V6_W2S(32, 8)},       {2048, 11, 3, true, V6_W2S(32, 11)},
    {2048, 8, 2, false, V6_PAIR(32, 8, 2)},  {2048, 11, 2, false, V6_PAIR(32, 11, 2)},
    {64, 3, 3, false, V6_PAIR(1, 3, 3)},     {64, 2, 3, false, V6_PAIR(1, 2, 3)},          {64, 1, 3, false, V6_PAIR(1, 1, 3)},
    {64, 3, 3, true, V6_W2S(1, 3)},          {64, 2, 3, true, V6_W2S(1, 2)},               {64, 1, 3, true, V6_W2S(1, 1)},
    {64, 3, 2, false, V6_PAIR(1, 3, 2)},     {64, 2, 2, false, V6_PAIR(1, 2, 2)},          {64, 1, 2, false, V6_PAIR(1, 1, 2)},
};
// k_gru_steps_v6<KPW, 0> (form V6H): the same recurrence with NO front-end of its own, behind the front-end GEMM -- for front-ends
// whose limb image cannot live in LDS.  The fused kernel keeps that image at 4 waves x KFW steps x 3 limbs x 1 KiB = 12 KiB per
// unit of KFW next to 22.5 KiB of reduction / publish buffers: KFW = 11 takes 132 + 22.5 = 154.5 of the 160 KiB a workgroup can
// have, KFW = 12 would take 166.5.  So V6H_MIN_KFW = 12, whatever H.  Keyed by H alone.
const int V6H_MIN_KFW = 12;
const V6Inst g_v6h_inst[] = {
    {1024, 0, 3, false, V6_PAIR(16, 0, 3)},
    {2048, 0, 3, true, V6_W2S(32, 0)},       // (three limbs, third weight limb streamed; no pair form: option v6_limbs_h2048 = 2 leaves such a pass on the per-step path)
    {64, 0, 3, false, V6_PAIR(1, 0, 3)},     {64, 0, 3, true, V6_W2S(1, 0)},               {64, 0, 2, false, V6_PAIR(1, 0, 2)},
};
#undef V6_PAIR
#undef V6_W2S
// the 16-row fused kernels: k_gru_steps_v5 (fp16 pairs) and k_gru_steps_v4 (fp32 MFMA), always built together
struct Fused16Inst { int H, KFW; void (*v5)(Step3Params); void (*v4)(Step3Params); };
const Fused16Inst g_fused16_inst[] = {
    {1024, 8, k_gru_steps_v5<16, 8>, k_gru_steps_v4<16, 8>}, {1024, 6, k_gru_steps_v5<16, 6>, k_gru_steps_v4<16, 6>},
    {64, 2, k_gru_steps_v5<1, 2>, k_gru_steps_v4<1, 2>},     {64, 1, k_gru_steps_v5<1, 1>, k_gru_steps_v4<1, 1>},
};
// k_outproj_v6, the projection from the limb triples a k_gru_steps_v6 pass leaves
struct Out6Inst { int H; void (*fn)(Out6Params); };
const Out6Inst g_out6_inst[] = {{1024, k_outproj_v6<16>}, {2048, k_outproj_v6<32>}, {64, k_outproj_v6<1>}};

inline int exact3_kpw(const Dims& m) { return m.H / 64; }
// limbs < 0: any form of that geometry (what the layouts ask: a limb image exists whatever the options pick)
inline const V6Inst* find_v6(const Dims& m, int limbs = -1, bool w2s = false) {
    for (const V6Inst& i : g_v6_inst)
        if (i.H == m.H && i.KFW == m.KFW && (limbs < 0 || (i.limbs == limbs && i.w2s == w2s))) return &i;
    return nullptr;
}
inline const Fused16Inst* find_fused16(const Dims& m) {
    for (const Fused16Inst& i : g_fused16_inst)
        if (i.H == m.H && i.KFW == m.KFW) return &i;
    return nullptr;
}
inline const V6Inst* find_v6h(const Dims& m, int limbs = -1, bool w2s = false) {
    if (m.KFW < V6H_MIN_KFW) return nullptr;
    for (const V6Inst& i : g_v6h_inst)
        if (i.H == m.H && (limbs < 0 || (i.limbs == limbs && i.w2s == w2s))) return &i;
    return nullptr;
}
inline bool exact3_fused(const Dims& m) { return find_v6(m) != nullptr; }      // front-end inside the kernel: limb image afold_t, limb input xt
// an exact-operand geometry: 32-row tiles from 4 rows on, recurrent / projection limb images -- fused or behind the front-end GEMM
inline bool exact3_ok(const Dims& m) { return exact3_fused(m) || find_v6h(m) != nullptr; }
// the form of k_gru_steps_v6 the options pick at this H: limbs per operand, third weight limb streamed
inline int v6_limbs(const Dims& m) {
    return (m.H == 64 && opt(OPT_V6_LIMBS_H64) == 2) || (m.H == 2048 && opt(OPT_V6_LIMBS_H2048) == 2) ? 2 : 3;
}
inline bool v6_w2s(const Dims& m) { return v6_limbs(m) == 3 && (m.H == 2048 || (m.H == 64 && opt(OPT_V6_W2S_H64))); }

// prepared image: offsets in floats, every block 64-float aligned
struct Prep {
    long afold, afold3, afold_h, afold_t, cfold, wrec, wrec2, wrec_h, wrec_t, wrec_l2b, bhn, wyT, wo, bo, wo2, bo2, wo3, sin_w, sin_b, sout_w,
        sout_b, range, total;
};

Prep prep_layout(const Dims& m, bool sin, bool sout) {
    Prep p;
    long o = 0;
    auto take = [&](long n) { long r = o; o += up(n, 64); return r; };
    p.afold = take((long)m.H3 * m.Kfe);
    p.afold3 = take((long)m.nch * 4 * m.KFW * 3 * 256);
    p.afold_h = take((long)m.nch * 4 * ((m.KFW + 1) / 2) * 6 * 256);   // front-end weights as fp16 pairs (LDS image of v5)
    p.cfold = take(m.H3);
    p.wrec = take((long)(m.H / 4) * m.nch * 256);
    p.wrec2 = take((long)m.nch * 4 * m.nch * 256);
    p.wrec_h = take((long)m.nch * 4 * (m.H / 32) * 2 * 256);   // fp16-pair image of wrec2 for k_gru_steps_v5
    // fp16-triple images of k_gru_steps_v6 (exact fp32 operands): recurrent B operands per (octet, wave, 16-k step, limb) and
    // the front-end LDS image; only for the sizes that kernel is built for
    p.wrec_t = exact3_ok(m) ? take((long)(m.H / 8) * 4 * exact3_kpw(m) * 3 * 256) : -1;
    p.afold_t = exact3_fused(m) ? take((long)(m.H / 8) * 4 * m.KFW * 3 * 256) : -1;
    p.wrec_l2b = exact3_ok(m) ? take((long)(m.H / 8) * 4 * exact3_kpw(m) * 128) : -1;   // third weight limbs as bf8 bytes (streamed form)
    p.bhn = take(m.H);
    p.wyT = take((long)m.H3 * m.Co);
    p.wo = take((long)m.Cop * m.H);
    p.bo = take(m.Cop);
    p.wo2 = take((long)m.Cop * m.H);
    p.bo2 = take(m.Cop);
    p.wo3 = exact3_ok(m) ? take((long)((m.Cop + 31) / 32) * (m.H / 16) * 3 * 256) : -1;   // projection B operands as limb triples
    p.sin_w = sin ? take((long)m.C * m.C) : -1;
    p.sin_b = sin ? take(m.C) : -1;
    p.sout_w = sout ? take((long)m.Co * m.Co) : -1;
    p.sout_b = sout ? take(m.Co) : -1;
    p.range = take(64);      // word 0: a folded weight does not fit its limb image (cvae_flag_unfit); the deep part of an image shares it
    p.total = o;
    return p;
}

// pass workspace: offsets in floats.  Brows = total batch rows of the pass (cells stacked along the batch axis)
struct Work {
    long status, xnp, xs, xs_plane, xt, xt_slack, gx, hbuf, hs, y, dy, gx0, prof, flags, total;
    int Bp, Tp, prof_blocks;
    long mtot;
};

// Batch rows are padded to whole row tiles: one 16-row tile for the word-exchange kernel (at most 3 rows), 32-row tiles
// (k_gru_steps_v6: exact operands) from 4 rows on wherever that kernel exists (fused or hoisted: exact3_ok) -- ONE arithmetic width for every batch size, a pass
// of 4..16 rows runs a half-empty tile rather than the 22-bit pair kernel -- else 16-row tiles up to 16 rows.  Independent of the
// pass's flags: the workspace size query has none.
inline int eval_row_pad(const Dims& m, int Brows) {
    return Brows <= 3 ? 16 : (exact3_ok(m) || Brows > 16 ? (int)up(Brows, 32) : 16);
}

Work work_layout(const Dims& m, int Brows, int T) {
    Work w;
    w.Bp = eval_row_pad(m, Brows);
    w.Tp = T + 2 * m.pad;
    w.mtot = (long)(T + 1) * w.Bp;
    long o = 0;
    auto take = [&](long n) { long r = o; o += up(n, 64); return r; };
    w.status = take(64);  // int32[4] status + barrier counter at word 8
    w.xnp = take((long)Brows * w.Tp * m.Cp + 64L * m.KFW + 64);
    w.xs_plane = up((long)Brows * w.Tp * m.Cp + 64L * m.KFW + 64, 8);   // halves per plane (hi, lo) of the fp16-pair copy
    w.xs = take(w.xs_plane);                                              // 2 planes x 2 bytes = xs_plane floats
    // k_gru_steps_v6's input: limb triples (5 bytes per element) + zero slack for the K padding of the last frames (16-bit words)
    w.xt_slack = (64L * m.KFW / 8 + 2) * 640 + 64;
    w.xt = exact3_fused(m) && w.Bp % 32 == 0 ? take(((long)w.Bp * w.Tp * m.Cp * 5 / 2 + w.xt_slack) / 2 + 8) : -1;
    w.gx = take((long)Brows * w.Tp * m.H3);
    w.hbuf = take((long)m.nch * w.mtot * 16);
    w.hs = take((long)m.nch * w.mtot * 24);     // exchanged state as fp16 pairs (64 B per row and 16 units) or triples (96 B)
    w.y = take((long)T * w.Bp * m.Cop);
    w.dy = take((long)w.Bp * m.Co);
    w.gx0 = take((long)w.Bp * m.H3);   // frame-0 feedback correction of the exact-operand kernel (prologue role gx0)
    w.prof_blocks = 256;
    w.prof = take(w.prof_blocks * 8L);  // long long[prof_blocks][4] step-timing counters
    w.flags = take((long)(w.Bp / 16) * m.nch);
    w.total = o;
    return w;
}

// Row tiles a block of an all-resident grid handles: as few as the chip allows (every CU gets a block), at most all of them.
// per_tile: blocks one row tile takes.  Option max_rt caps it (tests: several row tiles per block on small problems).
inline int row_tiles_per_block(int cus, int per_tile, int ntiles) {
    int rts = per_tile > 0 ? cus / per_tile : 1;
    rts = rts < 1 ? 1 : (rts > ntiles ? ntiles : rts);
    if (opt(OPT_MAX_RT) >= 1 && opt(OPT_MAX_RT) < rts) rts = (int)opt(OPT_MAX_RT);
    return rts;
}

// Which kernels an eval pass of a one-layer network runs (the one place that decides; cvae_plan_pass reports the form; the table
// of form x condition is DESIGN.md 4.1).  The forms are numbered so that a refused cooperative launch steps DOWN:
// V5 -> V4 -> V2 -> GENERIC -> PER_STEP (run_pass; LL, V6 and V6H return the error).
struct PassFacts {      // what a call's pointers decide
    bool h_in, y_last, h_last, many_draws;      // any cell with a carried-in state / a raw last projection / a state out / n_draws > 1
    bool fresh;                                 // any cell without a carried-in state
    bool h_in_y;                                // any cell with a carried-in state AND a y_in of its own: its frame-0 feedback correction
                                                //   W_ih[:, R*C:] . (y_in - out_1(h_in)) needs the dy role's H-long products
};
enum { PRO_ROWS = 0, PRO_DRAWS = 1, PRO_TILES = 2 };      // prologue launch: 64 threads per (row, frame); 256 (draws summed in slices); 256 per (32-row tile, frame)
enum { PROJ_GEMM = 0, PROJ_FUSED = 1, PROJ_V6 = 2 };      // projection: GEMM + k_epilogue; k_outproj<1|4|8>; k_outproj_v6
struct EvalPlan {
    int form;                             // CVAE_EVAL_*
    void (*k6)(Step6Params);              // the instance to launch: V6
    void (*k5)(Step3Params);              // V5
    void (*k4)(Step3Params);              // V4, and what a refused V5 steps down to
    void (*kout6)(Out6Params);            // PROJ_V6
    int rts;                              // row tiles per block (V6: of 32 rows; V5 / V4 / V2: of 16)
    int backoff;                          // first-poll back-off (LL: s_sleep units, V6: x 64 cycles)
    bool limbs;                           // the pass BUILDS limb operands: its prologue gets the range word
    bool pairs;                           // the prologue writes the fp16-pair copies (SPLIT_F16 off V6; V6: the limb triples instead)
    bool gx0_ready;                       // the prologue forms the frame-0 feedback correction (else k_gru_steps_v6 does: cvae_t0_fix)
    bool want_f32;                        // V6 also writes the fp32 state copy
    bool h0_zero;                         // V6 / V6H: slot 0 is all zeros (the prologue's fresh-pass branch) and frame 0 skips its recurrent product
    int prologue, proj;                   // PRO_*, PROJ_*
};

// projection off the fp32 states: k_outproj exists for 16, 64 and 128 padded outputs and does not leave the raw last projection
inline int plain_projection(const Dims& m, bool y_last) {
    const int ntn = m.Cop / 16;
    return !y_last && (ntn == 1 || ntn == 4 || ntn == 8) ? PROJ_FUSED : PROJ_GEMM;
}

inline bool generic_resident(const Dims& m, int cus) { return cus <= 0 || m.H / 4 <= cus; }      // one 256-thread block per CU is always admitted

EvalPlan plan_eval_pass(const Dims& m, int Brows, int T, int flags, int cus, bool unfit, const PassFacts& f) {
    EvalPlan pn;
    memset(&pn, 0, sizeof(pn));
    // an image whose folded weights do not fit the limb images (cvae_net_prepared_in_range) runs on the fp32-operand kernels
    if (unfit) flags &= ~CVAE_FLAG_SPLIT_F16;
    const int Bp = eval_row_pad(m, Brows);
    const long mtot = (long)(T + 1) * Bp;
    const bool persistent = (flags & CVAE_FLAG_PERSISTENT) && T > 1, generic = (flags & CVAE_FLAG_GENERIC_STEP) != 0;
    const bool hoisted = (flags & CVAE_FLAG_HOISTED_FRONTEND) != 0, exact = persistent && (flags & CVAE_FLAG_EXACT3) && !generic;
    const V6Inst* i6 = find_v6(m, v6_limbs(m), v6_w2s(m));
    const V6Inst* i6h = find_v6h(m, v6_limbs(m), v6_w2s(m));
    const Fused16Inst* i16 = find_fused16(m);
    if (exact && Brows <= 3 && T < 65536 && m.H % 64 == 0 && m.H <= 1024 && cus >= m.H / 4 && !opt(OPT_NO_LL)) {
        // at most three rows: a step is one store + one polled load per unit, plain fp32 FMAs; H/4 blocks, every one resident
        pn.form = CVAE_EVAL_LL;
        pn.backoff = opt(OPT_LL_BACKOFF) >= 0 ? (int)opt(OPT_LL_BACKOFF) : (Brows == 1 ? 22 : 20);   // swept per row count (round 4, after the prefetch reordering: profiles/r04_notes.md; round 2: 18 / 16)
    } else if (exact && !unfit && !hoisted && i6 && Bp % 32 == 0 && cus >= m.H / 8 && (long)m.nch * mtot * 80 < (1L << 31)) {
        // exact fp32 operands as fp16 triples: 32-row tiles, 8-unit octets, H/8 blocks per tile, every block resident
        pn.form = CVAE_EVAL_V6;
        pn.k6 = (flags & CVAE_FLAG_STEP_TIMING) && i6->fn_prof ? i6->fn_prof : i6->fn;
        pn.rts = row_tiles_per_block(cus, m.H / 8, Bp / 32);
        // One row tile per block (B <= 64 at hu1024): nothing can be published before the other blocks' front-ends are through, and
        // 256 waves polling through that window slow the publishes and operand loads they wait for.  The decoder's front-end is a
        // quarter shorter than the encoder's (KFW 6 vs 8), so its blocks arrive at the poll earlier: swept on MI355X
        // (tools/ab_eval_exp.sh, round 5), 64-cycle units -- decoder pass 421.7 (0) / 405.8 (4) / 397.1 (8) / 401.0 (12) / 409.0 us
        // (16), encoder pass 412.3 / 411.0 / 416.6 / 423.9 / 434.5 us.  Swept again once the front-end read its weights one step ahead
        // (1.6K instead of 2.0K cycles at KFW 8: the blocks reach the poll earlier still; profiles/v6_hot_loop_notes.md): encoder pass
        // 424.9 (0) / 416.4 (2) / 409.9 (4) / 400.3 (8) / 398.5 (10) / 399.9 (12) / 406.3 us (16), decoder pass 478.4 (0) / 419.9 (4) /
        // 399.2 (8) / 388.9 (10) / 386.9 (12) / 384.5 us (16).  The one-layer front-ends (KFW 3, 2) keep the earlier decoder value: not swept.
        // The many-to-many decoder widths take the value of the swept width next to them (KFW 5: 8, KFW 7 / 9 / 11: 10): not swept either.
        pn.backoff = opt(OPT_V6_BACKOFF) >= 0 ? (int)opt(OPT_V6_BACKOFF) : (m.H == 1024 ? (m.KFW > 6 ? 10 : (m.KFW == 6 ? 16 : 8)) : 0);
    } else if (exact && !unfit && !hoisted && i6h && Bp % 32 == 0 && cus >= m.H / 8 && (long)m.nch * mtot * 80 < (1L << 31)) {
        // the same recurrence behind the front-end GEMM, for a front-end too wide for the LDS limb image (KFW >= 12: find_v6h).
        // HOISTED_FRONTEND keeps its meaning -- the 16-row kernel behind the GEMM (V2) -- so that the two can be compared.
        pn.form = CVAE_EVAL_V6H;
        i6 = i6h;
        pn.k6 = (flags & CVAE_FLAG_STEP_TIMING) && i6h->fn_prof ? i6h->fn_prof : i6h->fn;
        pn.rts = row_tiles_per_block(cus, m.H / 8, Bp / 32);
        pn.backoff = opt(OPT_V6_BACKOFF) >= 0 ? (int)opt(OPT_V6_BACKOFF) : 0;      // (nothing runs in front of the poll; not swept)
    } else if (persistent && !generic && (m.H == 1024 || m.H == 64) && cus >= m.nch && (long)m.nch * mtot * 64 < (1L << 31)) {
        // the 16-row dataflow kernels (H/16 blocks per tile, every block resident): front-end fused where an instance exists for
        // the front-end width -- on fp16 pairs (V5) or the fp32 MFMA (V4) -- else behind a hoisted GEMM (V2)
        pn.form = hoisted || !i16 ? CVAE_EVAL_V2 : ((flags & CVAE_FLAG_SPLIT_F16) ? CVAE_EVAL_V5 : CVAE_EVAL_V4);
        if (i16) pn.k5 = i16->v5, pn.k4 = i16->v4;
        pn.rts = row_tiles_per_block(cus, m.nch, Bp / 16);
    } else {
        // the any-H kernel: one launch behind a grid barrier when its H/4 blocks are resident, else one launch per step
        pn.form = persistent && generic_resident(m, cus) ? CVAE_EVAL_GENERIC : CVAE_EVAL_PER_STEP;
    }
    const bool v6f = pn.form == CVAE_EVAL_V6, v6 = v6f || pn.form == CVAE_EVAL_V6H;      // fused; fused or hoisted
    pn.limbs = v6 || pn.form == CVAE_EVAL_V5;
    // the pair copies are written whenever SPLIT_F16 is set off V6, but only k_gru_steps_v5 reads them: a pass that ends up on
    // k_gru_steps_ll or on an fp32-operand kernel has nothing to report (limbs)
    pn.pairs = !v6 && (flags & CVAE_FLAG_SPLIT_F16);
    // A pass that MIXES fresh cells (no h_in: dy = y_in - out_1.b) with cells that continue a recurrence (h_in, no y_in: dy = 0) keeps
    // the prologue's gx0 role: the fresh cells then compute the bits they compute in a pass of fresh cells only (a live stream opens
    // sessions next to running ones: stream.py), and the role writes zeros for the continuing cells, which changes no bit of them.
    // Every other pass with a carried state -- all cells continuing (the windowed stage 6), or a cell with both h_in and y_in (the
    // chain's carry form, GRU_RNN.forward(h_in=...)) -- forms the correction in the recurrent kernel (cvae_t0_fix), as before.
    pn.gx0_ready = v6 && (!f.h_in || (f.fresh && !f.h_in_y));
    // no cell carries a state in <=> k_prologue zero-fills slot 0 (its !any_h branch reads the same pointers PassFacts was built from)
    pn.h0_zero = v6 && !f.h_in && opt(OPT_V6_SKIP_T0) != 0;
    // the fp32 state copy of a V6 pass is only read by the raw projection (y_last), k_hlast and the projections off the limb triples
    pn.want_f32 = v6 && (i6->limbs != 3 || f.y_last || f.h_last || (opt(OPT_EXP) & 16));      // (exp bit 4: always write it, for A/B measurements)
    // (V6H: the input goes through the fp32 GEMM -- no limb copy of it, the row-wise prologue; its range word then covers h_in only)
    pn.prologue = v6f ? PRO_TILES : (f.many_draws ? PRO_DRAWS : PRO_ROWS);
    if (!f.y_last && v6 && i6->limbs == 3) {
        pn.proj = PROJ_V6;      // the pass left the state as limb triples in the exchange buffer: project from there, same exact arithmetic
        for (const Out6Inst& o : g_out6_inst)
            if (o.H == m.H) pn.kout6 = o.fn;
    } else {
        pn.proj = plain_projection(m, f.y_last);
    }
    return pn;
}

bool prof_begin(hipStream_t st, int rows = 0, int cin = 0) {
    if (cx().prof.used == cx().prof.start.size()) {
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return false;
        cx().prof.start.push_back(a);
        cx().prof.stop.push_back(b);
        cx().prof.rows.push_back(0);
        cx().prof.cin.push_back(0);
    }
    cx().prof.rows[cx().prof.used] = rows;
    cx().prof.cin[cx().prof.used] = cin;
    return hipEventRecord(cx().prof.start[cx().prof.used], st) == hipSuccess;
}
void prof_end(hipStream_t st) {
    (void)hipEventRecord(cx().prof.stop[cx().prof.used], st);
    cx().prof.used++;
}

struct TrainProf {     // RAII bracket; inactive unless the option is set
    hipStream_t st;
    bool on;
    TrainProf(hipStream_t st_, int cls, double flop) : st(st_), on(false) {
        if (!opt(OPT_TRAIN_PROFILE)) return;
        if (cx().tprof.used == cx().tprof.start.size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
            cx().tprof.start.push_back(a); cx().tprof.stop.push_back(b); cx().tprof.cls.push_back(0); cx().tprof.flop.push_back(0.0);
        }
        cx().tprof.cls[cx().tprof.used] = cls;
        cx().tprof.flop[cx().tprof.used] = flop;
        on = hipEventRecord(cx().tprof.start[cx().tprof.used], st) == hipSuccess;
    }
    void end() {
        if (!on) return;
        (void)hipEventRecord(cx().tprof.stop[cx().tprof.used], st);
        cx().tprof.used++;
        on = false;
    }
    ~TrainProf() { end(); }
};

// a few words to zero in front of a chain of kernels: as a KERNEL (hipMemsetAsync of 32 bytes is followed by ~15 us of idle
// stream before the next kernel starts, rocprofv3 trace on MI355X; a kernel chains back to back)
__global__ void k_clear_words(int32_t* p, int n) {
    if ((int)threadIdx.x < n) p[threadIdx.x] = 0;
}
inline hipError_t clear_words(void* p, int n, hipStream_t st) {
    hipLaunchKernelGGL((k_clear_words), dim3(1), dim3(64), 0, st, (int32_t*)p, n);
    return hipGetLastError();
}

// Test aid (exp bit 7): slot 0 of a V6 pass's state buffers -- the limb triples and the fp32 copy -- overwritten with 0xFF bytes (NaN as
// half, as bf8 and as fp32) behind the prologue: a fresh pass whose frame 0 skips the recurrent product (v6_skip_t0) reads none of it.
// One block per 16-unit chunk: Bp * 80 B of triples and Bp * 64 B of fp32 state, both runs inside the chunk's (T + 1) * Bp rows.
__global__ void k_poison_slot0(unsigned* hx, unsigned* hbuf, long mtot, int Bp) {
    unsigned* a = hx + (long)blockIdx.x * mtot * 20;
    unsigned* b = hbuf + (long)blockIdx.x * mtot * 16;
    for (int i = threadIdx.x; i < Bp * 20; i += blockDim.x) a[i] = 0xffffffffu;
    for (int i = threadIdx.x; i < Bp * 16; i += blockDim.x) b[i] = 0xffffffffu;
}

int cu_count() {
    static int cached[16] = {};          // (asked several times per pass: the layouts depend on it)
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (dev >= 0 && dev < 16 && cached[dev] > 0) return cached[dev];
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    if (dev >= 0 && dev < 16) cached[dev] = n;
    return n;
}

// Range guard (CVAE_STATUS_RANGE): where a pass's prologue reports an operand the limb form cannot carry.  limbs: the pass builds
// limb operands; new_call: first pass of an entry point (a new serial number; the workspace epoch is written).
inline bool image_known_unfit(const float* P) {
    auto it = cx().image_unfit.find((const void*)P);
    return it != cx().image_unfit.end() && it->second;
}
inline void range_params(ProParams& pp, int* ws_status, bool limbs, bool new_call, const float* P, const Prep& pl) {
    if (new_call) {
        cx().range_serial += 1;
        if (cx().range_serial <= 0) cx().range_serial = 1;
    }
    long at = opt(OPT_EXACT_RANGE_AT);
    at = at < 1 ? 1 : (at > 65504 ? 65504 : at);
    pp.range_at = (float)at;
    pp.image_unfit = (const int*)(P + pl.range);
    if (cx().status_sink) {      // sticky, cleared by the host
        pp.range_word = limbs ? cx().status_sink + CVAE_STATUS_RANGE_WORD : nullptr;
        pp.range_epoch = nullptr;
        pp.range_val = CVAE_STATUS_RANGE;
    } else {
        pp.range_word = limbs ? ws_status + CVAE_WS_RANGE_WORD : nullptr;
        pp.range_epoch = new_call ? ws_status + CVAE_WS_RANGE_EPOCH : nullptr;
        pp.range_val = cx().range_serial;
    }
}

// One cell of a pass: passes that share weights and have no mutual dependence (rec || cv of a cycle) run as ONE
// pass whose batch is the cells' batches stacked; the recurrence then has extra independent row tiles to interleave.
struct Cell {
    const cvae_pass_input* in;
    const float* y_in;   // [B][Co]
    const float* h_in;   // [B][H] or null
    float* trj_out;      // [B][T][Co]
    float* y_last;       // [B][Co] or null
    float* h_last;       // [B][H] or null
};

// ---- The stages of an eval pass.  The one-layer pass (run_pass) and the stacked pass (run_pass_deep, cvae_deep.inc) are sequences
// of these; a stage takes pointers and sizes, never a workspace layout: the two passes keep their own (Work, DeepWork).

// slot whose state a cell carries on: the one behind ITS last valid frame (slot `frames`), not behind the pass's T steps -- a cell
// shorter than the pass keeps stepping over padding (or, for a window with ctx_after > 0, over frames that belong to the next
// window), and continuing from slot T restarted the next window from the wrong state
inline int last_slot(const cvae_pass_input* in, int T) { return in->frames > 0 && in->frames < T ? in->frames : T; }

// The rows of a pass: ncell cells of B rows each over T frames, padded to Bp rows; mtot = (T + 1) * Bp state rows per 16-unit chunk.
struct PassRows {
    const Cell* cells;
    int ncell, B, T, Bp;
    long mtot;
};

int check_cells(const Dims& m, const PassRows& r) {
    const Cell* cells = r.cells;
    const int ncell = r.ncell, B = r.B, T = r.T;
    if (ncell > CVAE_MAX_CELLS) return fail(-1, "at most %d stacked cells per pass", CVAE_MAX_CELLS);
    for (int c = 0; c < ncell; ++c) {
        const cvae_pass_input* in = cells[c].in;
        const int w_in = in->seg0.width + (in->lat ? draw_dim(in->lat_dim) : in->seg1.width);
        if (w_in != m.C) return fail(-1, "cell %d: pass input width %d != in_dim %d", c, w_in, m.C);
        if (in->frames < 0 || in->frames > T) return fail(-1, "cell %d: frames %d outside [0, T=%d]", c, in->frames, T);
        if (in->ctx_before < 0 || in->ctx_after < 0 || in->draw_frame0 < 0 || in->eps_draw_stride < 0)
            return fail(-1, "cell %d: negative window context / draw origin", c);
        if ((in->ctx_before || in->ctx_after || in->draw_frame0) && B != 1)
            return fail(-1, "cell %d: windows of a longer utterance (ctx_before / ctx_after / draw_frame0) are single-row cells, B=%d", c, B);
    }
    return 0;
}

// The launch shape of a pass's prologue and what it writes; a null pointer = the pass has no such output.
struct ProTargets {
    int shape;                // PRO_ROWS / PRO_DRAWS / PRO_TILES
    float* xnp;               // the assembled, normalised, padded input
    float* dy;                // y_in - out_1(h_in) per row
    float* slot0;             // state buffer whose slot 0 is initialised from the cells' h_in (stacked: the top layer's buffer and h_in;
                              //   k_deep_slot0 then fills every layer)
    unsigned* zero_words;     // hand-off flags to zero, and how many
    int nzero;
    int* zero_status;         // status words to clear, and how many (never the range word)
    int zero_status_n;
    int* ws_status;           // the workspace's own status words: home of the range word / epoch when no sink is set
    bool limbs, new_call;     // range_params
    float* hx;                // slot 0 as limb triples (V6, V6H)
    float* xt;                // the input as limb triples (V6) + nxt_slack zero words
    int nxt_slack;
    float* hs;                // fp16-pair copies of slot 0 and of the input (SPLIT_F16 off V6)
    float* xs;
    long xs_plane;
    float* gx0;               // frame-0 feedback correction (V6: no carried-in state, or fresh cells beside continuing ones)
    unsigned* ll_counter;     // launch counter of k_gru_steps_ll
};
struct RangeSlot { int* word; int val; float at; };      // where and how a kernel behind the prologue reports on the same guard

// One k_prologue launch in the shape the caller names (PRO_*): assemble + scale_in + padding, slot-0 init, dy (the feedback is
// out_1 of each cell's h_in), frame-0 feedback correction, zeroing.  Brows = ncell * B rows, padded to Bp.
void run_prologue(const Dims& m, const cvae_net_desc* d, const float* P, const Prep& pl, const PassRows& r, const ProTargets& o,
                  hipStream_t st, RangeSlot* range = nullptr) {
    const Cell* cells = r.cells;
    const int ncell = r.ncell, B = r.B, T = r.T, Bp = r.Bp, shape = o.shape;
    const int Brows = ncell * B, Tp = T + 2 * m.pad;
    ProParams pp;
    memset(&pp, 0, sizeof(pp));
    for (int c = 0; c < ncell; ++c) {
        const cvae_pass_input* in = cells[c].in;
        pp.cell[c].seg0 = CvaeSeg{in->seg0.ptr, in->seg0.width, in->seg0.row_stride};
        pp.cell[c].seg1 = CvaeSeg{in->seg1.ptr, in->seg1.width, in->seg1.row_stride};
        pp.cell[c].lat = in->lat;
        pp.cell[c].eps = in->eps;
        pp.cell[c].seed = in->seed;
        pp.cell[c].draw = in->draw_id;
        pp.cell[c].y_in = cells[c].y_in;
        pp.cell[c].h_in = cells[c].h_in;
        pp.cell[c].frames = in->frames;
        pp.cell[c].n_draws = in->n_draws;
        pp.cell[c].ctx_before = in->ctx_before; pp.cell[c].ctx_after = in->ctx_after;
        pp.cell[c].draw_frame0 = (long)in->draw_frame0; pp.cell[c].eps_stride = (long)in->eps_draw_stride;
        if (in->lat) pp.L = draw_dim(in->lat_dim);
        if (in->lat && draw_laplace(in->lat_dim)) pp.laplace |= 1u << c;
    }
    pp.ncell = ncell;
    pp.frame0 = (uint64_t)cx().draw_row0 * (uint64_t)T;
    pp.sin_w = d->has_scale_in ? P + pl.sin_w : nullptr;
    pp.sin_b = d->has_scale_in ? P + pl.sin_b : nullptr;
    pp.wo = P + pl.wo; pp.bo = P + pl.bo;
    pp.B = B; pp.T = T; pp.C = m.C; pp.Cp = m.Cp; pp.pad = m.pad; pp.Co = m.Co; pp.H = m.H; pp.Bp = Bp;
    pp.nslack = 64 * m.KFW + 64;
    pp.mtot = r.mtot;
    pp.xnp = o.xnp; pp.hbuf = o.slot0; pp.dy = o.dy;
    pp.hx = o.hx; pp.xt = o.xt; pp.nxt_slack = o.nxt_slack;
    pp.hs = o.hs; pp.xs = o.xs; pp.xs_plane = o.xs_plane;
    pp.zero_words = o.zero_words; pp.nzero = o.nzero;
    pp.zero_status = o.zero_status; pp.zero_status_n = o.zero_status_n;
    pp.ll_counter = o.ll_counter;
    pp.nA = (shape == PRO_TILES ? Bp / 32 : Brows) * Tp;      // PRO_TILES: one block per (32-row tile, padded frame)
    pp.nH = (int)nblk((long)Bp * m.H, 1024);
    pp.nD = (int)nblk((long)Brows * m.Co, 64);
    pp.nG = o.gx0 ? (int)nblk((long)Brows * m.H3 / 4, shape == PRO_ROWS ? 64 : 256) : 0;      // (four columns per thread of the launch's block size)
    pp.gx0 = o.gx0; pp.wyT = P + pl.wyT;
    range_params(pp, o.ws_status, o.limbs, o.new_call, P, pl);
    if (range) *range = RangeSlot{pp.range_word, pp.range_val, pp.range_at};
    const dim3 gp(pp.nA + pp.nH + pp.nD + pp.nG + 1);
    if (shape == PRO_TILES)
        hipLaunchKernelGGL((k_prologue), gp, dim3(256),
                           (size_t)32 * (m.C + 1) * sizeof(float) + (size_t)(m.Cp / 8) * 1280 + (size_t)32 * pp.L * sizeof(float), st, pp);
    else if (shape == PRO_DRAWS)     // 256 threads per block: the draws of a frame are summed in parallel slices
        hipLaunchKernelGGL((k_prologue), gp, dim3(256), (size_t)(m.C + 1024 + 256) * sizeof(float), st, pp);
    else
        hipLaunchKernelGGL((k_prologue), gp, dim3(64), m.C * sizeof(float), st, pp);
}

// gx[b*Tp + t] = afold . xnp[b, t:t+R, :] + cfold for all frames: one GEMM over overlapping rows (lda = Cp), in front of every
// recurrence that has no front-end of its own
void run_front_end_gemm(const Dims& m, const float* P, const Prep& pl, const float* xnp, float* gx, int rows, int Tp, hipStream_t st) {
    const int M = rows * Tp, N = m.H3;
    hipLaunchKernelGGL((k_gemm_nt<4, 4, 2, 2, false>), dim3(nblk(N, 128), nblk(M, 128)), dim3(256), 0, st, xnp, (long)m.Cp, 0L,
                       P + pl.afold, (long)m.Kfe, P + pl.cfold, gx, (long)m.H3, M, N, m.Kfe);
}

// Projection of the fp32 states in hbuf (slots 1..T), as plain_projection() chose: PROJ_FUSED = k_outproj (scale_out folded in,
// clamp, written straight into [B][T][Co]); PROJ_GEMM = y[t*Bp + b] = out_1(h_t) (A = hbuf chunk-major, rows offset by Bp) and one
// k_epilogue per cell, which also leaves the raw last projection in y_last.
void run_projection(const Dims& m, const cvae_net_desc* d, const float* P, const Prep& pl, const PassRows& r, int proj, const float* hbuf,
                    float* y, int clamp_lat_dim, hipStream_t st) {
    const Cell* cells = r.cells;
    const int ncell = r.ncell, B = r.B, T = r.T, Bp = r.Bp;
    const long mtot = r.mtot;
    if (proj == PROJ_FUSED) {
        OutParams op;
        op.hbuf = hbuf; op.mtot = mtot; op.wo2 = P + pl.wo2; op.bo2 = P + pl.bo2; op.H = m.H; op.Bp = Bp; op.T = T;
        op.B = B; op.ncell = ncell; op.Co = m.Co; op.clamp_from = d->has_scale_out ? -1 : clamp_dim(clamp_lat_dim);
        op.clamp_min = clamp_floor(clamp_lat_dim);
        for (int c = 0; c < CVAE_MAX_CELLS; ++c) op.out[c] = c < ncell ? cells[c].trj_out : nullptr;
        const int ntn = m.Cop / 16;
        const unsigned nb = (unsigned)((long)T * Bp / 16);
        const size_t lds = (size_t)4 * 16 * (m.Cop + 4) * sizeof(float);
        void (*const kout)(OutParams) = ntn == 1 ? k_outproj<1> : ntn == 4 ? k_outproj<4> : k_outproj<8>;
        hipLaunchKernelGGL(kout, dim3(nb), dim3(256), lds, st, op);
        return;
    }
    const int M = T * Bp, N = m.Co;
    hipLaunchKernelGGL((k_gemm_nt<2, 4, 4, 1, true>), dim3(nblk(N, 64), nblk(M, 128)), dim3(256), 0, st, hbuf + (long)Bp * 16, 0L, mtot,
                       P + pl.wo, (long)m.H, P + pl.bo, y, (long)m.Cop, M, N, m.H);
    for (int c = 0; c < ncell; ++c) {
        EpiParams ep;
        ep.y = y; ep.ldy = m.Cop;
        ep.sout_w = d->has_scale_out ? P + pl.sout_w : nullptr;
        ep.sout_b = d->has_scale_out ? P + pl.sout_b : nullptr;
        ep.clamp_from = d->has_scale_out ? -1 : clamp_dim(clamp_lat_dim);
        ep.clamp_min = clamp_floor(clamp_lat_dim);
        ep.B = B; ep.Bp = Bp; ep.T = T; ep.Co = m.Co; ep.b0 = c * B;
        ep.trj_out = cells[c].trj_out; ep.y_last = cells[c].y_last;
        ep.t_last = last_slot(cells[c].in, T) - 1;
        hipLaunchKernelGGL((k_epilogue), dim3(B * T), dim3(64), m.Co * sizeof(float), st, ep);
    }
}

// k_hlast for every cell that asks: its h_last = the state in slot last_slot() of hbuf (one layer's buffer)
void run_last_states(const Dims& m, const PassRows& r, const float* hbuf, hipStream_t st) {
    for (int c = 0; c < r.ncell; ++c)
        if (r.cells[c].h_last)
            hipLaunchKernelGGL((k_hlast), dim3(nblk((long)r.B * m.H, 256)), dim3(256), 0, st, hbuf, r.mtot, r.cells[c].h_last, r.B, r.Bp,
                               m.H, last_slot(r.cells[c].in, r.T), c * r.B);
}

// plan, prologue, the recurrence (one switch on the planned form), projection, last states
int run_pass(const Dims& m, const cvae_net_desc* d, const float* P, const Cell* cells, int ncell, int B, int T,
             int clamp_lat_dim, float* ws, int* status, int flags, hipStream_t st, bool clear_status = false) {
    const Prep pl = prep_layout(m, d->has_scale_in != 0, d->has_scale_out != 0);
    const int Brows = ncell * B;
    const Work wl = work_layout(m, Brows, T);
    int* const ws_status = status;
    if (cx().status_sink) status = cx().status_sink;    // host-visible sticky word: a time-out is seen without reading the workspace back
    const PassRows rows = {cells, ncell, B, T, wl.Bp, wl.mtot};
    if (int rc = check_cells(m, rows)) return rc;
    unsigned* bar = (unsigned*)(ws + wl.status) + 8;  // status words themselves are sticky: zeroed by the entry point
    float* xnp = ws + wl.xnp;
    float* gx = ws + wl.gx;
    float* hbuf = ws + wl.hbuf;
    float* dy = ws + wl.dy;
    unsigned* hflags = (unsigned*)(ws + wl.flags);
    long long* const step_prof = (flags & CVAE_FLAG_STEP_TIMING) ? (long long*)(ws + wl.prof) : nullptr;
    const int cus = cu_count();
    PassFacts facts = {};
    for (int c = 0; c < ncell; ++c) {
        facts.h_in = facts.h_in || cells[c].h_in != nullptr;
        facts.fresh = facts.fresh || cells[c].h_in == nullptr;
        facts.h_in_y = facts.h_in_y || (cells[c].h_in != nullptr && cells[c].y_in != nullptr);
        facts.y_last = facts.y_last || cells[c].y_last != nullptr;
        facts.h_last = facts.h_last || cells[c].h_last != nullptr;
        facts.many_draws = facts.many_draws || (cells[c].in->lat && cells[c].in->n_draws > 1);
    }
    const EvalPlan pn = plan_eval_pass(m, Brows, T, flags, cus, image_known_unfit(P), facts);

    {
        ProTargets o = {};
        o.shape = pn.prologue; o.xnp = xnp; o.dy = dy;
        o.slot0 = hbuf;
        // bar (8 words) ... flags are not adjacent: zero the flags here, the barrier words with the status block
        o.zero_words = hflags; o.nzero = wl.Bp / 16 * m.nch;
        o.zero_status = clear_status ? status : nullptr;     // (the recurrent kernel, the first writer of these words, runs behind the prologue)
        o.zero_status_n = cx().status_sink ? 4 : 8;          // (a sink is int32[4]: eight words ran over the end of the caller's buffer)
        o.ws_status = ws_status; o.limbs = pn.limbs; o.new_call = clear_status;
        // k_gru_steps_v6 reads limb triples -- the state always, the input where its front-end is fused -- every other kernel the fp32 buffers
        const bool triples = pn.form == CVAE_EVAL_V6 || pn.form == CVAE_EVAL_V6H;
        o.hx = triples ? ws + wl.hs : nullptr;    // (the pair buffer's space: same size, never both in one pass)
        o.xt = pn.form == CVAE_EVAL_V6 ? ws + wl.xt : nullptr;
        o.nxt_slack = (int)wl.xt_slack;
        o.hs = pn.pairs ? ws + wl.hs : nullptr;
        o.xs = pn.pairs ? ws + wl.xs : nullptr;
        o.xs_plane = wl.xs_plane;
        o.gx0 = pn.gx0_ready ? ws + wl.gx0 : nullptr;
        o.ll_counter = pn.form == CVAE_EVAL_LL ? (unsigned*)(ws + wl.status) + 16 : nullptr;
        run_prologue(m, d, P, pl, rows, o, st);
        if (triples && (opt(OPT_EXP) & 128))
            hipLaunchKernelGGL((k_poison_slot0), dim3(m.nch), dim3(256), 0, st, (unsigned*)(ws + wl.hs), (unsigned*)hbuf, wl.mtot, wl.Bp);
    }

    const size_t lds2 = (4 * 16 * 84 + 16 * 16) * sizeof(float);
    const bool prof = (flags & CVAE_FLAG_PROFILE) && prof_begin(st, ncell * B, m.C);
    // a refused cooperative launch (error handling, not selection: the plan only names kernels that exist)
    const auto refused = [](hipError_t e) {
        if (e == hipSuccess) return false;
        (void)hipGetLastError();
        return true;
    };
    int form = pn.form;      // steps down where a launch is refused
    // the front-end GEMM in front of every form whose kernel has no front-end of its own
    if (form == CVAE_EVAL_LL || form == CVAE_EVAL_V6H || form <= CVAE_EVAL_V2) run_front_end_gemm(m, P, pl, xnp, gx, Brows, wl.Tp, st);
    switch (form) {
    case CVAE_EVAL_LL: {
        StepLLParams q;
        q.hbuf = hbuf; q.mtot = wl.mtot; q.xbuf = ws + wl.hs; q.wrec2 = P + pl.wrec2; q.gx = gx; q.gx_bstride = (long)wl.Tp * m.H3;
        q.bhn = P + pl.bhn; q.B = Brows; q.Bp = wl.Bp; q.H = m.H; q.T = T; q.status = status;
        q.prof = step_prof;
        q.wyT = P + pl.wyT; q.dy = dy; q.Co = m.Co;
        q.dbg = (int*)(ws + wl.status);
        q.backoff = pn.backoff;
        q.nonce_src = (const unsigned*)(ws + wl.status) + 16;
        const dim3 gl(m.H / 4);
        const size_t ldsl = (size_t)(2 * 64 * 49 + 4 * 48) * sizeof(float);
        const hipError_t e = cvae_launch_coop(Brows == 1 ? k_gru_steps_ll<1> : Brows == 2 ? k_gru_steps_ll<2> : k_gru_steps_ll<3>, gl,
                                              dim3(256), ldsl, st, q);
        if (refused(e)) return fail(-3, "small-batch recurrent kernel failed to launch: %s", hipGetErrorString(e));
        break;
    }
    case CVAE_EVAL_V6:
    case CVAE_EVAL_V6H: {
        const bool fused = form == CVAE_EVAL_V6;
        Step6Params q;
        q.hbuf = hbuf; q.mtot = wl.mtot; q.hx = ws + wl.hs; q.wrec3 = P + pl.wrec_t; q.afold3 = fused ? P + pl.afold_t : nullptr; q.w2s = P + pl.wrec_l2b;
        q.cfold = P + pl.cfold; q.bhn = P + pl.bhn; q.xt = fused ? ws + wl.xt : nullptr; q.Tp = wl.Tp; q.Cp = m.Cp;
        q.gx = fused ? nullptr : gx; q.gx_bstride = (long)wl.Tp * m.H3;      // V6H: the GEMM's output, cfold included
        q.B = Brows; q.Bp = wl.Bp; q.H = m.H; q.T = T; q.flags = hflags; q.status = status;
        q.prof = step_prof;
        q.wyT = P + pl.wyT; q.dy = dy; q.Co = m.Co;
        q.gx0 = pn.gx0_ready ? ws + wl.gx0 : nullptr;
        q.want_f32 = pn.want_f32 ? 1 : 0;
        q.h0_zero = pn.h0_zero ? 1 : 0;
        q.rts = pn.rts;
        q.exp = (int)opt(OPT_EXP);   // measurement switches only
        q.backoff = pn.backoff;
        const size_t lds6 = (size_t)(4 * 32 * 40 + 32 * 8 + 384 + (fused ? 4 * m.KFW * v6_limbs(m) * 256 : 0)) * sizeof(float);
        const hipError_t e = cvae_launch_coop(pn.k6, dim3(m.H / 8 * pn.rts), dim3(256), lds6, st, q);
        if (refused(e)) return fail(-3, "exact-operand recurrent kernel failed to launch: %s", hipGetErrorString(e));
        break;
    }
    case CVAE_EVAL_V5:
    case CVAE_EVAL_V4: {      // front-end + recurrence in one launch (no gx buffer, no GEMM launch), block = (16 hidden units) x (row tiles)
        Step3Params q;
        q.hbuf = hbuf; q.mtot = wl.mtot; q.wrec2 = P + pl.wrec2; q.cfold = P + pl.cfold;
        q.xnp = xnp; q.Tp = wl.Tp; q.Cp = m.Cp; q.bhn = P + pl.bhn; q.B = Brows; q.Bp = wl.Bp; q.H = m.H; q.T = T;
        q.flags = hflags; q.status = status;
        q.prof = step_prof;
        q.wyT = P + pl.wyT; q.dy = dy; q.Co = m.Co;
        q.rts = pn.rts;
        q.hs = ws + wl.hs; q.wrec_h = P + pl.wrec_h; q.xs = ws + wl.xs; q.xs_plane = wl.xs_plane;
        q.exp = (int)opt(OPT_EXP);   // measurement switches only
        const dim3 g(m.nch * pn.rts);
        if (form == CVAE_EVAL_V5) {   // v4 with the recurrent product as three fp16 MFMAs on (hi, lo) pairs
            q.afold2 = P + pl.afold_h;
            const size_t lds5 = lds2 + (size_t)4 * ((m.KFW + 1) / 2) * 6 * 256 * sizeof(float);
            if (!refused(cvae_launch_coop(pn.k5, g, dim3(256), lds5, st, q))) break;
        }
        q.afold2 = P + pl.afold3;     // v4: front-end weights in LDS, double-buffered h operands
        const size_t lds4 = lds2 + (size_t)4 * m.KFW * 3 * 256 * sizeof(float);
        if (!refused(cvae_launch_coop(pn.k4, g, dim3(256), lds4, st, q))) break;
        run_front_end_gemm(m, P, pl, xnp, gx, Brows, wl.Tp, st);
        form = CVAE_EVAL_V2;
    }
        [[fallthrough]];
    case CVAE_EVAL_V2: {      // the same block geometry behind the hoisted front-end GEMM
        Step2Params q;
        q.hbuf = hbuf; q.mtot = wl.mtot; q.wrec2 = P + pl.wrec2; q.gx = gx; q.gx_bstride = (long)wl.Tp * m.H3;
        q.bhn = P + pl.bhn; q.B = Brows; q.Bp = wl.Bp; q.H = m.H; q.T = T; q.flags = hflags; q.status = status;
        q.prof = step_prof;
        q.wyT = P + pl.wyT; q.dy = dy; q.Co = m.Co;
        if (!refused(cvae_launch_coop(m.H == 1024 ? k_gru_steps_v2<16> : k_gru_steps_v2<1>, dim3(m.nch, pn.rts), dim3(256), lds2, st, q))) break;
        form = generic_resident(m, cus) ? CVAE_EVAL_GENERIC : CVAE_EVAL_PER_STEP;
    }
        [[fallthrough]];
    default: {                // CVAE_EVAL_GENERIC, CVAE_EVAL_PER_STEP: the any-H kernel
        const size_t step_lds = 4 * 64 * 20 * sizeof(float);
        StepParams sp;
        sp.hbuf = hbuf; sp.mtot = wl.mtot; sp.wrec = P + pl.wrec; sp.gx = gx; sp.gx_bstride = (long)wl.Tp * m.H3;
        sp.bhn = P + pl.bhn; sp.B = Brows; sp.Bp = wl.Bp; sp.H = m.H; sp.T = T; sp.t0 = 0; sp.bar = bar; sp.status = status;
        sp.nwg = (unsigned)(m.H / 4);
        sp.prof = nullptr;
        sp.wyT = P + pl.wyT; sp.dy = dy; sp.Co = m.Co;
        if (form == CVAE_EVAL_GENERIC) {
            // (the barrier counter is zeroed here, where its only user is launched: a memset is a launch of its own)
            CVAE_HIP_OK(hipMemsetAsync(bar, 0, 8 * sizeof(unsigned), st));
            if (!refused(cvae_launch_coop(k_gru_steps<true>, dim3(sp.nwg), dim3(256), step_lds, st, sp))) break;
        }
        for (int t = 0; t < T; ++t) {
            sp.t0 = t;
            hipLaunchKernelGGL((k_gru_steps<false>), dim3(sp.nwg), dim3(256), step_lds, st, sp);
        }
    }
    }
    if (prof) prof_end(st);

    if (pn.proj == PROJ_V6) {
        Out6Params op;
        op.hx = ws + wl.hs; op.mtot = wl.mtot; op.wo3 = P + pl.wo3; op.bo2 = P + pl.bo2; op.H = m.H; op.Bp = wl.Bp; op.T = T;
        op.B = B; op.ncell = ncell; op.Co = m.Co; op.clamp_from = d->has_scale_out ? -1 : clamp_dim(clamp_lat_dim);
        op.clamp_min = clamp_floor(clamp_lat_dim);
        for (int c = 0; c < CVAE_MAX_CELLS; ++c) op.out[c] = c < ncell ? cells[c].trj_out : nullptr;
        const dim3 g((unsigned)((long)T * wl.Bp / 32), (unsigned)((m.Cop + 31) / 32));
        hipLaunchKernelGGL(pn.kout6, g, dim3(256), (size_t)4 * 32 * 36 * sizeof(float), st, op);
    } else {
        run_projection(m, d, P, pl, rows, pn.proj, hbuf, ws + wl.y, clamp_lat_dim, st);
    }
    run_last_states(m, rows, hbuf, st);
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

const char* cvae_last_error_string(void) { return g_err; }
int cvae_abi_version(void) { return CVAE_ABI_VERSION; }

cvae_ctx* cvae_ctx_create(void) {
    cvae_ctx* c = new (std::nothrow) cvae_ctx();
    if (!c) {
        (void)fail(-3, "out of memory");
        return nullptr;
    }
    for (int i = 0; i < OPT_COUNT; ++i) c->opt[i] = g_opt[i].dflt;
    c->range_serial = (int)(((uintptr_t)c >> 6) & 0x3fffffff);      // (two contexts do not count the calls on a workspace alike)
    return c;
}

int cvae_ctx_destroy(cvae_ctx* ctx) {
    if (!ctx) return 0;
    if (tl_ctx == ctx) return fail(-1, "cvae_ctx_destroy from inside a call on the same context");
    // the events the context created (profiling brackets, side-stream joins); the caller has synchronised whatever used them
    for (hipEvent_t e : ctx->prof.start) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->prof.stop) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->tprof.start) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->tprof.stop) (void)hipEventDestroy(e);
    for (SideDone& d : ctx->side_done)
        if (d.ev) (void)hipEventDestroy(d.ev);
    for (hipEvent_t e : {ctx->side_ready, ctx->side_join, ctx->side_last, ctx->mask_fork, ctx->mask_join})
        if (e) (void)hipEventDestroy(e);
    delete ctx;
    return 0;
}

int cvae_set_status_sink(cvae_ctx* ctx, int32_t* sink) {
    CVAE_ENTER(ctx);
    cx().status_sink = sink;
    return 0;
}

int cvae_set_draw_origin(cvae_ctx* ctx, int64_t row0, int64_t global_rows, int64_t frames_per_row) {
    CVAE_ENTER(ctx);
    if (row0 < 0 || global_rows < 0 || frames_per_row < 0 || (global_rows > 0 && row0 >= global_rows))
        return fail(-1, "bad draw origin: row0 %lld of %lld rows", (long long)row0, (long long)global_rows);
    cx().draw_row0 = (long)row0;
    cx().draw_rows = (long)global_rows;
    cx().draw_frames = (long)frames_per_row;
    return 0;
}

int cvae_selftest_limbs(cvae_ctx* ctx, const float* x, float* y, int64_t n, void* stream) {
    CVAE_ENTER(ctx);
    if (!x || !y || n < 0 || n % 8) return fail(-1, "selftest: n must be a non-negative multiple of 8");
    if (n) hipLaunchKernelGGL((k_selftest_limbs), dim3(nblk(n / 8, 256)), dim3(256), 0, (hipStream_t)stream, x, y, (long)n);
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

int cvae_selftest_occupy(cvae_ctx* ctx, int blocks, size_t lds_bytes, int64_t cycles, void* stream) {
    CVAE_ENTER(ctx);
    if (blocks < 1 || cycles < 0 || lds_bytes > 160 * 1024) return fail(-1, "selftest_occupy: bad argument");
    hipLaunchKernelGGL((k_selftest_occupy), dim3(blocks), dim3(256), lds_bytes, (hipStream_t)stream, (long long)cycles, (int)(lds_bytes / 4));
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

int cvae_set_option(cvae_ctx* ctx, const char* name, int64_t value) {
    CVAE_ENTER(ctx);
    if (!name) return fail(-1, "null option name");
    for (int i = 0; i < OPT_COUNT; ++i)
        if (!strcmp(g_opt[i].name, name)) {
            ctx->opt[i] = (long)value;
            return 0;
        }
    return fail(-1, "unknown option '%s'", name);
}

int cvae_get_option(cvae_ctx* ctx, const char* name, int64_t* value) {
    CVAE_ENTER(ctx);
    if (!name || !value) return fail(-1, "null argument");
    for (int i = 0; i < OPT_COUNT; ++i)
        if (!strcmp(g_opt[i].name, name)) {
            *value = ctx->opt[i];
            return 0;
        }
    return fail(-1, "unknown option '%s'", name);
}

int cvae_reset_options(cvae_ctx* ctx) {
    CVAE_ENTER(ctx);
    for (int i = 0; i < OPT_COUNT; ++i) ctx->opt[i] = g_opt[i].dflt;
    return 0;
}

int cvae_set_draw_parts(cvae_ctx* ctx, int32_t parts) {
    CVAE_ENTER(ctx);
    if (parts < 1) return fail(-1, "bad draw parts %d", (int)parts);
    cx().draw_parts = parts;
    return 0;
}

size_t cvae_net_prepared_bytes(cvae_ctx* ctx, const cvae_net_desc* d) {
    CVAE_ENTER_SZ(ctx);
    Dims m;
    if (make_dims(d, &m)) return 0;
    return (size_t)prep_layout(m, d->has_scale_in != 0, d->has_scale_out != 0).total * sizeof(float);
}

size_t cvae_net_prepare_scratch_bytes(cvae_ctx* ctx, const cvae_net_desc* d) {
    CVAE_ENTER_SZ(ctx);
    Dims m;
    if (make_dims(d, &m)) return 0;
    return (size_t)fold_scratch(m).total * sizeof(double);
}

int cvae_net_prepare(cvae_ctx* ctx, const cvae_net_desc* d, const cvae_net_weights* w, void* prepared, size_t prepared_bytes,
                     void* scratch, size_t scratch_bytes, void* stream) {
    CVAE_ENTER(ctx);
    Dims m;
    if (int rc = make_dims(d, &m)) return rc;
    if (!w || !prepared || !scratch) return fail(-1, "null argument");
    if (!w->conv0_w || !w->conv0_b || !w->w_ih || !w->w_hh || !w->b_ih || !w->b_hh || !w->out_w || !w->out_b)
        return fail(-1, "missing weight pointer");
    if ((m.layers >= 2 && (!w->conv1_w || !w->conv1_b)) || (m.layers >= 3 && (!w->conv2_w || !w->conv2_b)))
        return fail(-1, "missing conv weight pointer for layers=%d", m.layers);
    if (d->has_scale_in && (!w->scale_in_w || !w->scale_in_b)) return fail(-1, "has_scale_in without scale_in weights");
    if (d->has_scale_out && (!w->scale_out_w || !w->scale_out_b)) return fail(-1, "has_scale_out without scale_out weights");
    if (prepared_bytes < cvae_net_prepared_bytes(ctx, d)) return fail(-2, "prepared buffer too small");
    if (scratch_bytes < cvae_net_prepare_scratch_bytes(ctx, d)) return fail(-2, "prepare scratch too small");
    hipStream_t st = (hipStream_t)stream;
    const Prep pl = prep_layout(m, d->has_scale_in != 0, d->has_scale_out != 0);
    float* P = (float*)prepared;
    const FoldScratch fs = fold_scratch(m);
    double* mfull = (double*)scratch + fs.ma;      // where the last layer's fold lands
    double* bprime = (double*)scratch + fs.ba;
    int* unfit = (int*)(P + pl.range);      // raised by the kernels that write limb images (cleared with the image, just below)
    cx().image_unfit.erase((const void*)P);

    CVAE_HIP_OK(hipMemsetAsync(P, 0, (size_t)pl.total * sizeof(float), st));
    {   // the fold, layer by layer (fp64; the one rounding to fp32 happens in k_prep_afold / k_prep_cfold)
        const float* const cw_[3] = {w->conv0_w, w->conv1_w, w->conv2_w};
        const float* const cb_[3] = {w->conv0_b, w->conv1_b, w->conv2_b};
        double* const sc = (double*)scratch;
        for (int n = 0; n < m.layers; ++n) {
            const bool in_a = (m.layers - 1 - n) % 2 == 0;
            double* mn = sc + (in_a ? fs.ma : fs.mb);
            double* bn = sc + (in_a ? fs.ba : fs.bb);
            const double* mp = sc + (in_a ? fs.mb : fs.ma);
            const double* bp = sc + (in_a ? fs.bb : fs.ba);
            if (n == 0) {
                hipLaunchKernelGGL((k_prep_fold0), dim3(nblk(fold_m_size(m, 0), 256)), dim3(256), 0, st, cw_[0], cb_[0], mn, bn, m.C, m.ks);
            } else {
                const int cp = m.cl[n - 1], rp = cp / m.C;
                hipLaunchKernelGGL((k_prep_fold_m), dim3(nblk(fold_m_size(m, n), 256)), dim3(256), 0, st, cw_[n], mp, mn, m.C, m.ks, cp, rp);
                hipLaunchKernelGGL((k_prep_fold_b), dim3(nblk(m.cl[n], 128)), dim3(128), 0, st, bp, cw_[n], cb_[n], bn, m.ks, cp);
            }
        }
    }
    hipLaunchKernelGGL((k_prep_afold), dim3(nblk((long)m.H3 * m.Kfe, 256)), dim3(256), 0, st, w->w_ih,
                       (const double*)mfull, P + pl.afold, m.C, m.Cp, m.R, m.tot, m.Kfe, m.H3);
    hipLaunchKernelGGL((k_prep_afold_h), dim3(nblk((long)m.nch * 4 * ((m.KFW + 1) / 2) * 3 * 512, 256)), dim3(256), 0, st,
                       (const float*)(P + pl.afold), P + pl.afold_h, m.H, m.Kfe, (m.KFW + 1) / 2, unfit);
    hipLaunchKernelGGL((k_prep_afold3), dim3(nblk((long)m.nch * 4 * m.KFW * 3 * 256, 256)), dim3(256), 0, st,
                       (const float*)(P + pl.afold), P + pl.afold3, m.H, m.Kfe, m.KFW);
    hipLaunchKernelGGL((k_prep_cfold), dim3(nblk(m.H3, 128)), dim3(128), 0, st, w->w_ih, w->b_ih, w->b_hh, w->out_b,
                       (const double*)bprime, P + pl.cfold, m.cw, m.Co, m.tot, m.H);
    hipLaunchKernelGGL((k_prep_wrec), dim3(nblk((long)(m.H / 4) * m.nch * 256, 256)), dim3(256), 0, st, w->w_ih, w->w_hh,
                       w->out_w, P + pl.wrec, m.cw, m.Co, m.tot, m.H);
    auto copy2d = [&](float* dst, long dld, const float* src, long sld, int rows, int cols) {
        hipLaunchKernelGGL((k_copy2d), dim3(nblk((long)rows * cols, 256)), dim3(256), 0, st, dst, dld, src, sld, rows, cols);
    };
    hipLaunchKernelGGL((k_prep_wrec2), dim3(nblk((long)m.nch * 4 * m.nch * 256, 256)), dim3(256), 0, st, w->w_ih, w->w_hh,
                       w->out_w, P + pl.wrec2, m.cw, m.Co, m.tot, m.H);
    if (m.H % 32 == 0)
        hipLaunchKernelGGL((k_prep_wrec_h), dim3(nblk((long)m.nch * 4 * (m.H / 32) * 512, 256)), dim3(256), 0, st,
                           (const float*)(P + pl.wrec2), P + pl.wrec_h, m.H, unfit);
    if (exact3_ok(m)) {
        hipLaunchKernelGGL((k_prep_wrec3), dim3(nblk((long)(m.H / 8) * 4 * exact3_kpw(m) * 512, 256)), dim3(256), 0, st,
                           (const float*)(P + pl.wrec2), P + pl.wrec_t, m.H, exact3_kpw(m), unfit);
        if (exact3_fused(m))
            hipLaunchKernelGGL((k_prep_afold3l), dim3(nblk((long)(m.H / 8) * 4 * m.KFW * 512, 256)), dim3(256), 0, st,
                               (const float*)(P + pl.afold), P + pl.afold_t, m.H, m.Kfe, m.KFW, unfit);
        hipLaunchKernelGGL((k_prep_wrec3_l2b), dim3(nblk((long)(m.H / 8) * 4 * exact3_kpw(m) * 512, 256)), dim3(256), 0, st,
                           (const float*)(P + pl.wrec2), (unsigned char*)(P + pl.wrec_l2b), m.H, exact3_kpw(m));
    }
    copy2d(P + pl.bhn, m.H, w->b_hh + 2 * m.H, m.H, 1, m.H);
    hipLaunchKernelGGL((k_copy2d_t), dim3(nblk((long)m.H3 * m.Co, 256)), dim3(256), 0, st, P + pl.wyT, w->w_ih + m.cw,
                       (long)m.tot, m.H3, m.Co);
    copy2d(P + pl.wo, m.H, w->out_w, m.H, m.Co, m.H);
    copy2d(P + pl.bo, m.Co, w->out_b, m.Co, 1, m.Co);
    hipLaunchKernelGGL((k_prep_wo2), dim3(nblk((long)m.Cop * m.H + m.Cop, 256)), dim3(256), 0, st, w->out_w, w->out_b,
                       d->has_scale_out ? w->scale_out_w : (const float*)nullptr,
                       d->has_scale_out ? w->scale_out_b : (const float*)nullptr, P + pl.wo2, P + pl.bo2, m.Co, m.Cop, m.H);
    if (exact3_ok(m))
        hipLaunchKernelGGL((k_prep_wo3), dim3(nblk((long)((m.Cop + 31) / 32) * (m.H / 16) * 512, 256)), dim3(256), 0, st,
                           (const float*)(P + pl.wo2), P + pl.wo3, m.H, m.Cop, (m.Cop + 31) / 32, unfit);
    if (d->has_scale_in) {
        copy2d(P + pl.sin_w, m.C, w->scale_in_w, m.C, m.C, m.C);
        copy2d(P + pl.sin_b, m.C, w->scale_in_b, m.C, 1, m.C);
    }
    if (d->has_scale_out) {
        copy2d(P + pl.sout_w, m.Co, w->scale_out_w, m.Co, m.Co, m.Co);
        copy2d(P + pl.sout_b, m.Co, w->scale_out_b, m.Co, 1, m.Co);
    }
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

size_t cvae_pass_workspace_bytes(cvae_ctx* ctx, const cvae_net_desc* d, int B, int T) {
    CVAE_ENTER_SZ(ctx);
    Dims m;
    if (make_dims(d, &m) || B < 1 || T < 1) return 0;
    return (size_t)work_layout(m, B, T).total * sizeof(float);
}

int cvae_plan_pass(cvae_ctx* ctx, const cvae_net_desc* d, int rows, int T, int flags) {
    CVAE_ENTER(ctx);
    Dims m;
    if (int rc = make_dims(d, &m)) return rc;
    if (rows < 1 || T < 1) return fail(-1, "bad sizes: rows=%d T=%d", rows, T);
    return plan_eval_pass(m, rows, T, flags, cu_count(), false, PassFacts{}).form;
}

int cvae_gru_rnn_forward(cvae_ctx* ctx, const cvae_net_desc* d, const void* prepared, const cvae_pass_input* in, const float* y_in,
                         const float* h_in, int B, int T, int clamp_lat_dim, float* trj_out, float* y_last,
                         float* h_last, void* workspace, size_t workspace_bytes, int flags, void* stream) {
    CVAE_ENTER(ctx);
    Dims m;
    if (int rc = make_dims(d, &m)) return rc;
    if (B < 1 || T < 1) return fail(-1, "empty batch: B=%d T=%d", B, T);
    if (!prepared || !in || !y_in || !trj_out || !workspace) return fail(-1, "null argument");
    if (!in->seg0.ptr || (in->seg1.width > 0 && !in->lat && !in->seg1.ptr)) return fail(-1, "null input segment");
    if (workspace_bytes < cvae_pass_workspace_bytes(ctx, d, B, T)) return fail(-2, "workspace too small");
    const Cell cell{in, y_in, h_in, trj_out, y_last, h_last};
    return run_pass(m, d, (const float*)prepared, &cell, 1, B, T, clamp_lat_dim, (float*)workspace, (int*)workspace,
                    flags, (hipStream_t)stream, true);
}

int cvae_gru_rnn_forward_stacked(cvae_ctx* ctx, const cvae_net_desc* d, const void* prepared, int ncell, const cvae_pass_input* in,
                                 const float* const* y_in, int B, int T, int clamp_lat_dim, float* const* trj_out,
                                 void* workspace, size_t workspace_bytes, int flags, void* stream) {
    CVAE_ENTER(ctx);
    Dims m;
    if (int rc = make_dims(d, &m)) return rc;
    if (B < 1 || T < 1 || ncell < 1 || ncell > CVAE_MAX_CELLS) return fail(-1, "bad sizes: ncell=%d B=%d T=%d", ncell, B, T);
    if (!prepared || !in || !y_in || !trj_out || !workspace) return fail(-1, "null argument");
    if (workspace_bytes < cvae_pass_workspace_bytes(ctx, d, ncell * B, T)) return fail(-2, "workspace too small");
    Cell cells[CVAE_MAX_CELLS];
    for (int c = 0; c < ncell; ++c) {
        if (!in[c].seg0.ptr || (in[c].seg1.width > 0 && !in[c].lat && !in[c].seg1.ptr) || !y_in[c] || !trj_out[c])
            return fail(-1, "cell %d: null pointer", c);
        cells[c] = Cell{&in[c], y_in[c], nullptr, trj_out[c], nullptr, nullptr};
    }
    return run_pass(m, d, (const float*)prepared, cells, ncell, B, T, clamp_lat_dim, (float*)workspace, (int*)workspace, flags,
                    (hipStream_t)stream, true);
}

int cvae_gru_rnn_forward_stacked_carry(cvae_ctx* ctx, const cvae_net_desc* d, const void* prepared, int ncell, const cvae_pass_input* in,
                                       const float* const* y_in, const float* const* h_in, int B, int T, int clamp_lat_dim,
                                       float* const* trj_out, float* const* h_last, void* workspace, size_t workspace_bytes,
                                       int flags, void* stream) {
    CVAE_ENTER(ctx);
    Dims m;
    if (int rc = make_dims(d, &m)) return rc;
    if (B < 1 || T < 1 || ncell < 1 || ncell > CVAE_MAX_CELLS) return fail(-1, "bad sizes: ncell=%d B=%d T=%d", ncell, B, T);
    if (!prepared || !in || !y_in || !trj_out || !workspace) return fail(-1, "null argument");
    if (workspace_bytes < cvae_pass_workspace_bytes(ctx, d, ncell * B, T)) return fail(-2, "workspace too small");
    Cell cells[CVAE_MAX_CELLS];
    for (int c = 0; c < ncell; ++c) {
        const float* hi = h_in ? h_in[c] : nullptr;
        if (!in[c].seg0.ptr || (in[c].seg1.width > 0 && !in[c].lat && !in[c].seg1.ptr) || !trj_out[c])
            return fail(-1, "cell %d: null pointer", c);
        if (!y_in[c] && !hi) return fail(-1, "cell %d: no y_in and no state to continue from", c);
        cells[c] = Cell{&in[c], y_in[c], hi, trj_out[c], nullptr, h_last ? h_last[c] : nullptr};
    }
    return run_pass(m, d, (const float*)prepared, cells, ncell, B, T, clamp_lat_dim, (float*)workspace, (int*)workspace, flags,
                    (hipStream_t)stream, true);
}

int cvae_sample(cvae_ctx* ctx, const float* lat, int rows, int lat_dim, const float* eps, uint64_t seed, uint64_t draw_id, float* z,
                float* eps_out, void* stream) {
    CVAE_ENTER(ctx);
    if (!lat || !z || rows < 0 || lat_dim < 1) return fail(-1, "bad argument");
    if (rows == 0) return 0;
    hipLaunchKernelGGL((k_sample), dim3(nblk((long)rows * lat_dim, 256)), dim3(256), 0, (hipStream_t)stream, lat, rows,
                       lat_dim, eps, seed, draw_id, z, eps_out, (uint64_t)cx().draw_row0 * (uint64_t)cx().draw_frames);
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

int cvae_sample_laplace(cvae_ctx* ctx, const float* lat, int rows, int lat_dim, const float* eps, uint64_t seed, uint64_t draw_id,
                        float* z, float* eps_out, void* stream) {
    CVAE_ENTER(ctx);
    if (!lat || !z || rows < 0 || lat_dim < 1) return fail(-1, "bad argument");
    if (rows == 0) return 0;
    hipLaunchKernelGGL((k_sample_laplace), dim3(nblk((long)rows * lat_dim, 256)), dim3(256), 0, (hipStream_t)stream, lat, rows,
                       lat_dim, eps, seed, draw_id, z, eps_out, (uint64_t)cx().draw_row0 * (uint64_t)cx().draw_frames);
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

int cvae_sample_laplace_backward(cvae_ctx* ctx, const float* dz, const float* lat, const float* z, int rows, int lat_dim, float* dlat,
                                 void* stream) {
    CVAE_ENTER(ctx);
    if (!dz || !lat || !z || !dlat || rows < 0 || lat_dim < 1) return fail(-1, "bad argument");
    if (rows == 0) return 0;
    hipLaunchKernelGGL((k_sample_laplace_bwd), dim3(nblk((long)rows * lat_dim, 256)), dim3(256), 0, (hipStream_t)stream, dz, lat, z,
                       rows, lat_dim, dlat);
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

// cycle workspace = [status 64 floats][per-pass workspace (max of enc/dec)][5 trajectories for the cycle in flight]
static long cycle_layout(const Dims& me, const Dims& md, int B, int T, long* pass_off, long* traj_off) {
    const long pe = work_layout(me, B, T).total, pd = work_layout(md, 2 * B, T).total;
    long o = 64;
    *pass_off = o;
    o += pe > pd ? pe : pd;
    *traj_off = o;
    o += up((long)B * T * me.Co, 64) * 2 + up((long)B * T * md.Co, 64) * 3;
    return o;
}

size_t cvae_cycle_workspace_bytes(cvae_ctx* ctx, const cvae_net_desc* enc, const cvae_net_desc* dec, int B, int T, int n_cyc) {
    CVAE_ENTER_SZ(ctx);
    Dims me, md;
    if (make_dims(enc, &me) || make_dims(dec, &md) || B < 1 || T < 1 || n_cyc < 1) return 0;
    long po, to;
    return (size_t)cycle_layout(me, md, B, T, &po, &to) * sizeof(float);
}

static int cycle_forward_impl(const cvae_net_desc* enc, const void* enc_prepared, const cvae_net_desc* dec,
                       const void* dec_prepared, const float* x, const float* cvx, int stdim, const float* code_src,
                       const float* code_trg, int ncode, const float* y_in_enc, const float* y_in_dec, int B, int T,
                       int n_cyc, int lat_dim_arg, const float* eps, uint64_t seed, float* out_lat, float* out_rec,
                       float* out_cv, float* out_latcv, float* out_reccyc, void* workspace, size_t workspace_bytes,
                       int flags, void* stream, const cvae_cycle_state* sin, const cvae_cycle_state* sout,
                       long cvx_cycle_stride, long code_trg_cycle_stride) {
    // cvx_cycle_stride / code_trg_cycle_stride (elements): cycle i reads cvx + i * stride and code_trg + i * stride -- the per-cycle
    // converted excitation and target codes of the many-to-many recipes; 0 = one tensor for every cycle (the pointers of before)
    // lat_dim_arg: L, or L | CVAE_DRAW_LAPLACE -- the three draws of a cycle are then Laplace draws (the flag travels in the decoder
    // passes' cvae_pass_input.lat_dim) and the encoder passes clamp at the Laplace floor
    const int lat_dim = draw_dim(lat_dim_arg);
    const int enc_clamp = draw_laplace(lat_dim_arg) ? (lat_dim | CVAE_CLAMP_LAPLACE) : lat_dim;
    Dims me, md;
    if (int rc = make_dims(enc, &me)) return rc;
    if (int rc = make_dims(dec, &md)) return rc;
    if (B < 1 || T < 1 || n_cyc < 1) return fail(-1, "empty work: B=%d T=%d n_cyc=%d", B, T, n_cyc);
    if (!enc_prepared || !dec_prepared || !x || !cvx || !code_src || !code_trg || !y_in_enc || !y_in_dec || !workspace)
        return fail(-1, "null argument");
    if (me.Co != 2 * lat_dim) return fail(-1, "encoder out_dim %d != 2*lat_dim %d", me.Co, 2 * lat_dim);
    if (md.C != ncode + lat_dim) return fail(-1, "decoder in_dim %d != ncode+lat_dim %d", md.C, ncode + lat_dim);
    if (me.C != stdim + md.Co) return fail(-1, "encoder in_dim %d != stdim+decoder out_dim %d", me.C, stdim + md.Co);
    // a cycle stride is 0 or reaches over at least one cycle's [B, T, width] block: slices never overlap
    if (cvx_cycle_stride < 0 || (cvx_cycle_stride > 0 && cvx_cycle_stride < (long)B * T * stdim))
        return fail(-1, "cvx_cycle_stride %ld: must be 0 or at least B*T*stdim = %ld", cvx_cycle_stride, (long)B * T * stdim);
    if (code_trg_cycle_stride < 0 || (code_trg_cycle_stride > 0 && code_trg_cycle_stride < (long)B * T * ncode))
        return fail(-1, "code_trg_cycle_stride %ld: must be 0 or at least B*T*ncode = %ld", code_trg_cycle_stride, (long)B * T * ncode);
    if (workspace_bytes < cvae_cycle_workspace_bytes(tl_ctx, enc, dec, B, T, n_cyc)) return fail(-2, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    long po, to;
    cycle_layout(me, md, B, T, &po, &to);
    float* pws = ws + po;
    const long ne = (long)B * T * me.Co, nd = (long)B * T * md.Co;
    float* t_lat = ws + to;
    float* t_latcv = t_lat + up(ne, 64);
    float* t_rec = t_latcv + up(ne, 64);
    float* t_cv = t_rec + up(nd, 64);
    float* t_reccyc = t_cv + up(nd, 64);
    const float* prev_reccyc = nullptr;
    int* status = (int*)workspace;
    const long neps = (long)B * T * lat_dim;
    if (sin && (!sin->y_enc || !sin->y_dec || !sin->h_enc || !sin->h_dec)) return fail(-1, "incomplete input cycle state");
    if (sout && (!sout->y_enc || !sout->y_dec || !sout->h_enc || !sout->h_dec)) return fail(-1, "incomplete output cycle state");
    // state of pass `slot` (encoder: 0 lat, 1 latcv; decoder: 0 rec, 1 cv, 2 reccyc) of cycle i
    auto ye = [&](const cvae_cycle_state* s, int i, int slot) { return s ? s->y_enc + ((long)i * 2 + slot) * B * me.Co : nullptr; };
    auto he = [&](const cvae_cycle_state* s, int i, int slot) { return s ? s->h_enc + ((long)i * 2 + slot) * B * me.H : nullptr; };
    auto yd = [&](const cvae_cycle_state* s, int i, int slot) { return s ? s->y_dec + ((long)i * 3 + slot) * B * md.Co : nullptr; };
    auto hd = [&](const cvae_cycle_state* s, int i, int slot) { return s ? s->h_dec + ((long)i * 3 + slot) * B * md.H : nullptr; };

    for (int i = 0; i < n_cyc; ++i) {
        float* lat = out_lat ? out_lat + i * ne : t_lat;
        float* latcv = out_latcv ? out_latcv + i * ne : t_latcv;
        float* rec = out_rec ? out_rec + i * nd : t_rec;
        float* cv = out_cv ? out_cv + i * nd : t_cv;
        // rec_cyc of cycle i feeds cycle i+1's encoder, which has consumed it before this cycle's last pass rewrites it
        float* reccyc = out_reccyc ? out_reccyc + i * nd : t_reccyc;
        cvae_pass_input in, in2;
        memset(&in, 0, sizeof(in));
        int rc;
        // lat = E(x) or E([x[:,:,:stdim] ; rec_cyc_{i-1}])      (train...:1334 / :1328)
        if (i == 0) {
            in.seg0 = cvae_seg{x, me.C, me.C};
        } else {
            in.seg0 = cvae_seg{x, stdim, me.C};
            in.seg1 = cvae_seg{prev_reccyc, md.Co, md.Co};
        }
        {
            const Cell c{&in, sin ? ye(sin, i, 0) : y_in_enc, he(sin, i, 0), lat, ye(sout, i, 0), he(sout, i, 0)};
            if ((rc = run_pass(me, enc, (const float*)enc_prepared, &c, 1, B, T, enc_clamp, pws, status, flags, st, i == 0))) return rc;
        }
        // rec = D([code_src ; z1]) and cv = D([code_trg[i] ; z2]) share the decoder and do not depend on each other
        // (train...:1335-1336): one stacked pass, 2B rows
        memset(&in, 0, sizeof(in));
        in.seg0 = cvae_seg{code_src, ncode, ncode};
        in.lat = lat; in.lat_dim = lat_dim_arg;
        in.eps = eps ? eps + (i * 3 + 0) * neps : nullptr;
        in.seed = seed; in.draw_id = (uint64_t)(i * 3 + 0);
        in2 = in;
        in2.seg0 = cvae_seg{code_trg + (long)i * code_trg_cycle_stride, ncode, ncode};
        in2.eps = eps ? eps + (i * 3 + 1) * neps : nullptr;
        in2.draw_id = (uint64_t)(i * 3 + 1);
        {
            const Cell c2[2] = {{&in, sin ? yd(sin, i, 0) : y_in_dec, hd(sin, i, 0), rec, yd(sout, i, 0), hd(sout, i, 0)},
                                {&in2, sin ? yd(sin, i, 1) : y_in_dec, hd(sin, i, 1), cv, yd(sout, i, 1), hd(sout, i, 1)}};
            if ((rc = run_pass(md, dec, (const float*)dec_prepared, c2, 2, B, T, -1, pws, status, flags, st))) return rc;
        }
        // latcv = E([cvx[i] ; cv])                                (train...:1337)
        memset(&in, 0, sizeof(in));
        in.seg0 = cvae_seg{cvx + (long)i * cvx_cycle_stride, stdim, stdim};
        in.seg1 = cvae_seg{cv, md.Co, md.Co};
        {
            const Cell c{&in, sin ? ye(sin, i, 1) : y_in_enc, he(sin, i, 1), latcv, ye(sout, i, 1), he(sout, i, 1)};
            if ((rc = run_pass(me, enc, (const float*)enc_prepared, &c, 1, B, T, enc_clamp, pws, status, flags, st))) return rc;
        }
        // rec_cyc = D([code_src ; z3])                            (train...:1338)
        memset(&in, 0, sizeof(in));
        in.seg0 = cvae_seg{code_src, ncode, ncode};
        in.lat = latcv; in.lat_dim = lat_dim_arg;
        in.eps = eps ? eps + (i * 3 + 2) * neps : nullptr;
        in.seed = seed; in.draw_id = (uint64_t)(i * 3 + 2);
        {
            const Cell c{&in, sin ? yd(sin, i, 2) : y_in_dec, hd(sin, i, 2), reccyc, yd(sout, i, 2), hd(sout, i, 2)};
            if ((rc = run_pass(md, dec, (const float*)dec_prepared, &c, 1, B, T, -1, pws, status, flags, st))) return rc;
        }
        prev_reccyc = reccyc;
    }
    return 0;
}

int cvae_cycle_forward_m2m(cvae_ctx* ctx, const cvae_net_desc* enc, const void* enc_prepared, const cvae_net_desc* dec,
                           const void* dec_prepared, const float* x, const float* cvx, int stdim, const float* code_src,
                           const float* code_trg, int ncode, const float* y_in_enc, const float* y_in_dec, int B, int T,
                           int n_cyc, int lat_dim, const float* eps, uint64_t seed, float* out_lat, float* out_rec,
                           float* out_cv, float* out_latcv, float* out_reccyc, void* workspace, size_t workspace_bytes,
                           int flags, void* stream, const cvae_cycle_state* state_in, const cvae_cycle_state* state_out,
                           int64_t cvx_cycle_stride, int64_t code_trg_cycle_stride) {
    CVAE_ENTER(ctx);
    return cycle_forward_impl(enc, enc_prepared, dec, dec_prepared, x, cvx, stdim, code_src, code_trg, ncode, y_in_enc, y_in_dec,
                              B, T, n_cyc, lat_dim, eps, seed, out_lat, out_rec, out_cv, out_latcv, out_reccyc, workspace,
                              workspace_bytes, flags, stream, state_in, state_out, (long)cvx_cycle_stride,
                              (long)code_trg_cycle_stride);
}

int cvae_cycle_forward(cvae_ctx* ctx, const cvae_net_desc* enc, const void* enc_prepared, const cvae_net_desc* dec,
                       const void* dec_prepared, const float* x, const float* cvx, int stdim, const float* code_src,
                       const float* code_trg, int ncode, const float* y_in_enc, const float* y_in_dec, int B, int T,
                       int n_cyc, int lat_dim, const float* eps, uint64_t seed, float* out_lat, float* out_rec,
                       float* out_cv, float* out_latcv, float* out_reccyc, void* workspace, size_t workspace_bytes,
                       int flags, void* stream) {
    return cvae_cycle_forward_m2m(ctx, enc, enc_prepared, dec, dec_prepared, x, cvx, stdim, code_src, code_trg, ncode, y_in_enc,
                                  y_in_dec, B, T, n_cyc, lat_dim, eps, seed, out_lat, out_rec, out_cv, out_latcv, out_reccyc,
                                  workspace, workspace_bytes, flags, stream, nullptr, nullptr, 0, 0);
}

int cvae_cycle_forward_carry(cvae_ctx* ctx, const cvae_net_desc* enc, const void* enc_prepared, const cvae_net_desc* dec,
                             const void* dec_prepared, const float* x, const float* cvx, int stdim, const float* code_src,
                             const float* code_trg, int ncode, const float* y_in_enc, const float* y_in_dec, int B, int T,
                             int n_cyc, int lat_dim, const float* eps, uint64_t seed, float* out_lat, float* out_rec,
                             float* out_cv, float* out_latcv, float* out_reccyc, void* workspace, size_t workspace_bytes,
                             int flags, void* stream, const cvae_cycle_state* state_in, const cvae_cycle_state* state_out) {
    return cvae_cycle_forward_m2m(ctx, enc, enc_prepared, dec, dec_prepared, x, cvx, stdim, code_src, code_trg, ncode, y_in_enc,
                                  y_in_dec, B, T, n_cyc, lat_dim, eps, seed, out_lat, out_rec, out_cv, out_latcv, out_reccyc,
                                  workspace, workspace_bytes, flags, stream, state_in, state_out, 0, 0);
}

int cvae_step_timing(cvae_ctx* ctx, const cvae_net_desc* d, int B, int T, const void* workspace, double out[8], void* stream) {
    CVAE_ENTER(ctx);
    Dims m;
    if (int rc = make_dims(d, &m)) return rc;
    if (!workspace || !out || B < 1 || T < 1) return fail(-1, "bad argument");
    const Work wl = work_layout(m, B, T);
    // one counter block per workgroup of the tuned kernel the documented flags select (the 16-row dataflow kernels; k_gru_steps_v6
    // launches as many at H = 1024), as far as the workspace's counter area reaches
    const EvalPlan pn = plan_eval_pass(m, B, T, CVAE_FLAG_PERSISTENT, cu_count(), false, PassFacts{});
    const int nwg = pn.rts < 1 ? 1 : (m.nch * pn.rts > wl.prof_blocks ? wl.prof_blocks : m.nch * pn.rts);
    std::vector<long long> h((size_t)nwg * 4);
    CVAE_HIP_OK(hipMemcpyAsync(h.data(), (const float*)workspace + wl.prof, h.size() * sizeof(long long),
                               hipMemcpyDeviceToHost, (hipStream_t)stream));
    CVAE_HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    for (int q = 0; q < 4; ++q) {
        double sum = 0, mx = 0;
        for (int g = 0; g < nwg; ++g) {
            const double v = (double)h[(size_t)g * 4 + q];
            sum += v;
            mx = v > mx ? v : mx;
        }
        out[q] = sum / nwg;
        out[4 + q] = mx;
    }
    return 0;
}

int cvae_profile_collect_launches(cvae_ctx* ctx, double* ms, int* rows, int* cin, int cap) {
    CVAE_ENTER(ctx);
    const int n = (int)cx().prof.used < cap ? (int)cx().prof.used : cap;
    for (int i = 0; i < n; ++i) {
        float t = 0.f;
        CVAE_HIP_OK(hipEventSynchronize(cx().prof.stop[i]));
        CVAE_HIP_OK(hipEventElapsedTime(&t, cx().prof.start[i], cx().prof.stop[i]));
        if (ms) ms[i] = t;
        if (rows) rows[i] = cx().prof.rows[i];
        if (cin) cin[i] = cx().prof.cin[i];
    }
    cx().prof.used = 0;
    return n;
}

int cvae_profile_collect(cvae_ctx* ctx, double* total_ms, int* launches) {
    CVAE_ENTER(ctx);
    double tot = 0.0;
    for (size_t i = 0; i < cx().prof.used; ++i) {
        float ms = 0.f;
        CVAE_HIP_OK(hipEventSynchronize(cx().prof.stop[i]));
        CVAE_HIP_OK(hipEventElapsedTime(&ms, cx().prof.start[i], cx().prof.stop[i]));
        tot += ms;
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = (int)cx().prof.used;
    cx().prof.used = 0;
    return 0;
}

int cvae_train_profile_collect(cvae_ctx* ctx, double total_ms[4], int launches[4], double flop[4]) {
    CVAE_ENTER(ctx);
    for (int c = 0; c < TPROF_CLASSES; ++c) {
        if (total_ms) total_ms[c] = 0.0;
        if (launches) launches[c] = 0;
        if (flop) flop[c] = 0.0;
    }
    for (size_t i = 0; i < cx().tprof.used; ++i) {
        float ms = 0.f;
        CVAE_HIP_OK(hipEventSynchronize(cx().tprof.stop[i]));
        CVAE_HIP_OK(hipEventElapsedTime(&ms, cx().tprof.start[i], cx().tprof.stop[i]));
        const int c = cx().tprof.cls[i];
        if (total_ms) total_ms[c] += ms;
        if (launches) launches[c] += 1;
        if (flop) flop[c] += cx().tprof.flop[i];
    }
    cx().tprof.used = 0;
    return 0;
}

int cvae_workspace_status(cvae_ctx* ctx, const void* workspace, int32_t status_out[4], void* stream) {
    CVAE_ENTER(ctx);
    if (!workspace || !status_out) return fail(-1, "null argument");
    int32_t w[CVAE_WS_RANGE_EPOCH + 1];
    CVAE_HIP_OK(hipMemcpyAsync(w, workspace, sizeof(w), hipMemcpyDeviceToHost, (hipStream_t)stream));
    CVAE_HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    for (int i = 0; i < 4; ++i) status_out[i] = w[i];
    // the range word of the workspace holds the serial number of the call that raised it: only the latest call's counts (ProParams)
    status_out[CVAE_STATUS_RANGE_WORD] = w[CVAE_WS_RANGE_WORD] != 0 && w[CVAE_WS_RANGE_WORD] == w[CVAE_WS_RANGE_EPOCH] ? CVAE_STATUS_RANGE : 0;
    return 0;
}

int cvae_net_prepared_in_range(cvae_ctx* ctx, const cvae_net_desc* d, int n_layers, const void* prepared, void* stream) {
    CVAE_ENTER(ctx);
    Dims m;
    if (int rc = make_dims(d, &m)) return rc;
    if (n_layers < 1 || !prepared) return fail(-1, "bad argument");
    const Prep pl = prep_layout(m, d->has_scale_in != 0, d->has_scale_out != 0);
    int32_t flag = 0;
    CVAE_HIP_OK(hipMemcpyAsync(&flag, (const float*)prepared + pl.range, sizeof(flag), hipMemcpyDeviceToHost, (hipStream_t)stream));
    CVAE_HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    if (cx().image_unfit.size() >= 4096) cx().image_unfit.clear();      // (addresses of images long gone)
    if (flag != 0) cx().image_unfit[prepared] = true;
    else cx().image_unfit.erase(prepared);
    return flag != 0 ? 0 : 1;
}

}  // extern "C"

#include "cvae_train.inc"
#include "cvae_stage4.inc"
#include "cvae_stage6.inc"
#include "cvae_validation.inc"
#include "cvae_stage5.inc"
#include "cvae_decode.inc"
#include "cvae_trainlog.inc"
#include "cvae_deep.inc"
#include "cvae_stream.inc"
