/*
 * cyclevae_hip.h -- C ABI of libcyclevae_hip.so: the CycleVAE-VC encoder -> latent -> decoder hot path
 * as hand-written HIP kernels for gfx950 (MI355X).
 *
 * The reference (patrickltobing/cyclevae-vc) has no FFI: its boundary for this path is the Python module
 * src/nets/gru_vae.py, found through PYTHONPATH (egs/one-to-one/path.sh:11).  The drop-in module
 * cyclevae-vc_amd/gru_vae.py keeps that module's names and binds the entry points below with ctypes
 * (see INTEGRATION.md).  Each entry point states the reference lines it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous float32 unless stated; shapes in comments
 *   - the caller owns all memory, including the `prepared` weight image and the `workspace`;
 *     the library allocates nothing and keeps no global state besides a thread-local error string and the process-wide
 *     settings of cvae_set_status_sink / cvae_set_draw_origin / cvae_set_draw_parts / cvae_set_side_stream / cvae_set_option;
 *     it reads NO environment variable
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); nothing synchronises the device
 *   - return value: 0 = ok, negative = error (cvae_last_error_string() describes it); never throws
 *   - hidden size must be a multiple of 16; kernel_size odd; conv layers (reference `dilation_size`) 1, 2 or 3 (ABI 10; 3 with
 *     kernel_size 3 only: the receptive field kernel_size^layers stays below 125 frames -- and with hidden % 64 == 0 only);
 *     training: layers == 2
 */
#ifndef CYCLEVAE_HIP_H
#define CYCLEVAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CVAE_ABI_VERSION 10

/* Shape of one reference GRU_RNN (src/nets/gru_vae.py:282-320). */
typedef struct cvae_net_desc {
    int32_t in_dim;        /* Cin                                   */
    int32_t out_dim;       /* Cout (encoder: 2*lat_dim)             */
    int32_t hidden;        /* H, multiple of 16                     */
    int32_t kernel_size;   /* 3 in the recipe                       */
    int32_t layers;        /* reference `dilation_size`: 1, 2 or 3  */
    int32_t has_scale_in;  /* scale_in_flag  (gru_vae.py:296-297)   */
    int32_t has_scale_out; /* scale_out_flag (gru_vae.py:317-318)   */
} cvae_net_desc;

/* Raw weights in the reference's state_dict layout; NULL where the layer is absent.  Conv layer n (0-based, n <
 * layers) maps ks^n*Cin channels to ks^(n+1)*Cin with dilation ks^n; W_ih sees the last layer's ks^layers*Cin channels + Cout.
 * conv1_* may be NULL for layers == 1; conv2_* (ABI 10, at the end of the struct) are NULL unless layers == 3. */
typedef struct cvae_net_weights {
    const float* scale_in_w;  /* scale_in.weight      [Cin,Cin,1]        */
    const float* scale_in_b;  /* scale_in.bias        [Cin]              */
    const float* conv0_w;     /* conv.conv.0.weight   [ks*Cin,Cin,ks]    */
    const float* conv0_b;     /* conv.conv.0.bias     [ks*Cin]           */
    const float* conv1_w;     /* conv.conv.1.weight   [ks^2*Cin,ks*Cin,ks] */
    const float* conv1_b;     /* conv.conv.1.bias     [ks^2*Cin]         */
    const float* w_ih;        /* gru.weight_ih_l0     [3H, ks^layers*Cin+Cout] */
    const float* w_hh;        /* gru.weight_hh_l0     [3H, H]            */
    const float* b_ih;        /* gru.bias_ih_l0       [3H]               */
    const float* b_hh;        /* gru.bias_hh_l0       [3H]               */
    const float* out_w;       /* out_1.weight         [Cout,H,1]         */
    const float* out_b;       /* out_1.bias           [Cout]             */
    const float* scale_out_w; /* scale_out.weight     [Cout,Cout,1]      */
    const float* scale_out_b; /* scale_out.bias       [Cout]             */
    const float* conv2_w;     /* conv.conv.2.weight   [ks^3*Cin,ks^2*Cin,ks] */
    const float* conv2_b;     /* conv.conv.2.bias     [ks^3*Cin]         */
} cvae_net_weights;

/* One row-segment of a pass input: element (b,t,c) lives at ptr[(b*T+t)*row_stride + c], c < width. */
typedef struct cvae_seg {
    const float* ptr;
    int32_t width;
    int32_t row_stride;
} cvae_seg;

/*
 * Input of one GRU_RNN pass = [seg0 ; seg1] along the feature axis (the torch.cat calls at
 * train_gru_cyclevae_gauss_batch.py:1328-1338).  If `lat` is non-NULL, seg1 is ignored and replaced by the
 * reparameterised draw z = mu + exp(log_var/2)*eps of lat[B,T,2*lat_dim] (sampling_vae_batch,
 * gru_vae.py:85-98): eps is read from `eps`[B,T,lat_dim] if non-NULL, else drawn on device with
 * Philox4x32-10 keyed by (seed, draw_id, frame b*T+t, dim / 4): one block yields the four N(0,1) values of a dim quad (Box-Muller,
 * cosine and sine branch of word pairs (0,1) and (2,3)).
 * lat_dim | CVAE_DRAW_LAPLACE: the Laplace posterior instead (sampling_vae_laplace, gru_vae.py:101-112): lat holds [mu ; log-scale],
 * z = mu + exp(s) * u(eps) with u(e) = -sign(e) * log1p(-2|e|); eps is the reference's uniform in (-0.4999, 0.5) if supplied, else
 * word dim & 3 of the same Philox block mapped as cvae_sample_laplace maps it (the same bits for the same seed, draw_id, frame,
 * dim).  With n_draws > 1: z = mu + exp(s) * mean_k u(eps_k).
 */
typedef struct cvae_pass_input {
    cvae_seg seg0, seg1;
    const float* lat;
    int32_t lat_dim;
    const float* eps;
    uint64_t seed;
    uint64_t draw_id;
    int32_t frames;  /* valid frames of this input (0 = all T): frames beyond are zero AFTER normalisation, exactly what the conv
                        padding of a shorter utterance run alone would see; lets utterances of different length share a pass */
    int32_t n_draws; /* > 1 with `lat`: z uses the MEAN of n_draws eps (draw ids draw_id .. draw_id + n_draws - 1, or
                        eps[n_draws][B][T][lat_dim]): the n_smpl_dec latent mean of decode_gru-cyclevae_gauss.py:304-305 */
    /* ABI 5 -- a pass over a WINDOW of a longer utterance (single-row cells, B = 1): the pointers address the window's first
       frame, and ctx_before / ctx_after frames of the same arrays in front of it / behind its last valid frame are real data that
       the dilated conv front-end sees instead of zero padding (the reference convolves an utterance in one piece,
       gru_vae.py:353-357; its +-4-frame reach must not notice where a window was cut).  draw_frame0: index of the window's frame 0
       in the Philox frame numbering of the whole utterance.  eps_draw_stride: floats between two draws in `eps` (0: B*T*lat_dim).
       All zero: the window is the utterance (what every earlier ABI did). */
    int32_t ctx_before, ctx_after;
    int64_t draw_frame0;
    int64_t eps_draw_stride;
} cvae_pass_input;

const char* cvae_last_error_string(void);
int cvae_abi_version(void);

/*
 * ABI 6 -- the handle.  The library keeps NO process-wide mutable state: everything that configures it lives in a context the
 * caller creates, and EVERY entry point below takes that context as its first argument ("no global state besides
 * a per-handle descriptor; one handle per (device, stream); not thread-safe per handle, independent across handles").  A context
 * holds: the status sink (cvae_set_status_sink), this rank's draw origin / parts (cvae_set_draw_origin, cvae_set_draw_parts), the
 * named options (cvae_set_option), the side stream and its join events (cvae_set_side_stream), the profiling brackets
 * (cvae_profile_collect*, cvae_train_profile_collect) and the record of which MFMA-order weight images its train images hold
 * (cvae_net_prepare_train_v: a train image must be used through the context that prepared it).  Two modules on two devices, or
 * two threads, use two contexts and never see each other's settings.  The only thread-local datum is the error string behind
 * cvae_last_error_string.  cvae_ctx_create returns NULL when out of memory; cvae_ctx_destroy(NULL) is a no-op; destroy a context
 * only after the streams it enqueued on have been synchronised (it owns HIP events).  A NULL context fails with -1 (size queries: 0).
 * (The reference has nothing to mirror here: it has no FFI; its per-process state is Python module state.)
 */
typedef struct cvae_ctx cvae_ctx;
cvae_ctx* cvae_ctx_create(void);
int cvae_ctx_destroy(cvae_ctx* ctx);

/*
 * Settings of a context (ABI <= 5 kept them process-wide).
 *
 * cvae_set_status_sink: `sink` = int32[4] the DEVICE can write and the HOST can read without a copy (pinned host memory), or
 * NULL.  When set, the persistent kernels report a timed-out hand-off spin there (sink[0] != 0) instead of in the workspace's
 * status words, so the host-side module can notice it before using any result, without a device synchronisation.  The word is
 * sticky: the caller clears it.  (The reference has nothing to replace here: its GRU loop is a Python loop, gru_vae.py:391-394.)
 *
 * ABI 8 -- the range word.  Status word 0 carries the codes 1-6 (hand-off time-outs, status 5 of the reverse training recurrences);
 * word CVAE_STATUS_RANGE_WORD (3) is a word of its own for CVAE_STATUS_RANGE (7): an eval pass on the limb-operand kernels
 * (CVAE_FLAG_EXACT3 / CVAE_FLAG_SPLIT_F16) was handed a value its fp16 limbs cannot carry -- a normalised input or a carried-in
 * state with !(|v| < option exact_range_at), NaN and inf included, or an image whose folded weights leave the fp16 range that the
 * caller never asked about (cvae_net_prepared_in_range).  The results of that pass are then NaN / inf where the reference is
 * finite: run it again without the two flags (the fp32-operand kernels take the same image and workspace).  Neither word masks
 * the other.  The check sits in the kernels that BUILD limb operands (the prologue of every pass, the slot-0 fill of the deep
 * passes): passes that build none (<= 3 rows, the fp32 / generic kernels, a hidden size without an exact form) never raise it,
 * and no pass has an extra launch.  With a sink the word is sticky like word 0 (sink[3], cleared by the caller; the passes do
 * not clear it); without one, cvae_workspace_status reports it for the LATEST call on that workspace.  Training entry points are
 * out of scope: their normalised input goes through fp32 GEMMs and the state of a GRU is bounded by 1.
 *
 * cvae_set_draw_origin: place of this process in a data-parallel job: row0 = global index of its first batch
 * row, global_rows = batch rows of the whole job (0 = this process alone), frames_per_row = T of the windows fed to
 * cvae_sample (whose `rows` are flattened frames; 0 = no offset there).  The on-device Philox streams (latent draws, dropout
 * masks) are keyed by GLOBAL row, so a row sees the same eps / masks on whichever rank it lands and results do not depend on
 * the number of ranks.  Defaults 0, 0, 0 reproduce the single-process numbering.
 *
 * cvae_set_draw_parts: the batch of the following train-mode passes is `parts` stacked copies of this process's rows (the two
 * decoder passes rec and cv of train...:1335-1336 run as ONE launch of 2B rows, stage4.chain_loss(stack_rec_cv=True)): copy c
 * of local row b is keyed as row c*global_rows + row0 + b of a parts*global_rows-row job, so the dropout masks stay
 * independent of the number of ranks.  Default 1; ignored when the batch is not a multiple of parts.
 */
int cvae_set_status_sink(cvae_ctx* ctx, int32_t* sink);
/*
 * cvae_status_latch (ABI 4): ONE stream-ordered launch that moves the status word from the sink into a DEVICE word the caller
 * owns: latch[0] = max(latch[0], sink[0]); sink[0] = 0.  A training loop that does not synchronise every step calls it at the end
 * of each step and gates the update on `latch` (cvae_adam_step): the latch stays raised -- every later step's update is skipped
 * -- until the caller, having SEEN the code through a stream-ordered copy, clears it with a stream-ordered memset.  The host
 * never writes the sink while steps are in flight (stage4.Stage4Step).  No sink set: no-op.
 */
int cvae_status_latch(cvae_ctx* ctx, int32_t* latch, void* stream);
int cvae_set_draw_origin(cvae_ctx* ctx, int64_t row0, int64_t global_rows, int64_t frames_per_row);
int cvae_set_draw_parts(cvae_ctx* ctx, int32_t parts);

/*
 * Tuning / diagnostic switches of a context, by name (every configuration the library has besides the `flags` arguments; the
 * reference has no counterpart).  Unknown names fail.  cvae_reset_options restores the defaults.
 *   name                default  meaning
 *   "max_rt"            0        > 0: cap on the row tiles a grid handles concurrently (tests: several row tiles per block)
 *   "no_ll"             0        1: passes of <= 3 rows run the dataflow kernel instead of the word-exchange kernel k_gru_steps_ll
 *   "ll_backoff"        -1       >= 0: s_sleep units before the first poll of a step in k_gru_steps_ll (-1: swept default)
 *   "v6_limbs_h64"      3        2: the two-limb form of k_gru_steps_v6 (what H = 2048 runs) at H = 64, for the emulator tests
 *   "exp"               0        measurement switches of the dataflow kernels (bit layout: Step6Params::exp)
 *   "train_kernel"      0        training recurrences: 0 exact fp32 operands (three fp16 limbs), non-zero fp16 pairs (22 bits)
 *   "bwd_overflow_at"   60000    |gate gradient * 2^8| from which the persistent reverse recurrences raise status 5 (tests lower it)
 *   "x3_tile"           0        exact-operand forward training recurrence: 16 / 32 force that row-tile geometry (0: by tiles per block)
 *   "train_per_step"    0        1: forward training recurrence as T launches
 *   "train_bwd_per_step" 0       1: reverse training recurrence as 2T launches (fp32 products; the fallback of a range overflow)
 *   "train_fp32_mfma"   0        1: the forward training recurrence on the fp32-input MFMA (kept for the tests)
 *   "train_backoff"     32       s_sleep units before the first poll of a step (pair-form forward training recurrence)
 *   "train_prof"        0        1: phase cycle sums of block 0 of the training recurrences (cvae_train_debug_counters)
 *   "train_old_gemm"    0        1: the simple GEMM kernels (the unaligned-operand fallbacks) everywhere
 *   "gemm_max_split"    16       cap on the contraction split the tile picker may choose for a training GEMM (1: never split)
 *   "bwd_ks"            8        K slices of the per-step reverse product (the any-H path, e.g. H = 2048); 1..32
 *   "v6_limbs_h2048"    3        2: k_gru_steps_v6 at H = 2048 on fp16 PAIRS (22-23 bit operands, 1.5x faster) instead of exact triples
 *                                with the third weight limb streamed from L2
 *   "v6_w2s_h64"        0        1: that streamed form at H = 64, for the emulator tests
 *   "step_col_tiles"    0        per-step forward training kernel (any-H path): 16-column tiles per block, 0 = pick, 1 / 2 = force
 *   "coop_launch"       0        1: the all-resident recurrent kernels are launched with hipLaunchCooperativeKernel (residency
 *                                checked by the runtime at every launch, ~27 us of idle GPU around each one on MI355X);
 *                                0: residency checked once per kernel through the occupancy query, then plain launches
 *   "gemm_force"        0        measurement: TM*10000 + TN*100 + ks forces tile and contraction split of every training GEMM
 *   "gemm_log"          0        measurement: every training GEMM bracketed by HIP events and printed to stderr (synchronises)
 *   "gemm_trace"        0        1: print when a GEMM takes a fallback kernel
 *   "train_xmap"        0        bit 0 / bit 1: XCD-aware block placement in the exact-operand forward / reverse training recurrence
 *   "ll_row_pad"        0        rows per frame of the time-major buffers of a training pass of <= 3 rows (the word-exchange kernels address
 *                                rows by stride only): 0 = exactly B, so that every GEMM of a one-utterance pass runs over T rows; 4: round 4
 *   "gemm_min_depth"    128      training GEMMs: a split contraction keeps at least this many k per slice (256 until round 5)
 *   "train_bwd_backoff" -1       >= 0: x 64 cycles before the first flag poll of a task of the persistent reverse training recurrences
 *                                (-1: 32 when a block has one row tile, else 0)
 *   "train_fwd_backoff" -1       >= 0: the same for the exact forward training recurrences with 16-row tiles (-1: 24 with one tile, else 0)
 *   "train_fwd_geom"    -1       exact forward training recurrence: 1 = 16-unit blocks (k_train_fwd_steps_w3), 0 = 8-unit blocks
 *                                (k_train_fwd_steps_x3 / x3h); -1: 16-unit blocks for passes of at least 64 rows
 *   "train_bwd_geom"    -1       exact reverse training recurrence: 1 = 16-unit blocks (k_train_bwd_steps_w3), 0 = 8-unit blocks
 *                                (k_train_bwd_steps_x3); -1: 16-unit blocks for passes of at least 64 rows
 *   "bwd_w3_l1_h64"     0        1: the 16-unit reverse recurrence at H = 64 keeps second limbs in LDS (what H = 1024 runs), for the emulator tests
 *   "train_profile"     0        1: HIP events on the launch stream around the training recurrences and GEMMs (cvae_train_profile_collect)
 *   "v6_backoff"        -1       >= 0: units of 64 cycles a block of k_gru_steps_v6 with one row tile sleeps before the first flag poll
 *                                of a step (-1: swept per front-end width: 8 for the decoder's KFW = 6, 2 for the encoder's 8)
 *   "exact_range_at"    65504    |x| from which an exchanged value of the limb-operand eval kernels (normalised input, carried-in state)
 *                                raises CVAE_STATUS_RANGE.  65504 (default, the largest finite half): the first limb overflows and the
 *                                result is unusable.  2048: the bound below which the (fp16, fp16, bf8) triple is EXACT; in between
 *                                the clamped bf8 limb costs at most 2^-23 relative.  Clamped to 1 .. 65504.
 *   "dtw_batch_cost"    1        cvae_dtw_batch: 1 = local costs written first by one grid-wide kernel over all problems of a chunk (a
 *                                T1 x T2 f64 slab per problem), 0 = computed inside the path kernel, cell by cell (one byte of work memory
 *                                per cell).  Same bits either way; profiles/validation_notes.md holds the measurement.
 *   "masks_on_side"     1        train-mode forward with a side stream set: the dropout mask of the recurrence's feedback operand is
 *                                drawn on the side stream, beside the prologue and the front-end GEMMs (0: on the launch stream)
 *   "v6_skip_t0"        1        k_gru_steps_v6 in a pass no cell of which carries a state in (slot 0 is all zeros): 1 = the tasks of
 *                                frame 0 request no state operand and issue no recurrent MFMA (each would add an exact +0: same bits);
 *                                0 = they multiply the zeros (profiles/v6_launch_ramp_notes.md)
 */
int cvae_set_option(cvae_ctx* ctx, const char* name, int64_t value);
int cvae_get_option(cvae_ctx* ctx, const char* name, int64_t* value);
int cvae_reset_options(cvae_ctx* ctx);

/*
 * Self-test of the operand transport of the exact-operand kernels (no reference counterpart: the reference multiplies fp32
 * values directly): y[i] = l0 + l1/2^11 + l2/2^22 where (l0, l1, l2) are the two halves and the bf8 byte a producer publishes for
 * x[i] and l2 has gone through the consumer's packed decode.  n a multiple of 8.  y == x bit for bit for |x| >= 2^-16 (and 0),
 * |y - x| <= 2^-40 below; tests also compare the device result bit for bit with the host build of the same code.
 */
int cvae_selftest_limbs(cvae_ctx* ctx, const float* x, float* y, int64_t n, void* stream);
/* Test aid (ABI 4): `blocks` workgroups of 256 threads that each hold `lds_bytes` of LDS and stay resident for `cycles` shader
 * cycles on `stream`: CU-side contention for the all-resident recurrent kernels, which are launched plainly after a one-time
 * occupancy check (tests/test_gpu_parity.py::test_hand_off_under_cu_contention). */
int cvae_selftest_occupy(cvae_ctx* ctx, int blocks, size_t lds_bytes, int64_t cycles, void* stream);
/*
 * Test aid (additive, ABI 10): ONE training GEMM / column sum through the wrapper a training pass calls, unchanged, so that
 * the options ("gemm_force", "train_old_gemm", "gemm_max_split", ...) act exactly as they do in a pass.  No reference counterpart
 * (the reference calls torch.nn.functional; these are the products its autograd graph holds).
 *
 * kind and the three extents, in the wrapper's own argument order:
 *   CVAE_GEMM_NT      C[m*ldc + n] (+)= sum_k A[m*lda + seg(k)] * B[n*ldb + k] + bias[n],   m < M, n < N, k < K
 *                     seg(k) = (k / seglen)*segstride + k % seglen; then, with a mask ([mask_B][mask_T][N], M = mask_T*mask_Bp):
 *                     row m = f*mask_Bp + b is multiplied by mask[(b*mask_T + f)*N + n], rows b >= mask_B become 0.
 *   CVAE_GEMM_TN      C[i*ldc + j] (+)= sum_m A[m*lda + i] * B[m*ldb + seg(j)],   m < M (contraction ROWS), i < N, j < K
 *   CVAE_GEMM_KS      C[m*ldc + n] (+)= sum_k A[m*lda + k] * B[n*ldb + k]         (the small-M product of the reverse recurrence)
 *   CVAE_GEMM_COLSUM  C[n] (+)= sum_m A[m*lda + n],   m < M, n < N                  (K, B unused)
 * use_split: hand the wrapper the split work space (partial tiles + arrival counters) inside `work`; 0: none (no split possible).
 *
 * Operand contracts (what the kernels may touch; the callers in a training pass pad their buffers accordingly).  [a_lo, a_hi),
 * [b_lo, b_hi) and [0, c_hi) are the floats the caller owns around A, B and C; a call whose kernels could leave them, or that
 * breaks another rule below, is refused with -1 and a message instead of being launched:
 *   nt      K and seglen multiples of 16; K a multiple of seglen, or K <= seglen (one segment).  A is touched at
 *           m*lda + s*segstride + [0, min(seglen, K)) for every segment s (segstride may be negative: a_lo < 0), B at
 *           n*ldb + [0, K), C at m*ldc + [0, N) only.  The LDS-tiled kernels run when lda, ldb, segstride are multiples of 4 and A, B
 *           are 16-byte aligned; otherwise (or with "train_old_gemm") the simple kernel runs, and THERE a mask is applied in place
 *           by a second kernel that rewrites the whole [M][ldc] block: columns N .. ldc-1 become 0 (c_hi >= M*ldc).
 *   tn      tiled when lda, ldb, seglen, segstride are multiples of 4 and A, B 16-byte aligned: every row of A is read as float4 up
 *           to up(N, 4) columns, every row of B to the end of the float4 that holds the last column of each segment.  The simple
 *           kernel reads exactly the N and K columns.
 *   ks      K a multiple of 16; A at m*lda + [0, K), B at n*ldb + [0, K).
 *   colsum  two-stage kernel (lda a multiple of 4, A 16-byte aligned, split work space given, not "train_old_gemm"): rows are
 *           read as float4 up to up(N, 4) columns; the simple kernel reads exactly N.  Without a split work space the simple
 *           kernel runs (the two-stage kernel needs the counters to write its result).
 *   all     extents >= 1, leading dimensions >= 0, ldc >= the output's columns, bias (nt only, may be NULL) holds N floats.
 *
 * work: cvae_selftest_gemm_work_bytes() bytes of device memory, 16-byte aligned, ZEROED ONCE by the caller: the partial-tile area
 * followed by CVAE_SELFTEST_GEMM_CNT uint32 arrival counters (the last bytes of `work`), which every call leaves at zero again.
 * ran (HOST int32[4], written before the call returns): what the wrapper launched -- {1 LDS-tiled / two-stage kernel or 0 simple
 * kernel, TM, TN (block tile 32*TM x 32*TN; 0 for ks and colsum), slices of the contraction (grid z, grid y for colsum)}.
 * The launch is asynchronous on `stream`.
 */
enum { CVAE_GEMM_NT = 0, CVAE_GEMM_TN = 1, CVAE_GEMM_KS = 2, CVAE_GEMM_COLSUM = 3 };
#define CVAE_SELFTEST_GEMM_CNT 4096
typedef struct cvae_gemm_case {
    int32_t kind, accumulate, use_split;
    int32_t M, N, K;
    int32_t seglen;
    int32_t mask_B, mask_Bp, mask_T;     /* read when mask != NULL */
    int64_t lda, ldb, ldc, segstride;
    int64_t a_lo, a_hi, b_lo, b_hi, c_hi;
    const float* A;
    const float* B;
    const float* bias;
    const float* mask;
    float* C;
} cvae_gemm_case;
size_t cvae_selftest_gemm_work_bytes(cvae_ctx* ctx);
int cvae_selftest_gemm(cvae_ctx* ctx, const cvae_gemm_case* c, void* work, size_t work_bytes, int32_t ran[4], void* stream);

/* Bytes of the caller-owned prepared-weights image / prepare-time scratch for a net. */
size_t cvae_net_prepared_bytes(cvae_ctx* ctx, const cvae_net_desc* d);
size_t cvae_net_prepare_scratch_bytes(cvae_ctx* ctx, const cvae_net_desc* d);

/*
 * Build the device weight image used by the forward kernels (call again whenever the weights change):
 * folds scale-free conv0*conv1*W_ih[:, :ks^2*Cin] into one ks^2-tap matrix, folds the autoregressive
 * feedback W_ih[:, ks^2*Cin:] * out_1 into the recurrent matrix, and lays both out for MFMA fragment loads.
 * Replaces nothing the reference does at run time; it is the load-time half of GRU_RNN.forward
 * (gru_vae.py:353-357 convs, :365/:392 gate matmuls, :371/:393 projection).
 */
int cvae_net_prepare(cvae_ctx* ctx, const cvae_net_desc* d, const cvae_net_weights* w, void* prepared, size_t prepared_bytes,
                     void* scratch, size_t scratch_bytes, void* stream);
/*
 * ABI 8: do the weights of a prepared image (cvae_net_prepare, cvae_net_prepare_deep with its n_layers) fit the limb images?  The
 * prepare kernels leave a flag in the image when a FOLDED weight (front-end fold, feedback fold + W_hh, scale_out . out_1, W_ih / W_hh
 * of an upper layer) reaches the largest finite half, 65504: its first limb would be inf.  Returns 1 = fits, 0 = does not,
 * negative = error; synchronises `stream` (call it once per image build, not per pass).  The context remembers a 0 by the image's
 * address: passes on that image through this context then run the fp32-operand kernels whatever exact / split flags they are
 * given (deep images: k_gru_steps_deep; cvae_plan_pass_deep does not see an image: for an unfit one the pass takes what it
 * reports for flags | CVAE_FLAG_GENERIC_STEP) -- the reference simply computes on such weights, and so does the pass.  A pass on
 * an unfit image the context was never asked about raises CVAE_STATUS_RANGE instead.  The answer is kept by ADDRESS until this
 * context prepares an image there again: ask again after an image was rebuilt at the same address through another context.
 */
int cvae_net_prepared_in_range(cvae_ctx* ctx, const cvae_net_desc* d, int n_layers, const void* prepared, void* stream);

/* Bytes of workspace one pass of (B,T) needs. */
size_t cvae_pass_workspace_bytes(cvae_ctx* ctx, const cvae_net_desc* d, int B, int T);

#define CVAE_FLAG_PERSISTENT 1 /* run the T recurrent steps as ONE launch of an all-resident grid (blocks hand over through flags) */
#define CVAE_FLAG_HOISTED_FRONTEND 32 /* with PERSISTENT: keep the front-end as a separate GEMM launch + gx buffer (tests, A/B) */
#define CVAE_FLAG_SPLIT_F16 256 /* with PERSISTENT: matrix products of the recurrent kernel as three fp16 MFMAs on (hi, lo) pairs,
                                   x = hi + lo/2048 (22-bit operands, f32 accumulate); without it the all-fp32-MFMA kernel runs.
                                   (bits 16, 64, 128 selected kernel generations that no longer exist: ignored) */
#define CVAE_CLAMP_LAPLACE (1 << 30) /* OR into a clamp_lat_dim argument: the Laplace variant's floor instead of ln(1e-6) */
#define CVAE_FLAG_EXACT3 512 /* with PERSISTENT: every matrix product of the recurrent kernel on EXACT fp32 operands, each carried
                                as three fp16 limbs (x = l0 + l1/2^11 + l2/2^22), six f16 MFMAs per product, f32 accumulate
                                (k_gru_steps_v6; H = 1024 or 64, more than 16 batch rows); takes precedence over SPLIT_F16 */
#define CVAE_FLAG_GENERIC_STEP 4 /* with PERSISTENT: use the any-H recurrent kernel even where a tuned one exists (tests) */
#define CVAE_FLAG_STEP_TIMING 8  /* debugging: the tuned recurrent kernel accumulates per-phase cycle counters */
#define CVAE_FLAG_PROFILE 2    /* bracket the recurrent kernel(s) of each pass with hipEvents (see cvae_profile_collect) */

#define CVAE_STATUS_RANGE 7        /* status code of an operand outside the window of the limb form (cvae_set_status_sink, ABI 8) */
#define CVAE_STATUS_RANGE_WORD 3   /* the status word that carries it */

/*
 * ABI 9: the recurrence an eval pass of a one-layer network with `rows` batch rows in all (cells x B of the stacked entry points)
 * would take on the current device under this context's options -- the one-layer counterpart of cvae_plan_pass_deep; the rule
 * table is DESIGN.md 4.1.  Negative = error.  Like the deep query it sees no image and no per-call pointers: a pass on an image
 * the context knows to be unfit (cvae_net_prepared_in_range) takes what this reports for flags & ~CVAE_FLAG_SPLIT_F16, with
 * CVAE_FLAG_EXACT3 ignored for passes of more than three rows.
 */
typedef enum cvae_eval_form {
    CVAE_EVAL_PER_STEP = 0, /* k_gru_steps<false>, one launch per step, behind the front-end GEMM                       */
    CVAE_EVAL_GENERIC = 1,  /* k_gru_steps<true>: the any-H kernel as one launch behind a grid barrier, front-end GEMM   */
    CVAE_EVAL_V2 = 2,       /* k_gru_steps_v2: 16-row dataflow kernel behind the front-end GEMM                          */
    CVAE_EVAL_V4 = 3,       /* k_gru_steps_v4: front-end fused, fp32 MFMA                                                */
    CVAE_EVAL_V5 = 4,       /* k_gru_steps_v5: front-end fused, fp16 pairs                                               */
    CVAE_EVAL_V6 = 5,       /* k_gru_steps_v6: 32-row tiles, exact fp32 operands as fp16 limbs                           */
    CVAE_EVAL_LL = 6,       /* k_gru_steps_ll: at most three rows, word exchange, behind the front-end GEMM              */
    CVAE_EVAL_V6H = 7       /* k_gru_steps_v6<KPW, 0>: the exact-operand recurrence behind the front-end GEMM (ABI 10: front-ends
                               too wide for the LDS limb image of V6, KFW >= 12)                                        */
} cvae_eval_form;
int cvae_plan_pass(cvae_ctx* ctx, const cvae_net_desc* d, int rows, int T, int flags);

/*
 * One GRU_RNN.forward in eval mode (gru_vae.py:322-455, live branch: res/noise/softmax/... flags off).
 *   in      : the pass input, B*T rows of Cin = seg0.width + (lat ? lat_dim : seg1.width) features
 *   y_in    : [B,Cout]  initial feedback (gru_vae.py:365)
 *   h_in    : [B,H] or NULL (zeros)      (gru_vae.py:364-367)
 *   clamp_lat_dim : >=0 -> clamp trj_out[..., clamp_lat_dim:] to >= ln(1e-6) (clamp_vae, gru_vae.py:410-412);
 *                   L | CVAE_CLAMP_LAPLACE -> to >= -7.2543288692621097, the log-scale floor of the Laplace variant
 *                   (clamp_vae_laplace, gru_vae.py:415-417); ignored when the net has scale_out.  The same
 *                   encoding holds for every clamp_lat_dim argument below (train-mode forward / backward included)
 *   trj_out : [B,T,Cout]; y_last: [B,Cout] raw last projection; h_last: [B,H]   (gru_vae.py:452-453)
 *   status  : int32[4] (the sink of cvae_set_status_sink, else read with cvae_workspace_status): status[0] != 0 after completion
 *             means a hand-off spin or grid barrier timed out; status[3] == CVAE_STATUS_RANGE that an operand of a limb-operand
 *             kernel was out of range (ABI 8, see cvae_set_status_sink): the pass ran to its end on inf / NaN operands
 */
int cvae_gru_rnn_forward(cvae_ctx* ctx, const cvae_net_desc* d, const void* prepared, const cvae_pass_input* in,
                         const float* y_in, const float* h_in, int B, int T, int clamp_lat_dim,
                         float* trj_out, float* y_last, float* h_last,
                         void* workspace, size_t workspace_bytes, int flags, void* stream);

/*
 * Up to 32 INDEPENDENT inputs through the same net as one pass (rows stacked along the batch axis: the recurrence is per row, so
 * stacking changes no result and divides the number of dependent steps).  Stage 6 runs E(src) || E(trg) and then its three
 * decoder passes this way (decode_gru-cyclevae_gauss.py:303-323), for one utterance pair or for several pairs at once (a step
 * costs the same chip-wide hand-off for 1 row and for 32: one row tile of the dataflow kernels).  in[c], y_in[c] [B][Cout], trj_out[c] [B][T][Cout] per cell;
 * h = 0, no y_last / h_last.  Workspace: cvae_pass_workspace_bytes(d, ncell * B, T).
 */
int cvae_gru_rnn_forward_stacked(cvae_ctx* ctx, const cvae_net_desc* d, const void* prepared, int ncell, const cvae_pass_input* in,
                                 const float* const* y_in, int B, int T, int clamp_lat_dim, float* const* trj_out,
                                 void* workspace, size_t workspace_bytes, int flags, void* stream);

/*
 * The same with carried state (ABI 5), for passes over consecutive windows of the stacked utterances (cvae_pass_input::ctx_*):
 * h_in[c] [B][H] or NULL (state 0); h_last[c] [B][H] or NULL.  y_in[c] == NULL with h_in[c] != NULL means "this window CONTINUES
 * the recurrence that left h_in[c]": the feedback of its first frame is out_1(h_in) through the folded recurrent matrix, exactly
 * what frame t of an unbroken pass does with h_{t-1} -- windows then reproduce the unbroken pass bit for bit (same kernel, same
 * per-row arithmetic).  The reference has one Python loop per pass (gru_vae.py:391-394) and nothing to mirror here; this entry
 * exists so that the decoder launch of window w can run beside the encoder launch of window w+1 (stage6.convert_pairs).
 */
int cvae_gru_rnn_forward_stacked_carry(cvae_ctx* ctx, const cvae_net_desc* d, const void* prepared, int ncell, const cvae_pass_input* in,
                                       const float* const* y_in, const float* const* h_in, int B, int T, int clamp_lat_dim,
                                       float* const* trj_out, float* const* h_last, void* workspace, size_t workspace_bytes,
                                       int flags, void* stream);

/*
 * ABI 7 -- networks with n_layers >= 2 GRU layers (the reference's `hidden_layers`, gru_vae.py:282-320: nn.GRU(tot_in_dim, H,
 * hidden_layers); "deep" here, because cvae_gru_rnn_forward_stacked above stacks ROWS).  Eval mode only: layer 0 reads
 * [conv front-end ; y_{t-1}] through weight_ih_l0, layer l >= 1 reads h_{l-1,t} through weight_ih_l{l} [3H][H], y_t = out_1(h_{L-1,t}),
 * no dropout between layers (gru_vae.py:376-394 with the module in eval mode).  `w` carries layer 0 and everything around the GRU
 * exactly as for cvae_net_prepare; `upper[l-1]` the four tensors of layer l = 1 .. n_layers-1 (an array in HOST memory of device
 * pointers).  The prepared image is the one-layer image of layer 0 (front-end fold, biases, projection) followed by per-layer
 * recurrent images [W_hh_l | U_l], U_0 = W_ih_l0[:, 9C:] . out_1.w (the feedback fold, applied to the TOP layer's previous state),
 * U_l = W_ih_l.  h_in / h_last are [n_layers][B][H] (what nn.GRU takes and returns) or NULL; everything else as in
 * cvae_gru_rnn_forward, whose `flags` apply as far as they make sense: CVAE_FLAG_PERSISTENT (one launch for the whole L*T chain of
 * sub-steps where the grid is resident), CVAE_FLAG_GENERIC_STEP (the any-H kernel even where the resident one exists),
 * CVAE_FLAG_PROFILE (one bracket per recurrence LAUNCH).  Every product is exact fp32 arithmetic on either kernel.
 * n_layers == 1: each of these entry points IS its one-layer counterpart (same image, same workspace, same kernels; `upper` unused).
 * cvae_plan_pass_deep reports the recurrence a pass would take: 0 one launch per sub-step, 1 the any-H kernel as one launch,
 * 2 the resident exact-operand kernel (H = 1024 or 64, n_layers * H/8 blocks resident); negative = error.
 * cvae_plan_pass_deep_tiles (additive, tests): the whole plan of the same rule, out (HOST int32[4]) = {path as above, Bp = rows
 * padded to 32, rts = row-tile sets in flight (1 off the resident kernel), tiles = the most row tiles one block handles per frame:
 * 32-row tiles of a resident block, ceil(Bp/32 / rts) <= 4 (a block carries its tiles' states in four registers; more rows than that
 * take the any-H kernel), else the Bp/16 16-row tiles every block of the any-H kernel walks, four a trip}.  Returns 0 or an error.
 */
typedef struct cvae_gru_layer {
    const float* w_ih;  /* gru.weight_ih_l{l}  [3H, H]  */
    const float* w_hh;  /* gru.weight_hh_l{l}  [3H, H]  */
    const float* b_ih;  /* gru.bias_ih_l{l}    [3H]     */
    const float* b_hh;  /* gru.bias_hh_l{l}    [3H]     */
} cvae_gru_layer;
size_t cvae_net_prepared_bytes_deep(cvae_ctx* ctx, const cvae_net_desc* d, int n_layers);
size_t cvae_net_prepare_scratch_bytes_deep(cvae_ctx* ctx, const cvae_net_desc* d, int n_layers);
int cvae_net_prepare_deep(cvae_ctx* ctx, const cvae_net_desc* d, int n_layers, const cvae_net_weights* w, const cvae_gru_layer* upper,
                          void* prepared, size_t prepared_bytes, void* scratch, size_t scratch_bytes, void* stream);
size_t cvae_pass_workspace_bytes_deep(cvae_ctx* ctx, const cvae_net_desc* d, int n_layers, int B, int T);
int cvae_plan_pass_deep(cvae_ctx* ctx, const cvae_net_desc* d, int n_layers, int B, int T, int flags);
int cvae_plan_pass_deep_tiles(cvae_ctx* ctx, const cvae_net_desc* d, int n_layers, int B, int T, int flags, int32_t out[4]);
int cvae_gru_rnn_forward_deep(cvae_ctx* ctx, const cvae_net_desc* d, int n_layers, const void* prepared, const cvae_pass_input* in,
                              const float* y_in, const float* h_in, int B, int T, int clamp_lat_dim, float* trj_out, float* y_last,
                              float* h_last, void* workspace, size_t workspace_bytes, int flags, void* stream);

/*
 * sampling_vae_batch (gru_vae.py:85-98) on device: z[n,l] = lat[n,l] + exp(lat[n,L+l]/2) * eps[n,l],
 * n < rows.  eps NULL -> Philox draw keyed (seed, draw_id, n, l).  eps_out (optional) receives the eps used.
 */
int cvae_sample(cvae_ctx* ctx, const float* lat, int rows, int lat_dim, const float* eps, uint64_t seed, uint64_t draw_id,
                float* z, float* eps_out, void* stream);

/*
 * SURVEY 8(f) row 4, first variant -- the Laplace posterior of the sibling recipes: sampling_vae_laplace (gru_vae.py:101-112, the
 * log-scale branch) on device: z[n,l] = lat[n,l] - exp(lat[n,L+l]) * sign(eps) * log1p(-2|eps|), eps ~ U(-0.4999, 0.5) as the
 * reference draws it (`uniform_(-0.4999, 0.5)`); eps NULL -> Philox keyed (seed, draw_id, n, l).  The backward gives
 * d lat = [dz ; dz * (z - mu)].  The matching clamp of GRU_RNN.forward is CVAE_CLAMP_LAPLACE in clamp_lat_dim; loss_vae_laplace
 * (:130-139) is torch ops in the drop-in module.
 */
int cvae_sample_laplace(cvae_ctx* ctx, const float* lat, int rows, int lat_dim, const float* eps, uint64_t seed, uint64_t draw_id,
                        float* z, float* eps_out, void* stream);
int cvae_sample_laplace_backward(cvae_ctx* ctx, const float* dz, const float* lat, const float* z, int rows, int lat_dim, float* dlat,
                                 void* stream);

/*
 * The Laplace posterior inside the fused paths: OR this into a lat_dim value, as CVAE_CLAMP_LAPLACE is OR-ed into clamp_lat_dim.
 * It is honoured by cvae_pass_input.lat_dim (the draw inside a pass prologue, single or the mean of n_draws), by the lat_dim of
 * cvae_cycle_forward / cvae_cycle_forward_carry (the three draws of every cycle are Laplace draws and the encoder passes clamp at
 * the Laplace floor), of cvae_latent_mean, of cvae_sample_cat / cvae_sample_cat_backward (d mu = dz, d s = dz * exp(s) * u(eps)) and
 * of cvae_stage4_loss (KL = sum_d(-s + b exp(-|mu|/b) + |mu| - 1), b = exp(s): loss_vae_laplace, gru_vae.py:130-139), and by
 * cvae_trainlog_window_args.L (record entries [3], [4] are that KL).  Every entry
 * strips the flag before it validates or uses the dimension; without it nothing changes.
 */
#define CVAE_DRAW_LAPLACE (1 << 30)

/* Bytes of workspace the fused cycle chain needs. */
size_t cvae_cycle_workspace_bytes(cvae_ctx* ctx, const cvae_net_desc* enc, const cvae_net_desc* dec, int B, int T, int n_cyc);

/*
 * The n_cyc reconversion loop in eval form (train_gru_cyclevae_gauss_batch.py:1326-1338 with do=False):
 * per cycle  lat = E(x | [x[:,:,:stdim]; rec_cyc_prev]),  rec = D([code_src; z1]),  cv = D([code_trg; z2]),
 *            latcv = E([cvx; cv]),  rec_cyc = D([code_src; z3]).
 *   x [B,T,Cin_enc]; cvx [B,T,stdim]; code_src/code_trg [B,T,ncode]; y_in_enc [B,2L]; y_in_dec [B,Cout_dec]
 *   eps: NULL (Philox from seed) or [n_cyc,3,B,T,L] in draw order (rec, cv, rec_cyc)
 *   outputs (each may be NULL to skip the copy-out): lat/latcv [n_cyc,B,T,2L]; rec/cv/reccyc [n_cyc,B,T,Cout_dec]
 */
int cvae_cycle_forward(cvae_ctx* ctx, const cvae_net_desc* enc, const void* enc_prepared,
                       const cvae_net_desc* dec, const void* dec_prepared,
                       const float* x, const float* cvx, int stdim,
                       const float* code_src, const float* code_trg, int ncode,
                       const float* y_in_enc, const float* y_in_dec,
                       int B, int T, int n_cyc, int lat_dim, const float* eps, uint64_t seed,
                       float* out_lat, float* out_rec, float* out_cv, float* out_latcv, float* out_reccyc,
                       void* workspace, size_t workspace_bytes, int flags, void* stream);

/*
 * The same chain continued from / returning the state of every pass: the windowed form of the loop
 * (train_gru_cyclevae_gauss_batch.py:1299-1311: each of the 5 passes of a cycle restarts from ITS OWN (y_last, h) of the previous
 * window; the conv front-end is re-padded with zeros per window).  Pass order inside a cycle: encoder slots {lat, latcv},
 * decoder slots {rec, cv, reccyc}.  state_in NULL = fresh window (y_in_enc / y_in_dec, h = 0); state_out NULL = not wanted.
 * y values are the RAW last projections (pre-clamp / pre-scale_out, gru_vae.py:452).
 */
typedef struct cvae_cycle_state {
    float* y_enc; /* [n_cyc][2][B][2*lat_dim]  */
    float* y_dec; /* [n_cyc][3][B][Cout_dec]   */
    float* h_enc; /* [n_cyc][2][B][H_enc]      */
    float* h_dec; /* [n_cyc][3][B][H_dec]      */
} cvae_cycle_state;
int cvae_cycle_forward_carry(cvae_ctx* ctx, const cvae_net_desc* enc, const void* enc_prepared,
                             const cvae_net_desc* dec, const void* dec_prepared,
                             const float* x, const float* cvx, int stdim,
                             const float* code_src, const float* code_trg, int ncode,
                             const float* y_in_enc, const float* y_in_dec,
                             int B, int T, int n_cyc, int lat_dim, const float* eps, uint64_t seed,
                             float* out_lat, float* out_rec, float* out_cv, float* out_latcv, float* out_reccyc,
                             void* workspace, size_t workspace_bytes, int flags, void* stream,
                             const cvae_cycle_state* state_in, const cvae_cycle_state* state_out);

/*
 * The chain of the many-to-many recipes: every cycle has its own target codes and its own converted excitation (the
 * src_trg_code_list[i] / cv_src_list[i] of a FeatureDatasetMultTrainVAE item).  cvae_cycle_forward_carry's arguments plus two
 * strides in ELEMENTS: cycle i reads cvx + i * cvx_cycle_stride ([B,T,stdim]) and code_trg + i * code_trg_cycle_stride
 * ([B,T,ncode]), i.e. contiguous [n_cyc,B,T,.] tensors pass B*T*stdim and B*T*ncode:
 *   cv_i = D([code_trg[i] ; z2]),  latcv_i = E([cvx[i] ; cv_i]);  lat_i, rec_i and rec_cyc_i as before (code_src is one tensor).
 * A stride of 0 reads one tensor in every cycle; either stride may be 0 on its own.  state_in / state_out may be NULL (the fresh
 * form).  cvae_cycle_forward and cvae_cycle_forward_carry ARE this call with both strides 0: same launches, same arguments, same
 * bits.  ncode is any width >= 1 (decoder in_dim = ncode + lat_dim).  Returns -1 before anything is enqueued for a stride that
 * is negative, or positive and shorter than one cycle's block.
 */
int cvae_cycle_forward_m2m(cvae_ctx* ctx, const cvae_net_desc* enc, const void* enc_prepared,
                           const cvae_net_desc* dec, const void* dec_prepared,
                           const float* x, const float* cvx, int stdim,
                           const float* code_src, const float* code_trg, int ncode,
                           const float* y_in_enc, const float* y_in_dec,
                           int B, int T, int n_cyc, int lat_dim, const float* eps, uint64_t seed,
                           float* out_lat, float* out_rec, float* out_cv, float* out_latcv, float* out_reccyc,
                           void* workspace, size_t workspace_bytes, int flags, void* stream,
                           const cvae_cycle_state* state_in, const cvae_cycle_state* state_out,
                           int64_t cvx_cycle_stride, int64_t code_trg_cycle_stride);

/*
 * Measurement aid for bench.py: with CVAE_FLAG_PROFILE every pass records a hipEvent pair on `stream` around its
 * recurrent kernel (the dominant kernel: k_gru_steps).  This call waits for the recorded pairs, returns their
 * summed elapsed time and count, and clears the list.  The events are the only thing the library ever allocates.
 */
int cvae_profile_collect(cvae_ctx* ctx, double* total_ms, int* launches);
/* The same brackets launch by launch (ABI 4): fills ms / rows / cin (stacked batch rows and input channels of the pass each
 * bracket belongs to: which instantiation and geometry of the recurrent kernel ran) for up to `cap` launches, returns how many,
 * forgets them.  bench.py groups them into the per-instantiation rooflines. */
int cvae_profile_collect_launches(cvae_ctx* ctx, double* ms, int* rows, int* cin, int cap);

/*
 * Debugging aid: after a cvae_gru_rnn_forward with CVAE_FLAG_PERSISTENT|CVAE_FLAG_STEP_TIMING on the tuned kernel,
 * out[0..3] = mean over blocks and out[4..7] = max over blocks of the cycle sums spent in
 * {operand loads + MFMA, reduce + gates + publish, store drain, barrier wait} over the T steps.  Synchronises.
 */
int cvae_step_timing(cvae_ctx* ctx, const cvae_net_desc* d, int B, int T, const void* workspace, double out[8], void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Training (stage 4, train_gru_cyclevae_gauss_batch.py:1326-1420): train-mode pass with a tape, BPTT backward, Adam.
 * Recurrences: at H = 1024 / 64 persistent launches (exact fp32 operands as fp16 triples by default, option "train_kernel"; 16-unit
 * blocks from 64 rows on, 8-unit blocks below; word-exchange kernels for passes of at most three rows), per-step launches at other
 * sizes; GEMMs on the fp32-input MFMA.
 * ------------------------------------------------------------------------------------------------------------------ */

/* Gradient outputs in the reference's state_dict layout (scale_in / scale_out are frozen, train...:369-372). */
typedef struct cvae_net_grads {
    float *conv0_w, *conv0_b, *conv1_w, *conv1_b, *w_ih, *w_hh, *b_ih, *b_hh, *out_w, *out_b;
} cvae_net_grads;

size_t cvae_train_image_bytes(cvae_ctx* ctx, const cvae_net_desc* d);
/* Weight image for the train-mode kernels; rebuild after every optimiser step.  gru_drop_p: the dropout probability the passes run
 * on this image will be called with (the `do_prob` of the reference module, gru_vae.py:312-316; 0 when dropout is off): the
 * exact-operand forward recurrence multiplies the feedback weights with the MASKED state, so the mask's scale 1/(1-p) is folded
 * into that weight image here.  cvae_gru_rnn_forward_train must be given the same p_drop (supplied masks: 0 or 1/(1-p)). */
int cvae_net_prepare_train(cvae_ctx* ctx, const cvae_net_desc* d, const cvae_net_weights* w, void* image, size_t image_bytes, float gru_drop_p,
                           void* stream);
/* The same with a choice of the MFMA-order weight images to build (ABI 4): `variants` = OR of 1 (exact-operand tile kernels), 2
 * (fp16-pair kernels), 4 (fp32-MFMA persistent forward); 0 = none of them -- enough for passes of at most three rows (word-exchange
 * kernels) and for the per-step launch paths.  cvae_net_prepare_train = variants 7.  cvae_train_variants_needed(d, B, T): what a
 * pass of that shape needs under the current options.  A pass whose image lacks what it needs fails with -4 (the library keeps a
 * host-side record per image address); the unused images are ~300 MB of writes and ~0.15 ms of kernels per net at hu1024. */
int cvae_net_prepare_train_v(cvae_ctx* ctx, const cvae_net_desc* d, const cvae_net_weights* w, void* image, size_t image_bytes, float gru_drop_p,
                             int variants, void* stream);
int cvae_train_variants_needed(cvae_ctx* ctx, const cvae_net_desc* d, int B, int T);
/* cvae_plan_train_pass (additive, tests): the recurrence forms a train-mode pass of that shape takes under the current options, as
 * the rule the passes themselves consult computes them.  out (HOST int32[12]) = {Bp = rows per frame of the time-major buffers;
 * forward form: 0 word exchange, 1 exact operands in 16-unit blocks, 2 in 8-unit blocks with 32-row tiles, 3 with 16-row tiles,
 * 4 fp16 pairs, 5 fp32 MFMA, 6 T per-step launches; forward row tiles side by side; the most row tiles one forward block row owns
 * per step (32-row tiles of form 2, 16-row tiles otherwise; 0 for forms 0 and 6); 16-column tiles per block of the per-step forward;
 * 1 when the forward writes the gate tape and the state copies in full (no memset); reverse form: 0 word exchange, 1 exact
 * operands in 16-unit blocks, 2 in 8-unit blocks, 3 fp16 pairs, 4 2T per-step launches; reverse row tiles side by side; 16-row tiles
 * per launch of the reverse recurrence (0: the whole pass in one); the most tiles one reverse block row owns in one launch (0 for
 * forms 0 and 4); 1 when the reverse recurrence writes every row of the gate gradients (no memset); the image variants as
 * cvae_train_variants_needed}.  Returns 0 or an error. */
int cvae_plan_train_pass(cvae_ctx* ctx, const cvae_net_desc* d, int B, int T, int32_t out[12]);
size_t cvae_train_tape_bytes(cvae_ctx* ctx, const cvae_net_desc* d, int B, int T);     /* per pass, kept until its backward */
size_t cvae_train_scratch_bytes(cvae_ctx* ctx, const cvae_net_desc* d, int B, int T);  /* shared by all passes */

/*
 * GRU_RNN.forward with do=True (gru_vae.py:353-355 conv_drop, :378-382 gru_drop on the state fed to out_1; the carried h
 * is un-dropped).  x [B,T,Cin] contiguous.  cmask [B,T,ks^2*Cin] / gmask [T,B,H]: dropout masks already scaled by
 * 1/(1-p), or NULL to draw them with Philox from `seed`.  Activations needed by the backward are written to `tape`.
 */
int cvae_gru_rnn_forward_train(cvae_ctx* ctx, const cvae_net_desc* d, const void* image, const float* x, const float* y_in, const float* h_in,
                               int B, int T, int clamp_lat_dim, const float* cmask, const float* gmask, uint64_t seed,
                               float p_drop, float* trj_out, float* y_last, float* h_last, void* tape, size_t tape_bytes,
                               void* scratch, size_t scratch_bytes, void* stream);

/*
 * Backward of that pass (the autograd the reference gets from `batch_loss.backward()`, train...:1419): dout [B,T,Cout] is
 * d loss / d trj_out; y_last / h_last are treated as detached (train...:1301).  Writes dx [B,T,Cin] (may be NULL) and the
 * parameter gradients (accumulate != 0 adds to what is there).
 */
/*
 * cvae_set_side_stream (process-wide, NULL = off, the default): when cvae_gru_rnn_backward is called with accumulate != 0, the
 * four weight-gradient contractions of the recurrent / projection weights and their bias sums -- results nothing in the same
 * backward chain reads -- are enqueued on this second stream, so that they overlap the NEXT pass's reverse recurrence (a
 * latency-bound kernel that leaves most of every CU idle).  The caller then must (1) give consecutive backward calls of a net
 * different `scratch` buffers (the library makes a call wait for the side work that last used its scratch), (2) keep the `tape` of
 * a pass alive until the join, (3) call cvae_join_side_stream(stream) before anything on `stream` reads the gradient buffers.
 * The reference has no counterpart: autograd runs its backward on one stream.
 */
int cvae_set_side_stream(cvae_ctx* ctx, void* stream);
int cvae_join_side_stream(cvae_ctx* ctx, void* stream);

int cvae_gru_rnn_backward(cvae_ctx* ctx, const cvae_net_desc* d, const void* image, const float* dout, int B, int T, int clamp_lat_dim,
                          const void* tape, void* scratch, size_t scratch_bytes, float* dx, const cvae_net_grads* g,
                          int accumulate, void* stream);

/* With the option "train_profile" set, every launch (or per-step launch sequence) of the training recurrences and every training
 * GEMM (its split-contraction reduction included) is bracketed by a HIP event pair on the stream it is launched on.  This call waits
 * for them and returns, per class {0 forward recurrence, 1 reverse recurrence, 2 forward / data-gradient GEMMs, 3 weight-gradient
 * contractions}, the summed duration (ms), the number of brackets and the summed 2*M*N*K of the GEMM classes; then forgets them.
 * Measurement only (an event record leaves ~6 us of idle stream on either side of a launch). */
int cvae_train_profile_collect(cvae_ctx* ctx, double total_ms[4], int launches[4], double flop[4]);

/* Debugging aid: with the option "train_prof" set, block 0 of the persistent training forward recurrence
 * accumulates shader-cycle sums per phase {poll, loads+MFMA, reduce+cell math, publish} in out[0..3] (out[4..7] unused). */
int cvae_train_debug_counters(cvae_ctx* ctx, const cvae_net_desc* d, int B, int T, const void* scratch, long long out[8], void* stream);

/* torch.optim.Adam semantics (no weight decay), `step` counted from 1 (train...:377, :1420), over one flat buffer.
 * gate: NULL, or an int32 the DEVICE can read (normally the status sink of cvae_set_status_sink): when it is non-zero at the time
 * the kernel runs -- a hand-off timed out or a gate gradient left the exchange range during this step -- the update is skipped and
 * parameters and moments keep their values, so a bad step can never corrupt the optimiser state. */
int cvae_adam_step(cvae_ctx* ctx, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1,
                   float beta2, float eps, int step, const int32_t* gate, void* stream);
/* The same update with the step counter ON THE DEVICE (ABI 4): state = int32[4] in device memory, state[0] = number of updates
 * applied so far (the caller zeroes it once, or writes the `step` of a resumed optimiser), state[1..2] scratch for the bias
 * corrections.  The counter advances only when the gate lets the update through, so a loop that does not synchronise every step
 * keeps Adam's bias correction right across skipped steps -- on every data-parallel rank alike, since `gate` is then the
 * MAX-reduced latch of cvae_status_latch. */
int cvae_adam_step_counted(cvae_ctx* ctx, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1,
                           float beta2, float eps, int32_t* state, const int32_t* gate, void* stream);

/*
 * Stage-4 glue between the passes of a training step (no GEMM: element-wise, one launch each).
 *
 * cvae_sample_cat: the decoder input of train...:1335-1338, [code ; sampling_vae_batch(lat)] (gru_vae.py:85-98 + torch.cat), for
 * `parts` = 1 pass or for the two passes rec || cv stacked along the batch axis (parts = 2: rows [0,B) use code0 / eps0 / draw0,
 * rows [B,2B) code1 / eps1 / draw1).  lat [B][T][2L]; code [B][T][ncode]; eps NULL = Philox keyed (seed, draw, global frame, dim)
 * like cvae_sample; out [parts*B][T][ncode+L]; eps_out [parts][B][T][L] receives the eps used (the backward reads it).
 * cvae_sample_cat_backward: dout [parts*B][T][ncode+L] -> dlat [B][T][2L] (written, not accumulated).
 *
 * cvae_stage4_loss: one cycle's terms of the batch loss of train...:1363-1410 and their gradients.  Per frame (b, t) with weight
 * w[b][t] (1/n_j over the first n_j = min(flen_acc[j], T) frames of a selected utterance, else 0: the mean over frames, summed
 * over utterances):  w * ( K |rec - tgt|_1 + K |reccyc - tgt|_1 + kl_scale KL(lat) + latcv_w[b] KL(latcv) ),
 * K = 10/ln10 sqrt2 (gru_vae.py:525-527), KL = 0.5 sum(exp(s) + mu^2 - s - 1) (gru_vae.py:117-123), tgt = x[b][t][stdim:stdim+D].
 * kl_scale / latcv_w carry the reference's :1393 quirk (KL(lat) counted twice for more than one selected utterance, KL(latcv) of
 * the last selected utterance only); reccyc / latcv NULL = half cycle (:283-287).  Writes the four gradient arrays (d loss / d
 * trajectory, same shapes), frame_loss [B*T] (scratch) and loss[0] (+= when accumulate != 0) summed in a fixed order.
 */
int cvae_sample_cat(cvae_ctx* ctx, const float* lat, const float* code0, const float* code1, const float* eps0, const float* eps1, uint64_t seed,
                    uint64_t draw0, uint64_t draw1, int B, int T, int lat_dim, int ncode, int parts, float* out, float* eps_out,
                    void* stream);
int cvae_sample_cat_backward(cvae_ctx* ctx, const float* dout, const float* lat, const float* eps, int B, int T, int lat_dim, int ncode, int parts,
                             float* dlat, void* stream);
int cvae_stage4_loss(cvae_ctx* ctx, const float* rec, const float* reccyc, const float* lat, const float* latcv, const float* x, int x_stride, int stdim,
                     const float* w, const float* latcv_w, float kl_scale, int B, int T, int D, int lat_dim, float* d_rec,
                     float* d_reccyc, float* d_lat, float* d_latcv, float* frame_loss, float* loss, int accumulate, void* stream);
/*
 * The script's own per-utterance loss calls (train...:1366-1372) as one launch each way (ABI 4), for the UNCHANGED script flow:
 * cvae_mcd_l1 = TWFSEloss(x, y, twf=None, GV=False, L2=False) (gru_vae.py:525-533): per frame mcd_i = (10/ln10) sqrt2 sum_d |x - y|,
 * out3 = (sum, mean, unbiased std), frame_mcd [frames] kept for the backward; x / y rows of D floats with the given row strides.
 * cvae_mcd_l1_backward: dx [frames][D] from the three upstream gradients g3 (device).  cvae_kl_gauss = loss_vae (gru_vae.py:117-123):
 * mean over frames of 0.5 sum_l (exp(s) + mu^2 - s - 1), param rows [mu | s] of 2 * lat_dim floats; cvae_kl_gauss_backward: dparam
 * [frames][2 * lat_dim] contiguous.  As torch ops these are ~8 launches forward and as many autograd nodes backward per call, five
 * calls per utterance and cycle.
 */
int cvae_mcd_l1(cvae_ctx* ctx, const float* x, long x_stride, const float* y, long y_stride, int frames, int D, float* frame_mcd, float* out3, void* stream);
int cvae_mcd_l1_backward(cvae_ctx* ctx, const float* x, long x_stride, const float* y, long y_stride, int frames, int D, const float* frame_mcd,
                         const float* out3, const float* g3, float* dx, void* stream);
int cvae_kl_gauss(cvae_ctx* ctx, const float* param, long stride, int frames, int lat_dim, float* out1, void* stream);
int cvae_kl_gauss_backward(cvae_ctx* ctx, const float* param, long stride, int frames, int lat_dim, const float* g1, float* dparam, void* stream);

/*
 * Stage-6 post-processing next to the decoder output, f64 on the device like the reference's numpy on
 * the host.  GV post-filter, decode_gru-cyclevae_gauss.py:417-420:
 *   mean_d = mean_t c[t][d];  out[t][0] = c[t][0] (+ dpow[t]);  out[t][d] = sqrt(gv_trg[d-1]/cvgv[d-1]) * (c[t][d]-mean_d) + mean_d
 * c [T][D] fp32 (the decoder trajectory); dpow NULL or [T] (the power correction of mod_pow, feature_extract_vc.py:131-138,
 * whose SPTK mc2e is out of scope); gv_trg, cvgv [D-1]; out [T][D] f64; out_var NULL or [D-1] = np.var(out[:,1:], 0)
 * (decode...:421); work: 2*D doubles of device scratch.
 */
int cvae_gv_postfilter(cvae_ctx* ctx, const float* c, int T, int D, const double* dpow, const double* gv_trg, const double* cvgv, double* out,
                       double* out_var, double* work, void* stream);

/*
 * Energy of the impulse response of every frame's mel-cepstrum, f64: SPTK's mc2e, which the reference reaches through
 * pysptk.mc2e in mod_pow (feature_extract_vc.py:131-138; decode_gru-cyclevae_gauss.py:406: the power correction
 * dpow = log(mc2e(mcep) / mc2e(cvmcep)) / 2 added to coefficient 0, i.e. the `dpow` argument of cvae_gv_postfilter):
 * c' = freqt(mc, irlen - 1, -alpha), h = c2ir(c', irlen), e = sum h^2.  mc [T][ld] device memory, float32 (is_f64 = 0) or
 * float64; e_out [T].  pysptk is not in the reference tree nor in this image: restated from SPTK's published freqt / c2ir.
 */
int cvae_mc2e(cvae_ctx* ctx, const void* mc, int is_f64, long ld, int T, int D, double alpha, int irlen, double* e_out, void* stream);

/*
 * Frame-wise mel-cepstral distortion of two ALIGNED sequences over coefficients d0..D-1, f64 (gru_vae.py:523 L2 / :525 L1;
 * the per-frame values dtw_c.calc_mcd is called for at decode...:377-378 with d0 = 0 "mcdpow" and d0 = 1 "mcd").
 * a, b [rows][ld] fp32; frames [rows] f64; stats NULL or [4] = sum, mean, population std (np.std), sample std (torch.std).
 */
int cvae_mcd_aligned(cvae_ctx* ctx, const float* a, long lda, const float* b, long ldb, int rows, int D, int d0, int l2, double* frames,
                     double* stats, void* stream);

/*
 * Dynamic time warping of org [T1][D] onto the time axis of trg [T2][D], f64, on the device -- the role of dtw_c.dtw_org_to_trg at
 * decode_gru-cyclevae_gauss.py:334-364, :424 and train...:679-688 (there: a D2H copy per utterance and a host library).  dtw_c's
 * source is not in the reference tree: PARITY UNPINNED; the algorithm is the textbook one, every choice documented at
 * oracle/cyclevae_oracle.py::dtw_org_to_trg (local cost mel-cd, or cosine distance with mcd = 0; steps (1,1), (1,0), (0,1) with unit
 * weights; free of windows; target frame j takes the path's org frame of smallest local cost).  Outputs: aligned [T2][D], twf [T2]
 * (int64 org index per target frame), frames [T2] (their local costs), mean_out [1].  work: cvae_dtw_work_bytes(T1, T2) of device memory.
 */
size_t cvae_dtw_work_bytes(cvae_ctx* ctx, int T1, int T2);
int cvae_dtw_org_to_trg(cvae_ctx* ctx, const double* org, const double* trg, int T1, int T2, int D, int mcd, double* aligned, long long* twf,
                        double* frames, double* mean_out, void* work, size_t work_bytes, void* stream);

/*
 * Batched DTW (the per-epoch validation pass, train_gru_cyclevae_gauss_batch.py:895-951: twelve alignments per utterance pair).
 * P problems of cvae_dtw_org_to_trg in ONE call whose launch count does not depend on P: per chunk one copy of the problem
 * list into the head of `work`, (option dtw_batch_cost = 1) one grid-wide local-cost kernel, and one path kernel with ONE BLOCK
 * PER PROBLEM.  A block keeps the two previous anti-diagonals of the accumulated cost in LDS (three rotating rows of T1 doubles;
 * T1 > CVAE_DTW_LDS_ROWS: in `work`), stores one back-pointer byte per cell, follows the bytes back from (T1-1, T2-1), and warps.
 * Blocks are independent ordinary kernels: no cooperative launch, no flags between blocks.
 * Semantics and bits are those of cvae_dtw_org_to_trg (oracle/cyclevae_oracle.py::dtw_org_to_trg; PARITY UNPINNED as there): steps
 * (i-1,j-1), (i-1,j), (i,j-1), unit weights, strict "<" in that order; target frame j takes the path's org frame of smallest local
 * cost, "<=" walking backwards; mean_out = mean of those costs.  The local cost is k_dtw_cost's expression in k_dtw_cost's
 * summation order.
 * probs: HOST array (read before the call returns).  org [T1][ld_org], trg [T2][ld_trg] f64 device; aligned NULL or [T2][D];
 * twf [T2]; frames [T2]; mean_out [1].  Outputs of different problems must not overlap; inputs may be shared.
 * work: cvae_dtw_batch_work_bytes(P, max T1, max T2) bytes of device memory, which is the need of all P problems at once or
 * CVAE_DTW_BATCH_WORK_CAP, whichever is smaller (never less than ONE problem needs): cvae_dtw_batch splits P into consecutive
 * chunks that fit `work_bytes` and runs them one behind the other on `stream`.
 */
#define CVAE_DTW_BATCH_WORK_CAP ((size_t)1 << 30)
#define CVAE_DTW_LDS_ROWS 2048
typedef struct cvae_dtw_problem {
    const double* org;
    const double* trg;
    int64_t ld_org, ld_trg;      /* row strides in doubles, >= D */
    int32_t T1, T2, D;
    int32_t mcd;                 /* non-zero: mel-cd local cost [dB]; 0: cosine distance */
    double* aligned;             /* NULL: not wanted */
    long long* twf;
    double* frames;
    double* mean_out;
} cvae_dtw_problem;
size_t cvae_dtw_batch_work_bytes(cvae_ctx* ctx, int P, int T1max, int T2max);
int cvae_dtw_batch(cvae_ctx* ctx, const cvae_dtw_problem* probs, int P, void* work, size_t work_bytes, void* stream);

/*
 * Batched utterance statistics of the validation pass: ONE launch, one block per job, f64 arithmetic on fp32 inputs, every
 * reduction a fixed-order tree (the result does not depend on the grid).  jobs: n descriptors in DEVICE-visible memory (the
 * caller uploads the list it built on the host; bad descriptors cannot be refused from the host side -- a row index outside
 * 0 .. src_rows-1 makes the job's results NaN instead of reading there).  Results of kinds other than GATHER64 go to
 * out[out_off ...].
 *   CVAE_STAT_GV        out[c - c0] = population variance (two-pass) over rows 0 .. rows-1 of column c of a, c0 <= c < c1
 *                       (np.var(traj[:flen, 1:], axis=0) with c0 = 1, c1 = D: train...:888-893, there in float32)
 *   CVAE_STAT_MCD_SPC   out[0] = mean over k < rows of (10/ln10) sqrt(2 sum_{c0 <= c < c1} (a[idx[k]][c] - b[idx[k]][c])^2)
 *                       (dtw_c.calc_mcd on the speech frames, :932-948; a and b are given at their first compared column's origin)
 *   CVAE_STAT_MCD_L1    out[0] = mean over t < rows of (10/ln10) sqrt2 sum_{c < c1} |a[t][c] - b[t][c]|     (criterion_mcd(L2=False,
 *                       GV=False)'s mean, :1006-1013; cvae_mcd_l1's second output, here in f64)
 *   CVAE_STAT_KL        out[0] = mean over t < rows of 0.5 sum_{l < c1} (exp(s) + mu^2 - s - 1), a[t] = [mu (c1) | s (c1)]
 *                       (loss_vae, :1015-1019; cvae_kl_gauss in f64)
 *   CVAE_STAT_KL_LAPLACE  out[0] = mean over t < rows of sum_{l < c1} (-s + b exp(-|mu|/b) + |mu| - 1), b = exp(s), the operands of
 *                       CVAE_STAT_KL in its summation order (loss_vae_laplace, gru_vae.py:130-139: the Laplace posterior's loss_lat_*)
 *   CVAE_STAT_GATHER64  dst[k][c - c0] = (double)a[idx[k]][c], k < rows, c0 <= c < c1: the packed f64 DTW operands of :895-951
 *   CVAE_STAT_LATDIST   out[0] = mean_c sqrt(mean_t (a[t][c] - b[t][c])^2), a and b F64 [rows][lda / ldb], c < c1      (:898)
 */
enum { CVAE_STAT_GV = 0, CVAE_STAT_MCD_SPC = 1, CVAE_STAT_MCD_L1 = 2, CVAE_STAT_KL = 3, CVAE_STAT_GATHER64 = 4, CVAE_STAT_LATDIST = 5 };
typedef struct cvae_stat_job {
    int32_t kind, rows;          /* rows: flen, n_spc, or the rows of the aligned pair */
    int32_t c0, c1;
    int32_t src_rows, pad_;      /* rows of a (and b) that idx may address */
    const void* a;
    const void* b;
    int64_t lda, ldb;            /* row strides in elements */
    const int64_t* idx;          /* MCD_SPC, GATHER64: rows int64 frame indices */
    double* dst;                 /* GATHER64: [rows][c1 - c0] */
    int64_t out_off;
} cvae_stat_job;
int cvae_eval_stats(cvae_ctx* ctx, const cvae_stat_job* jobs, int n, double* out, void* stream);
/*
 * Two further job kinds (stage 5, calc_cvgv_gru-cyclevae_gauss.py:210-249), F64 operands; out[0] = np.mean, out[1] = np.std
 * (population, two-pass) of a per-frame array.  src_rows: the rows the operands hold -- rows outside 1 .. src_rows give NaN, NaN
 * instead of a read behind them.
 *   CVAE_STAT_MEANSTD64 the array is a[t * lda], t < rows: the per-frame costs a DTW problem leaves in `frames` (lda = 1)   (:212-215)
 *   CVAE_STAT_MCD64     the array is (10/ln10) sqrt(2 sum_{c0 <= c < c1} (a[t][c] - b[t][c])^2), t < rows, a and b [rows][lda / ldb]
 *                       given at column 0: dtw_c.calc_mcd's frame array as oracle.mcd_aligned defines it (PARITY UNPINNED)   (:224-229)
 */
enum { CVAE_STAT_MEANSTD64 = 6, CVAE_STAT_MCD64 = 7 };
enum { CVAE_STAT_KL_LAPLACE = 8 };       /* (listed with CVAE_STAT_KL above) */

/*
 * The n_draws-draw latent mean of stage 5 / 6 as an array of its own (calc_cvgv_gru-cyclevae_gauss.py:180-184: lat_feat, which the
 * script feeds to the decoder AND aligns with DTW; inside the pass prologue the same mean is never written out).  One launch per
 * 32 jobs of a HOST list (read before the call returns):
 *   out[t][l] = lat[t][l] + exp(lat[t][L + l] / 2) * (sum_{k < n_draws} eps_k[t][l]) / n_draws,   t < frames, l < L = lat_dim
 * lat [frames][2L], out [frames][L] fp32 device; eps NULL, or [n_draws][frames][L] fp32 device.  eps NULL: draw k of frame t is keyed
 * (seed, draw_id + k, t, l) through cvae_randn4, as the pass prologue keys the draws of a single-row cell (the data-parallel draw
 * origin does not enter).  The draws are added in the order k = 0, 1, ... by one thread per (frame, four dims), with either source
 * of eps: the result does not depend on the grid.  Any lat_dim >= 1 (not only multiples of 4), n_draws >= 1, frames >= 1.
 */
typedef struct cvae_latmean_job {
    const float* lat;
    const float* eps;
    uint64_t draw_id;
    int32_t frames, pad_;
    float* out;
} cvae_latmean_job;
int cvae_latent_mean(cvae_ctx* ctx, const cvae_latmean_job* jobs, int n_jobs, int lat_dim, int n_draws, uint64_t seed, void* stream);

/*
 * Stage 6 in batched form (decode_gru-cyclevae_gauss.py:328-475: per utterance pair six mod_pow, three GV post-filters, two
 * differential cepstra).  Both entry points take a HOST job list (read before the call returns) and issue a number of launches that
 * does not depend on the list's length.
 *
 * cvae_mc2e_batch: cvae_mc2e's energies (same semantics, oracle.mc2e) for every frame of every job at one (alpha, irlen):
 * mc [T][ld] float32 (is_f64 = 0) or float64, D >= 2 coefficients, e_out [T].  One copy of the list, one kernel that builds the
 * freqt map of the call (it depends on alpha, irlen and the largest D only), one kernel with a 64-lane block per frame.  irlen 2 ..
 * 4000 with (2 irlen + max D + 64) doubles of LDS <= 64 KiB.  work: cvae_mc2e_batch_work_bytes(n_jobs, max D, irlen) bytes of device
 * memory (0: bad arguments).  A frame's energy does not depend on the other frames or jobs of the call.
 */
typedef struct cvae_mc2e_job {
    const void* mc;
    int32_t is_f64, T, D, pad_;
    int64_t ld;                  /* row stride in elements, >= D */
    double* e_out;
} cvae_mc2e_job;
size_t cvae_mc2e_batch_work_bytes(cvae_ctx* ctx, int n_jobs, int Dmax, int irlen);
int cvae_mc2e_batch(cvae_ctx* ctx, const cvae_mc2e_job* jobs, int n_jobs, double alpha, int irlen, void* work, size_t work_bytes,
                    void* stream);
/*
 * cvae_decode_jobs: one launch, one block per job, f64, fixed-order reductions.
 *   CVAE_DEC_MODPOW  c [T][ldc] (float32, or float64 with c_f64 = 1) -> x [T][D] f64:
 *                      x[t][0] = c[t][0] + log(e_ref[t] / e_c[t]) / 2   (mod_pow, feature_extract_vc.py:131-138; e_ref or e_c NULL: + 0)
 *                      x[t][d] = c[t][d], d >= 1;        dpow NULL or [T]: the correction that was added
 *                    x may be c itself (c_f64 = 1, ldc = D): the in-place correction of decode...:432.
 *                    diff NULL or [T][D]: x - ref, ref [T][ldref] float32 / float64 (ref_f64)                        (:470, :474)
 *                    gv NULL or [D-1], then cvgv [D-1], g [T][D], var [D-1]: the post-filter of :419-422 applied to x,
 *                      g[t][0] = x[t][0];  g[t][d] = sqrt(gv[d-1] / cvgv[d-1]) (x[t][d] - mean_t x[.][d]) + mean_t x[.][d]
 *                      var = np.var(g[:, 1:], axis=0) (two-pass)
 *   CVAE_DEC_GATHER  x[k][c - c0] = c[idx[k]][c], k < T, c0 <= c < c1, c float32 / float64; an index outside 0 .. src_rows-1 gives
 *                    a NaN row instead of a read there (cvae_eval_stats' GATHER64 for f64 sources)
 * work: n_jobs * sizeof(cvae_decode_job) bytes of device memory.  Outputs of different jobs must not overlap.
 */
enum { CVAE_DEC_MODPOW = 0, CVAE_DEC_GATHER = 1 };
typedef struct cvae_decode_job {
    int32_t kind, T, D, c_f64;
    int32_t ref_f64, src_rows, c0, c1;
    const void* c;
    int64_t ldc;
    const double* e_ref;
    const double* e_c;
    const double* gv;
    const double* cvgv;
    double* x;
    double* g;
    double* var;
    double* dpow;
    const void* ref;
    int64_t ldref;
    double* diff;
    const int64_t* idx;
} cvae_decode_job;
int cvae_decode_jobs(cvae_ctx* ctx, const cvae_decode_job* jobs, int n_jobs, void* work, size_t work_bytes, void* stream);

/*
 * The per-window half of the stage-4 training log (train_gru_cyclevae_gauss_batch.py:1364-1371, :1431-1439, and the buffers of
 * :1312-1316 / :1349-1353): ONE launch per frame window (one per CVAE_TRAINLOG_MAX_UTT utterances), one block per (cycle i,
 * utterance j), f64 arithmetic on the fp32 trajectories, every reduction a fixed-order tree: a record does not depend on the grid
 * nor on the other utterances of the call.  The call reads the four HOST arrays before it returns, copies nothing and waits for
 * nothing: the generator's bookkeeping travels as kernel arguments.
 *   traj[i]      the five trajectories of cycle i as stage4.chain_forward returns them, contiguous fp32 device arrays:
 *                [0] lat [B][T][2L], [1] rec [B][T][D], [2] cv [B][T][D], [3] latcv [B][T][2L], [4] reccyc [B][T][D]
 *   x_win        batch_src[0][src_idx_s]: the window's T rows of every utterance, row stride x_row_stride >= stdim + D floats,
 *                utterance stride x_utt_stride; the target of a frame is its columns stdim .. stdim + D - 1
 *   spcidx       [B][spc_ld] int64 device: the utterances' speech-frame indices
 *   selected, flen_acc, s_idx, e_idx    HOST [B]: select_utt_idx as a 0/1 array, and the generator's flen_acc, spcidx_src_s_idx,
 *                spcidx_src_e_idx
 * rec_out [n_cyc][B][9] f64 device:
 *   [0..4]  utterance selected and n = min(flen_acc[j], T) > 0: the means over the window's frames 0 .. n-1 of
 *           (10/ln10) sqrt2 sum_d |y[t][d] - x[t][stdim + d]| for y = rec, reccyc, cv   (criterion_mcd(L2=False, GV=False), :1366-1368)
 *           and of 0.5 sum_l (exp(s) + mu^2 - s - 1) for lat, latcv                        (loss_vae, :1370-1371); else NaN.
 *           L given as L | CVAE_DRAW_LAPLACE: the last two are the means of sum_l (-s + b exp(-|mu|/b) + |mu| - 1), b = exp(s)
 *           (loss_vae_laplace, gru_vae.py:130-139); nothing else of the call changes
 *   [5..8]  utterance selected, s_idx[j] >= 0: with f_k = spcidx[j][s_idx[j] + k], k <= e_idx[j] - s_idx[j], r_k = f_k - src_idx_s,
 *           the means over k of (10/ln10) sqrt(2 sum_{d >= d0} (x[r_k][stdim + d] - y[r_k][d])^2) for (y, d0) = (rec, 0), (rec, 1),
 *           (reccyc, 0), (reccyc, 1): dtw_c.calc_mcd as oracle.mcd_aligned defines it (PARITY UNPINNED), :1435-1439.  An r_k outside
 *           0 .. T-1 or an e_idx outside the index rows gives the utterance's four figures NaN instead of a read there; else NaN
 * acc: all NULL, or the four utterance-long buffers [B][acc_rows][D] (rec, cv, reccyc) and [B][acc_rows][2L] (lat): the blocks of
 *   cycle 0 copy the window's T rows of EVERY utterance to rows src_idx_s .. src_idx_s + T - 1 (refused when they do not fit).
 */
#define CVAE_TRAINLOG_MAX_CYC 8
#define CVAE_TRAINLOG_MAX_UTT 128
typedef struct cvae_trainlog_window_args {
    const float* traj[CVAE_TRAINLOG_MAX_CYC][5];
    const float* x_win;
    int64_t x_row_stride, x_utt_stride;
    const int64_t* spcidx;
    int64_t spc_ld;
    const int32_t* flen_acc;
    const int32_t* s_idx;
    const int32_t* e_idx;
    const uint8_t* selected;
    int32_t n_cyc, B, T, D, L, stdim, src_idx_s, acc_rows;
    float* acc[4];
    double* rec_out;
} cvae_trainlog_window_args;
int cvae_trainlog_window(cvae_ctx* ctx, const cvae_trainlog_window_args* a, void* stream);

/*
 * Live streams (stream.py: StreamConverter) -- a list of strided row copies as ONE launch: element (r, c) of a job, r < rows,
 * c < width, goes from src[r * src_stride + c] to dst[r * dst_stride + c] (fp32 device arrays, strides in floats).  A stream step
 * appends the frames pushed since the last step to its sessions' input buffers, compacts their buffers and packs their converted
 * frames with one call each, whatever the number of sessions (as single copies: 3 x sessions launches per step).  `jobs` is a HOST
 * array read before the call returns; the table travels in the kernel arguments, 96 jobs per launch (more: several launches).
 * rows == 0 jobs are legal and do nothing.  Refused (-1, nothing enqueued): a null pointer with rows > 0, a negative field, width
 * larger than a stride, a job whose source and destination ranges overlap (blocks run in no order).  16-byte accesses where both
 * pointers and both strides of a job are 16-byte aligned, single floats for the rest of a row and for every other job.
 */
typedef struct cvae_move_job {
    float* dst;
    const float* src;
    int32_t rows, width;
    int64_t dst_stride, src_stride;
} cvae_move_job;
int cvae_stream_move(cvae_ctx* ctx, const cvae_move_job* jobs, int njobs, void* stream);

/* Copy status words (int32[4]) of a workspace to the host; synchronises `stream`.  status[0]!=0 = barrier timeout;
 * status[3] == CVAE_STATUS_RANGE: the latest call on this workspace met an operand outside the limb window (no sink set). */
int cvae_workspace_status(cvae_ctx* ctx, const void* workspace, int32_t status_out[4], void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CYCLEVAE_HIP_H */
