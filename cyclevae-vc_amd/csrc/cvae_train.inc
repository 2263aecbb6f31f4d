// Training entry points of libcyclevae_hip.so (included by cvae_lib.hip): train-mode forward with a tape, BPTT backward,
// Adam.  The recurrences are persistent cooperative launches where the size allows (H = 1024, 64: exact-operand kernels of
// cvae_train_w3.h / cvae_train_x3.h by default, fp16-pair kernels with train_kernel = 1) and per-step launches otherwise, in the
// forms plan_train_pass chooses; everything batched is an MFMA GEMM over time-major buffers (cvae_train_kernels.h).
// A pass is a TrainPass (dimensions, layouts, plan, pointers) run through named stages.  Forward: draw_train_masks, run_train_prologue,
// run_train_front_end, run_fwd_recurrence, run_train_projection.  Backward: wait_for_side_scratch, run_bwd_dy, run_bwd_recurrence or
// run_bwd_steps, launch_wgrad / launch_wgrad_side, run_input_chain, run_conv_wgrad (DESIGN.md 4.2).
namespace {

struct TDims {
    int Cq, C3, C3p, C9, C9p, K0, K1, F0, Tp;
};

TDims make_tdims(const Dims& m, int T) {
    TDims t;
    t.Cq = (int)up(m.C, 16);
    t.C3 = m.cl[0];
    t.C3p = (int)up(m.cl[0], 16);
    t.C9 = m.cl[1];
    t.C9p = (int)up(m.cl[1], 16);
    t.K0 = m.ks * t.Cq;
    t.K1 = m.ks * t.C3p;
    t.F0 = T + m.R - m.ks;   // conv0 output frames
    t.Tp = T + m.R - 1;      // padded input frames
    return t;
}

// the persistent training recurrences (all-resident grids, weights in registers / LDS) are built for these sizes
inline bool persist_ok(const Dims& m) { return m.H == 1024 || m.H == 64; }
inline int x3_kpw(const Dims& m) { return m.H / 64; }
inline int w3_gpw(const Dims& m) { return m.H >= 128 ? m.H / 128 : 1; }      // 32-unit producer groups per wave (k_train_bwd_steps_w3)

// Which MFMA-order weight images a train image holds (cvae_net_prepare_train_v): bit 0 the exact-operand tile kernels (w3f, w3h,
// wbk3, wfw3, wbw3), bit 1 the fp16-pair kernels (wrec_t8, wrec_t8h, wbk), bit 2 the fp32-MFMA persistent forward (wrec_t8).  The
// GEMM-form weights, the per-step images (wrec_t, wbp) and the fp32 image the word-exchange kernels read are always built.
enum { TV_EXACT = 1, TV_PAIR = 2, TV_FP32 = 4, TV_ALL = 7 };

// The recurrence forms of a training pass.  Forward: word exchange (<= 3 rows, cvae_train_ll.h), exact operands in 16-unit blocks
// (cvae_train_w3.h), in 8-unit blocks with 32- or 16-row tiles (cvae_train_x3.h), the fp16-pair or fp32-MFMA persistent kernel
// (cvae_train_kernels.h), T per-step launches.  Reverse: word exchange, exact operands in 16- or 8-unit blocks, fp16 pairs
// (cvae_train_bwd.h), 2T per-step launches.
enum FwdForm { FWD_LL, FWD_W3, FWD_X3, FWD_X3H, FWD_PAIR, FWD_FP32, FWD_STEPS };
enum BwdForm { BWD_LL, BWD_W3, BWD_X3, BWD_PAIR, BWD_STEPS };

struct TrainPlan {
    int Bp;                  // rows per frame of the time-major tape and scratch
    FwdForm fwd;
    int fwd_rts;             // row tiles side by side: (H / units per block) x rts blocks, a block takes tiles i, i + rts, ...
    int fwd_col_tiles;       // 16-column tiles per block of FWD_STEPS (and of the run-time fall-back to it)
    int fwd_backoff;         // before the first flag poll of a step / task (FWD_LL: its own units)
    int fwd_need;            // image variant without which the pass is refused (-4)
    bool fwd_full_writes;    // the gate tape and the state copies need no memset
    BwdForm bwd;
    int bwd_rts, bwd_backoff;
    int bwd_per_launch;      // row tiles per launch of BWD_W3 / BWD_X3 (0: the whole pass in one)
    bool bwd_writes_gates;   // every row of dgi / dgh written by the reverse recurrence (dead rows as zeros): no memset
    int variants;            // the weight images the forms of this shape may need, their fall-backs included
    // what cvae_plan_train_pass reports on top (tests): the most row tiles one block row owns -- per step in the forward (32-row
    // tiles of FWD_X3, 16-row tiles otherwise), per launch in the reverse; 0 for the forms without row tiles (LL, STEPS)
    int fwd_tiles, bwd_tiles;
};

// THE place where a training pass's recurrence forms are chosen: forward and backward of a pass call it with the same shape and
// must see the same options (the tape layout depends on it).  Today's rule, as a table: DESIGN.md section 4.2.
TrainPlan plan_train_pass(const Dims& m, int B, int T) {
    const bool ok = persist_ok(m), fp32 = opt(OPT_TRAIN_FP32_MFMA) != 0, per_step = opt(OPT_TRAIN_PER_STEP) != 0,
               bwd_per_step = opt(OPT_TRAIN_BWD_PER_STEP) != 0, no_ll = opt(OPT_NO_LL) != 0, exact = opt(OPT_TRAIN_KERNEL) == 0;
    const long x3_tile = opt(OPT_X3_TILE), max_rt = opt(OPT_MAX_RT), fwd_geom = opt(OPT_TRAIN_FWD_GEOM), bwd_geom = opt(OPT_TRAIN_BWD_GEOM);
    const int cus = cu_count();
    // as many of the pass's `tiles` row tiles side by side as leave every block of `units` units a CU of its own (option max_rt caps it)
    auto fit = [&](int units, int tiles) {
        int r = cus / (m.H / units);
        r = r > tiles ? tiles : r;
        r = r < 1 ? 1 : r;
        return max_rt >= 1 && max_rt < r ? (int)max_rt : r;
    };
    // blocks with ONE tile sleep before their first poll (nothing else covers the hand-off; early polls slow the publishes)
    auto backoff = [](long o, int tiles, int rts, int one_tile) { return o >= 0 ? (int)o : (tiles + rts - 1) / rts == 1 ? one_tile : 0; };
    const int ll_backoff = opt(OPT_LL_BACKOFF) >= 0 ? (int)opt(OPT_LL_BACKOFF) : (B == 1 ? 18 : 16);
    TrainPlan p = {};

    // at most three rows: the word-exchange kernels.  They address rows by stride only, so when both directions run them the
    // time-major buffers hold exactly B rows per frame (option ll_row_pad): every GEMM of a one-utterance pass runs over T rows.
    // (the forward's choice does not look at train_bwd_per_step: with it, a pass of <= 3 rows runs the forward on 16 rows per frame)
    const bool ll_fwd = exact && !fp32 && !per_step && !no_ll && B <= 3 && T > 1 && T < 65536 && ok && cus >= m.H / 4;
    const bool ll_rows = ll_fwd && !bwd_per_step;
    // 4..16 rows: ONE 16-row tile; else the exact kernels' 32-row tiles
    p.Bp = ll_rows ? (opt(OPT_LL_ROW_PAD) > 0 ? (int)opt(OPT_LL_ROW_PAD) : B) : B <= 16 && ok && x3_tile != 32 ? 16 : (int)up(B, ok ? 32 : 16);
    const int nt16 = p.Bp / 16, nrt32 = p.Bp / 32;
    const long mtot = (long)(T + 1) * p.Bp;

    // ---- forward
    p.fwd = FWD_STEPS;
    if (ll_fwd) {
        p.fwd = FWD_LL;
        p.fwd_backoff = ll_backoff;
    } else if (exact && !fp32 && !per_step && ok && T > 1) {
        p.fwd_need = TV_EXACT;
        const long fbo = opt(OPT_TRAIN_FWD_BACKOFF);
        const int rt32 = fit(8, nrt32), ntile32 = (nrt32 + rt32 - 1) / rt32;
        const bool fits8 = cus >= m.H / 8 && (long)m.nch * mtot * 80 < (1L << 31);
        if (cus >= m.H / 16 && (long)(T + 1) * (m.H / 32) * nt16 * 2560 < (1L << 32) &&
            (fwd_geom == 1 || (fwd_geom < 0 && x3_tile == 0 && nt16 >= 4))) {
            p.fwd = FWD_W3;                  // 64 rows on: 16-unit blocks (64 rows: one tile per block behind the back-off)
            p.fwd_rts = fit(16, nt16);
            p.fwd_backoff = backoff(fbo, nt16, p.fwd_rts, 24);
        } else if (fits8 && ntile32 <= 4 && (x3_tile == 32 || (x3_tile != 16 && ntile32 >= 2))) {
            p.fwd = FWD_X3;                  // 32-row tiles where a block gets at least two (h kept in registers: at most four)
            p.fwd_rts = rt32;
        } else if (fits8) {
            p.fwd = FWD_X3H;                 // 16-row tiles
            p.fwd_rts = fit(8, nt16);
            p.fwd_backoff = backoff(fbo, nt16, p.fwd_rts, 24);
        }
    }
    if (p.fwd == FWD_STEPS && !per_step && T > 1 && ok && cus >= m.H / 8 && (long)m.nch * mtot * 64 < (1L << 31)) {
        p.fwd = fp32 ? FWD_FP32 : FWD_PAIR;  // (also where the exact forms do not fit)
        p.fwd_rts = fit(8, nt16);
        p.fwd_backoff = (int)opt(OPT_TRAIN_BACKOFF);
    }
    // per-step launches: two 16-column tiles per block where that still gives every CU a block (hu2048: 256 blocks)
    const long ct = opt(OPT_STEP_COL_TILES);
    p.fwd_col_tiles = (m.H / 4) % 2 == 0 && ct != 1 && (ct == 2 || m.H / 8 >= cus) ? 2 : 1;
    p.fwd_full_writes = T > 1 && !per_step && ok && p.fwd != FWD_LL;

    // ---- reverse
    p.bwd = BWD_STEPS;
    if (ok && !bwd_per_step && T > 1 && cus >= m.H / 8 && (long)T * (m.H / 8) * nt16 * 2560 < (1L << 32)) {
        if (exact && !no_ll && B <= 3 && T < 65536 && cus >= m.H / 4) {
            p.bwd = BWD_LL;
            p.bwd_backoff = ll_backoff;
        } else {
            p.bwd_rts = fit(8, nt16);
            if (exact && cus >= m.H / 16 && (bwd_geom == 1 || (bwd_geom < 0 && nt16 >= 4))) {
                // 16-unit blocks with two tiles each wherever the pass has two: a 64-row pass runs on half the chip, the side
                // stream's weight-gradient GEMMs (which cannot share a CU with such a block) get the other half
                p.bwd = BWD_W3;
                p.bwd_rts = fit(16, nt16);
                if (nt16 >= 2 && p.bwd_rts > nt16 / 2) p.bwd_rts = nt16 / 2;
            } else {
                p.bwd = exact ? BWD_X3 : BWD_PAIR;
            }
            p.bwd_backoff = backoff(opt(OPT_TRAIN_BWD_BACKOFF), nt16, p.bwd_rts, 32);
            // at most two tiles per block and launch (the carried z-path gradient stays in registers; rows are independent)
            if (p.bwd != BWD_PAIR && nt16 > 2 * p.bwd_rts) p.bwd_per_launch = 2 * p.bwd_rts;
        }
    }
    // (a pass of <= 3 rows whose reverse recurrence is not the word-exchange one still zeroes its gate gradients)
    p.bwd_writes_gates = p.bwd != BWD_LL && p.bwd != BWD_STEPS && !(B <= 3 && exact && !no_ll);

    // ---- weight images: the forward's include what it falls back to when its grid or exchange buffer does not fit
    if (!ll_rows) {
        if (!per_step && T > 1) p.variants |= fp32 ? TV_FP32 : exact && ok ? TV_EXACT | TV_PAIR : TV_PAIR;
        if (!bwd_per_step && T > 1 && ok) p.variants |= exact ? TV_EXACT : TV_PAIR;
    }
    if (p.fwd_rts > 0) p.fwd_tiles = ((p.fwd == FWD_X3 ? nrt32 : nt16) + p.fwd_rts - 1) / p.fwd_rts;
    if (p.bwd_rts > 0) p.bwd_tiles = ((p.bwd_per_launch && p.bwd_per_launch < nt16 ? p.bwd_per_launch : nt16) + p.bwd_rts - 1) / p.bwd_rts;
    return p;
}

struct TPrep {
    long w0r, w1r, wix, cfold_t, wrec_t, wrec_t8, wrec_t8h, bhn, whhT, wyT, wbp, wbk, wo, woT, bo, wixT, w1t, w0t, b0, b1, sin_w, sin_b,
        sout_w, sout_b, ffold, w3f, w3h, wbk3, wbw3, wfw3, total;
};

TPrep tprep_layout(const Dims& m, bool sin, bool sout) {
    const TDims t = make_tdims(m, 1);
    TPrep p;
    long o = 0;
    auto take = [&](long n) { long r = o; o += up(n, 64); return r; };
    p.w0r = take((long)t.C3 * t.K0);
    p.w1r = take((long)t.C9 * t.K1);
    p.wix = take((long)m.H3 * t.C9p);
    p.cfold_t = take(m.H3);
    p.wrec_t = take((long)(m.H / 4) * 2 * m.nch * 256);
    p.wrec_t8 = take((long)(m.H / 8) * 2 * 2 * m.nch * 256);
    p.wrec_t8h = take((long)(m.H / 8) * 2 * m.nch * 2 * 256);   // the same weights as fp16 pairs (k_train_fwd_steps_h)
    p.bhn = take(m.H);
    p.whhT = take((long)m.H * m.H3);
    p.wyT = take((long)m.Co * m.H3);
    p.wbp = take((long)(m.H + m.Cop) * m.H3);   // [whhT ; wyT] as 1 KiB MFMA fragments: [col tile][K chunk][16][16]
    // persistent reverse recurrence (k_train_bwd_steps): [W_hh^T | F^T] as fp16 pairs in MFMA operand order, and out_1.w^T
    p.wbk = persist_ok(m) ? take((long)(m.H / 8) * 4 * (m.H / 32) * 2 * 256) : -1;
    p.wo = take((long)m.Cop * m.H);
    p.woT = take((long)m.H * m.Cop);
    p.bo = take(m.Cop);
    p.wixT = take((long)t.C9p * m.H3);
    p.w1t = take((long)t.C3 * m.ks * t.C9p);
    p.w0t = take((long)t.Cq * m.ks * t.C3p);
    p.b0 = take(t.C3);
    p.b1 = take(t.C9);
    p.sin_w = sin ? take((long)m.C * m.C) : -1;
    p.sin_b = sin ? take(m.C) : -1;
    p.sout_w = sout ? take((long)m.Co * m.Co) : -1;
    p.sout_b = sout ? take(m.Co) : -1;
    p.ffold = take((long)m.H3 * m.H);        // F = W_ih[:, C9:] . out_1.w  [3H][H], fp64-accumulated once (k_prep_ffold)
    // exact-operand forward recurrence (k_train_fwd_steps_x3): [W_hh | F] as fp16 triples in MFMA operand order
    p.w3f = persist_ok(m) ? take((long)(m.H / 8) * 4 * 2 * x3_kpw(m) * 3 * 256) : -1;
    p.w3h = persist_ok(m) ? take((long)(m.H / 8) * 2 * 2 * (m.H / 32) * 3 * 256) : -1;   // the same for the 16-row-tile kernel
    p.wbk3 = persist_ok(m) ? take((long)(m.H / 8) * 4 * (m.H / 32) * 640) : -1;       // [W_hh^T | F^T] as triples (k_train_bwd_steps_x3)
    p.wbw3 = persist_ok(m) ? take((long)(m.H / 16) * 4 * w3_gpw(m) * 6 * 640) : -1;    // the same without its zero rows, 16-unit blocks (k_train_bwd_steps_w3)
    p.wfw3 = persist_ok(m) ? take((long)(m.H / 16) * 4 * w3_gpw(m) * 6 * 640) : -1;    // [W_hh | F] without its zero column tiles, 16-unit blocks (k_train_fwd_steps_w3)
    p.total = o;
    return p;
}

struct TTape {   // per pass, lives from forward to backward
    long xnp, c0, cmask, gmask, xcm, hrow, orow, gates, ybuf, zero_end, total;
    int Bp;
};

TTape ttape_layout(const Dims& m, int B, int T, int Bp) {
    const TDims t = make_tdims(m, T);
    TTape p;
    p.Bp = Bp;
    long o = 0;
    auto take = [&](long n) { long r = o; o += up(n, 64); return r; };
    // first what relies on being zeroed (input padding frames, batch padding rows, K padding columns) ...
    p.xnp = take((long)t.Tp * p.Bp * t.Cq + 64);
    p.c0 = take((long)t.Tp * p.Bp * t.C3p);
    p.xcm = take((long)T * p.Bp * t.C9p);
    p.ybuf = take((long)(T + 1) * p.Bp * m.Cop);
    p.zero_end = o;
    // ... then what the persistent recurrences write in full, dead rows included (the per-step path zeroes it as well)
    p.cmask = take((long)B * T * t.C9);
    p.gmask = take((long)T * B * m.H);
    p.hrow = take((long)(T + 1) * p.Bp * m.H);
    p.orow = take((long)(T + 1) * p.Bp * m.H);
    p.gates = take((long)T * p.Bp * 4 * m.H);
    p.total = o;
    return p;
}

static const long GEMM_PART_FLOATS = 16L << 20;   // partial tiles of row-split weight-gradient GEMMs / column sums
static const long GEMM_CNT = 4096;                // arrival counters (one per output tile) of a split GEMM, combined in the launch
static const int BWD_KS = 8;       // K slices of the per-step backward products (k_bwd_step_gemm)
static const int BWD_KS_MAX = 32;  // (the partial-sum area is sized for this many; option bwd_ks)
static const int BWD_NTN = 1;      // 16-column tiles per block of k_bwd_step_gemm (the launch refuses an H / 16 that is no multiple of it)

struct TScratch {   // shared by all passes, contents need not survive a call
    long gi, hbuf, obuf, dy, tflags, tprof, dyl, dytot, dyfb, dh, bpart, gpart, dgi, dgh, dc1p, dc0p, dxn, tmpw, gx, dovl, bflags, gpart2,
        hx3, ox3, dgic, dghc, fcnt, bcnt, bcnt2, llx, total;
};

TScratch tscratch_layout(const Dims& m, int T, long Bp) {
    const TDims t = make_tdims(m, T);
    const long mtot = (long)(T + 1) * Bp;
    TScratch p;
    long o = 0;
    auto take = [&](long n) { long r = o; o += up(n, 64); return r; };
    p.gi = take((long)T * Bp * m.H3);
    p.hbuf = take((long)m.nch * mtot * 16);
    p.obuf = take((long)m.nch * mtot * 16);
    p.dy = take((long)Bp * m.Co);
    p.tflags = take((long)(Bp / 16) * (m.H / 4) + 64);   // flags + status words of the persistent recurrences
    p.fcnt = take(GEMM_CNT);   // arrival counters of the forward pass's split GEMMs: zeroed together with tflags (one memset per pass)
    p.llx = take(2L * 4 * m.H * 4);   // exchange words of the word-exchange recurrences: [2 slots][<= 3 rows (+1)][H][4 floats]
    p.tprof = take(64);   // long long[8]: phase cycle sums of block 0 (forward 0..3, backward 4..7) with the option train_prof
    // exchanged h and o of k_train_fwd_steps_x3: limb triples, 5 bytes per value, tile-planar (2560 B per 16 units x 32 rows)
    p.hx3 = persist_ok(m) ? take((long)m.nch * nblk(mtot, 32) * 640) : -1;
    p.ox3 = persist_ok(m) ? take((long)T * nblk(Bp, 32) * 1024) : -1;        // dropout bits of the feedback operand (k_train_x3_maskbits)
    // partial-sum areas: always written before they are read, so they sit in front of the zeroed backward scratch
    p.bpart = take((long)BWD_KS_MAX * Bp * (m.H + m.Cop));
    p.dgic = take((long)Bp * m.H3);      // one step's gate gradients, chunk-major, for the per-step reverse product
    p.dghc = take((long)Bp * m.H3);
    p.gpart = take(GEMM_PART_FLOATS);
    p.gpart2 = take(GEMM_PART_FLOATS);   // partial tiles of the GEMMs that run on the side stream (cvae_set_side_stream)
    // persistent reverse recurrence: exchanged gate gradients (one 2 KiB tile per step, producer octet and 16-row tile) and
    // W_o^T dyl_t for every step
    p.gx = persist_ok(m) ? take((long)T * (m.H / 8) * (Bp / 16) * 640) : -1;   // (640: the 2.5 KiB pieces of the triple form)
    p.dovl = persist_ok(m) ? take((long)T * Bp * m.H) : -1;
    // gate gradients: the persistent reverse recurrence writes every row of them (dead rows as zeros); the per-step path relies
    // on a memset of its own
    p.dgi = take((long)T * Bp * m.H3);
    p.dgh = take((long)T * Bp * m.H3);
    p.dyl = take((long)T * Bp * m.Cop);
    p.dytot = take((long)T * Bp * m.Cop);
    p.dyfb = take((long)Bp * m.Cop);
    p.dh = take((long)Bp * m.H);
    p.dc1p = take((long)(T + 2 * (m.R - m.ks)) * Bp * t.C9p);
    p.dc0p = take((long)(t.F0 + 2 * (m.ks - 1)) * Bp * t.C3p);
    p.dxn = take((long)t.Tp * Bp * t.Cq);
    const long w1 = (long)t.C9 * t.K1, w0 = (long)t.C3 * t.K0;
    p.tmpw = take(w1 > w0 ? w1 : w0);
    p.bflags = take((long)(Bp / 16) * (m.H / 8) + 64);    // flags + status word of k_train_bwd_steps (inside the zeroed area)
    p.bcnt = take(GEMM_CNT);     // arrival counters of the backward pass's split GEMMs / column sums (inside the zeroed area) ...
    p.bcnt2 = take(GEMM_CNT);    // ... and of those that run on the side stream
    p.total = o;
    return p;
}

// Tile shape and contraction split for an LDS-tiled GEMM with an n_rows x n_cols output and `depth` contraction rows.
// Cost model fitted to a sweep of all tiles x splits over the training step's shapes on MI355X (tools/gemm_sweep.sh,
// profiles/r02_notes_training.md): a workgroup alone on a CU runs its MFMA stream at ~0.75 of what four co-resident ones reach
// together (global-load issue, LDS stores and the stage barrier are only hidden by OTHER workgroups' MFMAs), so the best choice
// has 2-4 workgroups per CU, whole rounds over the 256 CUs and little padding; small tiles pay more LDS traffic per flop.
// ks > 1 only when the caller can take partial tiles (part_cap floats).
static void pick_tile(int n_rows, int n_cols, long depth, long part_cap, int& TM, int& TN, int& ks, int cap = 0, bool nt = false, bool main_stream = false) {
    static const int cand[][2] = {{4, 4}, {3, 4}, {2, 4}, {3, 2}, {2, 2}, {1, 2}, {1, 1}};
    static const double tile_rate[] = {1.0, 1.0, 0.95, 0.93, 0.9, 0.7, 0.6};
    static const double conc_rate[] = {0.0, 0.75, 0.9, 0.97, 1.0, 1.0, 1.0, 1.0, 1.0};
    // workgroups a CU holds by registers (kernel resource usage of the build; <4,4>: k_gemm_tn2 three, k_gemm_nt2 four)
    static const int occ_cap[] = {3, 4, 5, 6, 8, 8, 8};
    // k_gemm_nt2 (the launch stream's GEMMs): constants fitted to a sweep of every (tile, split) over every shape of an encoder and a
    // decoder pass at 64 x 80 (tools/gemm_sweep.sh, round 5)
    static const double tile_rate_nt[] = {1.0, 1.02, 0.61, 0.71, 0.87, 0.78, 0.68};
    static const double conc_rate_nt[] = {0.0, 0.59, 0.71, 0.76, 0.92, 1.0, 1.0, 1.0, 1.0};
    const bool fit = nt && main_stream;
    const double* trate = fit ? tile_rate_nt : tile_rate;
    const double* crate = fit ? conc_rate_nt : conc_rate;
    const double comb = fit ? 0.38 : 0.3, launch = fit ? 6.8e5 : 2.0e5;
    double best = 1e30;
    TM = TN = ks = 1;
    int ci = 0;
    for (const auto& c : cand) {
        if (cap > 0 && (c[0] > cap || c[1] > cap)) { ++ci; continue; }
        const long blocks = (long)nblk(n_rows, 32 * c[0]) * nblk(n_cols, 32 * c[1]);
        const long lds = 2L * 16 * (32 * c[0] + 32 * c[1] + 8) * 4;
        const long occ = ci == 0 && nt ? 4 : occ_cap[ci];
        const long kres = 150000 / lds < occ ? 150000 / lds : occ;
        for (long k = 1; k <= 16 && k <= opt(OPT_GEMM_MAX_SPLIT); k *= 2) {
            if (k > 1 && (part_cap <= 0 || k * n_rows * n_cols > part_cap || depth / k < opt(OPT_GEMM_MIN_DEPTH))) break;
            const long nb = blocks * k, nbpc = (nb + 255) / 256, conc = nbpc < kres ? nbpc : kres;
            const double stages = (double)nblk(nblk(depth, 16), k);
            const double tb = 1024.0 * c[0] * c[1] * 16.0 * stages;                 // MACs of one workgroup
            double cost = (double)((nbpc + conc - 1) / conc) * conc * tb / (trate[ci] * crate[conc]);
            if (k > 1) cost += comb * (double)(k + 1) * n_rows * n_cols;            // the in-launch combine of the slices
            cost += launch;                                                         // a launch
            if (cost < best) { best = cost; TM = c[0]; TN = c[1]; ks = (int)k; }
        }
        ++ci;
    }
    if (const long f = opt(OPT_GEMM_FORCE)) {   // measurement only: TM*10000 + TN*100 + ks for every GEMM
        const int a = (int)(f / 10000), b = (int)(f / 100 % 100), k = (int)(f % 100);
        if (a >= 1 && b >= 1) { TM = a; TN = b; ks = 1; }
        if (k > 1 && part_cap > 0 && (long)k * n_rows * n_cols <= part_cap) ks = k;
    }
}

static inline bool al4(long v) { return (v & 3) == 0; }
static inline bool al16p(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <int TM, int TN, class... Args>
static void launch_tn2(dim3 g, hipStream_t st, Args... args) {
    const size_t lds = GemmTileCfg<TM, TN>::lds_bytes;
    hipLaunchKernelGGL((k_gemm_tn2<TM, TN>), g, dim3(256), lds, st, args...);
}
template <int TM, int TN, class... Args>
static void launch_nt2(dim3 g, hipStream_t st, Args... args) {
    const size_t lds = GemmTileCfg<TM, TN>::lds_bytes;
    hipLaunchKernelGGL((k_gemm_nt2<TM, TN>), g, dim3(256), lds, st, args...);
}
#define CVAE_TILE_DISPATCH(LAUNCH, TM_, TN_, g_, ...)                               \
    do {                                                                           \
        if (TM_ == 4 && TN_ == 4) LAUNCH<4, 4>(g_, st, __VA_ARGS__);               \
        else if (TM_ == 3 && TN_ == 4) LAUNCH<3, 4>(g_, st, __VA_ARGS__);          \
        else if (TM_ == 2 && TN_ == 4) LAUNCH<2, 4>(g_, st, __VA_ARGS__);          \
        else if (TM_ == 3 && TN_ == 2) LAUNCH<3, 2>(g_, st, __VA_ARGS__);          \
        else if (TM_ == 2 && TN_ == 2) LAUNCH<2, 2>(g_, st, __VA_ARGS__);          \
        else if (TM_ == 1 && TN_ == 2) LAUNCH<1, 2>(g_, st, __VA_ARGS__);          \
        else LAUNCH<1, 1>(g_, st, __VA_ARGS__);                                    \
    } while (0)

// cvae_set_side_stream: the weight-gradient GEMMs of a backward pass (nothing in the same backward chain reads their results) go
// to a second stream, where they overlap the NEXT pass's reverse recurrence -- a latency-bound kernel with one wave per SIMD that
// leaves registers, LDS and most matrix-pipe slots of every CU free.  the context's side_done table remembers, per scratch buffer, the event after
// which its dgi / dgh / gpart2 may be overwritten again.
// The weight images (TV_*) each train image holds: a per-context registry keyed by the image address.  A pass that needs an image
// the caller left out (or an image this context did not prepare) is refused, never run on garbage.
static int image_variants(const void* image) {
    auto it = cx().train_var.find(image);
    if (it == cx().train_var.end()) return 0;       // (an image this context did not prepare holds none of them: refused with -4)
    it->second.second = ++cx().train_var_tick;
    return it->second.first;
}
static void image_variants_record(const void* image, int variants) {
    auto& tv = cx().train_var;
    if (tv.size() >= 64 && tv.find(image) == tv.end()) {       // bounded: the least recently used address goes
        auto old = tv.begin();
        for (auto it = tv.begin(); it != tv.end(); ++it)
            if (it->second.second < old->second.second) old = it;
        tv.erase(old);
    }
    tv[image] = std::make_pair(variants & TV_ALL, ++cx().train_var_tick);
}

static hipEvent_t side_event_for(const void* scratch) {
    int free_i = -1;
    for (int i = 0; i < 8; ++i) {
        if (cx().side_done[i].scratch == scratch) return cx().side_done[i].ev;
        if (!cx().side_done[i].scratch && free_i < 0) free_i = i;
    }
    if (free_i < 0) {               // more than 8 scratch buffers seen: recycle the oldest entry; a scratch that is no longer in the
        free_i = (int)(cx().side_evict++ % 8);   // table waits for cx().side_last (cvae_gru_rnn_backward), which is never earlier
    }
    if (!cx().side_done[free_i].ev) (void)hipEventCreateWithFlags(&cx().side_done[free_i].ev, hipEventDisableTiming);
    cx().side_done[free_i].scratch = scratch;
    return cx().side_done[free_i].ev;
}

// CYCLEVAE_GEMM_LOG=1 (measurement only): every GEMM is bracketed by HIP events and printed with its shape and rate
struct GemmLog {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipStream_t st;
    const char* what;
    int M, N, K, TM, TN, ks;
    bool on;
    GemmLog(hipStream_t st_, const char* what_, int M_, int N_, int K_) : st(st_), what(what_), M(M_), N(N_), K(K_), TM(0), TN(0), ks(1) {
        on = opt(OPT_GEMM_LOG) != 0;
        if (on) { (void)hipEventCreate(&e0); (void)hipEventCreate(&e1); (void)hipEventRecord(e0, st); }
    }
    ~GemmLog() {
        if (!on) return;
        (void)hipEventRecord(e1, st);
        (void)hipEventSynchronize(e1);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        fprintf(stderr, "GEMM %s rows=%d cols=%d depth=%d tile=%dx%d ks=%d  %.1f us  %.1f TFLOP/s\n", what, M, N, K, 32 * TM, 32 * TN, ks,
                1e3 * ms, 2.0 * M * N * K / (1e9 * ms));
        
    }
};

// scratch that lets a GEMM with a small output split its contraction over several workgroups: GEMM_PART_FLOATS of partial tiles and
// GEMM_CNT ZEROED arrival counters (the combining block of every tile leaves its counter at zero again)
struct SplitWs {
    float* part = nullptr;
    unsigned* cnt = nullptr;
};

// cvae_selftest_gemm: what a wrapper launched -- {1 LDS-tiled / two-stage kernel or 0 simple kernel, TM, TN, slices of the contraction}
static inline void gemm_ran(int tiled, int TM, int TN, int nz) {
    if (int32_t* r = cx().gemm_ran) { r[0] = tiled; r[1] = TM; r[2] = TN; r[3] = nz; }
}

// C[m*ldc + n] (+)= sum_k A[m*lda + seg(k)] * Bm[n*ldb + k] + bias[n], then the optional mask epilogue (EpiMask: [B][T][N], M = T*Bp).
// Operand contract: K and seglen multiples of 16; K a multiple of seglen, or K <= seglen (one segment).  A is read at
// m*lda + s*segstride + [0, min(seglen, K)) for every segment s (segstride may be negative), Bm at n*ldb + [0, K); C is touched at
// m*ldc + [0, N) only.  The LDS-tiled kernels need lda, ldb, segstride multiples of 4 and 16-byte aligned A, Bm; anything else (or
// train_old_gemm) runs k_gemm_nt_seg, where a mask is applied in place by k_mul_mask_tm, which rewrites the WHOLE [M][ldc] block
// (columns N .. ldc-1 become 0: C must be writable to M*ldc there).
void gemm_nt(hipStream_t st, const float* A, long lda, int seglen, long segstride, const float* Bm, long ldb, const float* bias,
             float* C, long ldc, int M, int N, int K, int accumulate, SplitWs ws = SplitWs(), EpiMask em = EpiMask{nullptr, 0, 0, 0}) {
    float* part = ws.part;
    GemmLog lg(st, "nt", M, N, K);
    TrainProf tprof(st, TPROF_GEMM, 2.0 * M * N * K);
    const bool old = opt(OPT_TRAIN_OLD_GEMM) != 0;
    if (!old && al4(lda) && al4(ldb) && al4(segstride) && al16p(A) && al16p(Bm)) {
        int TM, TN, ks;
        pick_tile(M, N, K, part ? GEMM_PART_FLOATS : 0, TM, TN, ks, st == cx().side && cx().side ? cx().side_cap : 0, true, !(st == cx().side && cx().side));
        lg.TM = TM; lg.TN = TN; lg.ks = ks;
        const long ntile = (long)nblk(N, 32 * TN) * nblk(M, 32 * TM);
        if (ks > 1 && (ntile > GEMM_CNT || (long)ks * ntile * 1024 * TM * TN > GEMM_PART_FLOATS)) ks = 1;   // (padded tiles must fit)
        const int kchunk = ks > 1 ? (int)up(nblk(K, ks), 16) : K;
        const int nz = ks > 1 ? nblk(K, kchunk) : 1;
        float* pp = nz > 1 ? part : nullptr;
        const dim3 g(nblk(N, 32 * TN), nblk(M, 32 * TM), nz);
        gemm_ran(1, TM, TN, nz);
        // split contraction: the partial tiles are combined inside the launch by the last block of each tile (cvae_split_combine)
        CVAE_TILE_DISPATCH(launch_nt2, TM, TN, g, A, lda, seglen, segstride, Bm, ldb, bias, C, ldc, M, N, K, accumulate, kchunk, pp, ws.cnt, em);
        return;
    }
    gemm_ran(0, 0, 0, 1);
    if (opt(OPT_GEMM_TRACE)) fprintf(stderr, "gemm_nt fallback M=%d N=%d K=%d lda=%ld ldb=%ld ss=%ld\n", M, N, K, lda, ldb, segstride);
    hipLaunchKernelGGL((k_gemm_nt_seg<4, 4, 2, 2>), dim3(nblk(N, 128), nblk(M, 128)), dim3(256), 0, st, A, lda, seglen,
                       segstride, Bm, ldb, bias, C, ldc, M, N, K, accumulate);
    if (em.mask)     // (this path has no fused epilogue: mask in place)
        hipLaunchKernelGGL((k_mul_mask_tm), dim3(nblk((long)M * ldc, 256)), dim3(256), 0, st, C, (const float*)C, em.mask, em.B, em.Bp,
                           em.T, N, (int)ldc);
}

// C[n1*ldc + n2] (+)= sum_m A[m*lda + n1] * Bm[m*ldb + seg(n2)]   (contraction over the M rows; weight gradients).
// `part`: null, or GEMM_PART_FLOATS of scratch that lets a small output split its contraction over several workgroups
// Operand contract: the LDS-tiled kernels (lda, ldb, seglen, segstride multiples of 4, 16-byte aligned A, Bm) load float4 guarded
// on their FIRST element: every row of A must be readable to up(N1, 4) columns, every row of Bm to the end of the float4 that
// holds the last column of each segment (all callers pad these rows: H3, C9p, Cop, tot).  k_gemm_tn reads exactly N1 / N2 columns.
void gemm_tn(hipStream_t st, const float* A, long lda, const float* Bm, long ldb, int seglen, long segstride, float* C, long ldc,
             int M, int N1, int N2, int accumulate, SplitWs ws = SplitWs()) {
    float* part = ws.part;
    GemmLog lg(st, "tn", N1, N2, M);
    TrainProf tprof(st, TPROF_WGRAD, 2.0 * N1 * N2 * M);
    const bool old = opt(OPT_TRAIN_OLD_GEMM) != 0;
    if (!old && al4(lda) && al4(ldb) && al4(seglen) && al4(segstride) && al16p(A) && al16p(Bm)) {
        int TM, TN, ks;
        pick_tile(N1, N2, M, part ? GEMM_PART_FLOATS : 0, TM, TN, ks, st == cx().side && cx().side ? cx().side_cap : 0);
        lg.TM = TM; lg.TN = TN; lg.ks = ks;
        const long ntile = (long)nblk(N2, 32 * TN) * nblk(N1, 32 * TM);
        if (ks > 1 && (ntile > GEMM_CNT || (long)ks * ntile * 1024 * TM * TN > GEMM_PART_FLOATS)) ks = 1;
        const int mchunk = ks > 1 ? (int)up(nblk(M, ks), 16) : M;
        const int nz = ks > 1 ? nblk(M, mchunk) : 1;
        float* pp = nz > 1 ? part : nullptr;
        const dim3 g(nblk(N2, 32 * TN), nblk(N1, 32 * TM), nz);
        gemm_ran(1, TM, TN, nz);
        CVAE_TILE_DISPATCH(launch_tn2, TM, TN, g, A, lda, Bm, ldb, seglen, segstride, C, ldc, M, N1, N2, accumulate, mchunk, pp, ws.cnt);
        return;
    }
    gemm_ran(0, 0, 0, 1);
    if (opt(OPT_GEMM_TRACE)) fprintf(stderr, "gemm_tn fallback M=%d N1=%d N2=%d lda=%ld ldb=%ld sl=%d ss=%ld\n", M, N1, N2, lda, ldb, seglen, segstride);
    hipLaunchKernelGGL((k_gemm_tn), dim3(nblk(N2, 64), nblk(N1, 64)), dim3(256), 0, st, A, lda, Bm, ldb, seglen, segstride, C,
                       ldc, M, N1, N2, accumulate);
}

// C[m*ldc + n] (+)= sum_k A[m*lda + k] * Bm[n*ldb + k].  Operand contract: K a multiple of 16 (the waves split 16-k chunks; a
// remainder would be dropped); A is read at m*lda + [0, K), Bm at n*ldb + [0, K) as float4 (lda, ldb multiples of 4 in every caller).
void gemm_ks(hipStream_t st, const float* A, long lda, const float* Bm, long ldb, float* C, long ldc, int M, int N, int K,
             int accumulate) {
    gemm_ran(1, 0, 0, 1);
    // 16 columns per block: these products have M = Bp rows only, so parallelism must come from N and the K split
    const size_t lds = (size_t)4 * 16 * (16 + 4) * sizeof(float);
    hipLaunchKernelGGL((k_gemm_ks<1>), dim3(nblk(N, 16), nblk(M, 16)), dim3(256), lds, st, A, lda, Bm, ldb, C, ldc, M, N, K,
                       accumulate);
}

// What the forward and the backward of one training pass share: dimensions, layouts, the plan, base pointers.  Both entry points
// open one (after their own argument checks) and hand it to the stages below, in order; DESIGN.md 4.2 has the stages as a table.
struct TrainPass {
    Dims m; TDims t;
    TPrep pl; TrainPlan pn; TTape tl; TScratch sl;       // the image's layout, the plan, the layouts of tape and scratch
    const cvae_net_desc* d;
    const float* P;      // the train image
    float* TP;           // the tape: written by the forward, only read by the backward (which casts its const away to open the pass)
    float* S;            // the scratch
    int B, T, Bp, M;     // M = T * Bp rows of the time-major buffers
    long mtot;           // (T + 1) * Bp: with the slot of the incoming state
    hipStream_t st;
    SplitWs fws, bws;    // gpart with the forward's arrival counters (cleared by the prologue) / the backward's (by its memset)
};

// p.m is filled (make_train_dims): the layouts and the plan, which must be the same in both directions (the backward never checked B, T)
void open_train_pass(TrainPass& p, const cvae_net_desc* d, const void* image, int B, int T, void* tape, void* scratch, void* stream) {
    p.d = d; p.B = B; p.T = T; p.st = (hipStream_t)stream;
    p.t = make_tdims(p.m, T);
    p.pl = tprep_layout(p.m, d->has_scale_in != 0, d->has_scale_out != 0);
    p.pn = plan_train_pass(p.m, B, T);
    p.tl = ttape_layout(p.m, B, T, p.pn.Bp); p.sl = tscratch_layout(p.m, T, p.pn.Bp);
    p.P = (const float*)image; p.TP = (float*)tape; p.S = (float*)scratch;
    p.Bp = p.tl.Bp; p.M = T * p.Bp; p.mtot = (long)(T + 1) * p.Bp;
    p.fws = SplitWs{p.S + p.sl.gpart, (unsigned*)(p.S + p.sl.fcnt)};
    p.bws = SplitWs{p.S + p.sl.gpart, (unsigned*)(p.S + p.sl.bcnt)};
}

// Dropout masks into the tape, which keeps them for the backward: supplied (parity tests inject the reference's) or drawn with Philox.
// With a side stream set, the mask of the recurrence's feedback operand (gmask, two thirds of the draws; first read by the mask-bit
// kernel behind the three front-end GEMMs) is drawn THERE, beside the prologue and those GEMMs: 25-40 us less on the critical path of
// every pass of 64 rows (the masks depend on nothing but the seed).  Returns 1 where the recurrence has to wait for mask_join, < 0: error.
int draw_train_masks(const TrainPass& p, const float* cmask, const float* gmask, uint64_t seed, float p_drop) {
    const int B = p.B, T = p.T;
    const long nc = (long)B * T * p.t.C9, ng = (long)T * B * p.m.H;      // values of conv_drop's mask / of the feedback operand's
    float *const cm = p.TP + p.tl.cmask, *const gm = p.TP + p.tl.gmask;
    const long mparts = cx().draw_parts > 1 && B % cx().draw_parts == 0 ? cx().draw_parts : 1;
    const long rows = cx().draw_rows > 0 ? cx().draw_rows : (long)B / mparts;
    // one k_mask_gen launch: n values of Philox stream `id`, `inner` of them per batch row
    auto draw = [&](hipStream_t s, float* dst, long n, uint64_t id, long inner) {
        hipLaunchKernelGGL((k_mask_gen), dim3(nblk(n, 256)), dim3(256), 0, s, dst, n, seed, id, p_drop, (long)B, inner, rows, cx().draw_row0, mparts);
    };
    if (!cmask && !gmask && cx().side && opt(OPT_MASKS_ON_SIDE) && ng >= (1L << 20)) {
        if (!cx().mask_fork) CVAE_HIP_OK(hipEventCreateWithFlags(&cx().mask_fork, hipEventDisableTiming));
        if (!cx().mask_join) CVAE_HIP_OK(hipEventCreateWithFlags(&cx().mask_join, hipEventDisableTiming));
        CVAE_HIP_OK(hipEventRecord(cx().mask_fork, p.st));                 // (behind the tape's memset)
        CVAE_HIP_OK(hipStreamWaitEvent(cx().side, cx().mask_fork, 0));
        draw(cx().side, gm, ng, 2, p.m.H);
        CVAE_HIP_OK(hipEventRecord(cx().mask_join, cx().side));
        draw(p.st, cm, nc, 1, (long)T * p.t.C9);
        return 1;
    }
    if (!cmask && !gmask) {
        hipLaunchKernelGGL((k_mask_gen2), dim3(nblk(nc + ng, 256)), dim3(256), 0, p.st, cm, nc, (long)T * p.t.C9, gm, ng, (long)p.m.H, seed, p_drop,
                           (long)B, rows, cx().draw_row0, mparts);
        return 0;
    }
    if (cmask) CVAE_HIP_OK(hipMemcpyAsync(cm, cmask, (size_t)nc * sizeof(float), hipMemcpyDeviceToDevice, p.st));
    else draw(p.st, cm, nc, 1, (long)T * p.t.C9);
    if (gmask) CVAE_HIP_OK(hipMemcpyAsync(gm, gmask, (size_t)ng * sizeof(float), hipMemcpyDeviceToDevice, p.st));
    else draw(p.st, gm, ng, 2, p.m.H);
    return 0;
}

// scale_in, the time-major padded input, slot 0 of the state buffers, y_in; it also clears the flags / status words of the
// recurrence and the arrival counters of this pass's split GEMMs
void run_train_prologue(const TrainPass& p, const float* x, const float* y_in, const float* h_in) {
    const Dims& m = p.m; const TTape& tl = p.tl; const TScratch& sl = p.sl;
    TrainProParams pp;
    pp.x = x; pp.y_in = y_in; pp.h_in = h_in; pp.bo = p.P + p.pl.bo;
    pp.sin_w = p.d->has_scale_in ? p.P + p.pl.sin_w : nullptr;
    pp.sin_b = p.d->has_scale_in ? p.P + p.pl.sin_b : nullptr;
    pp.B = p.B; pp.Bp = p.Bp; pp.T = p.T; pp.C = m.C; pp.Cq = p.t.Cq; pp.pad = m.pad; pp.Co = m.Co; pp.Cop = m.Cop; pp.H = m.H;
    pp.xnp = p.TP + tl.xnp; pp.hbuf = p.S + sl.hbuf; pp.obuf = p.S + sl.obuf; pp.hrow = p.TP + tl.hrow; pp.orow = p.TP + tl.orow;
    pp.ybuf = p.TP + tl.ybuf; pp.dy = p.S + sl.dy; pp.mtot = p.mtot;
    pp.nA = p.B * p.T; pp.nH = (int)nblk((long)p.Bp * m.H, 1024); pp.nY = (int)nblk((long)p.Bp * m.Cop, 64);
    pp.zero_ptr = p.S + sl.tflags; pp.zero_n = sl.fcnt + GEMM_CNT - sl.tflags;
    hipLaunchKernelGGL((k_train_prologue), dim3(pp.nA + pp.nH + pp.nY + nblk(pp.zero_n, 64)), dim3(64), m.C * sizeof(float), p.st, pp);
}

// conv0, conv1 with conv_drop in its epilogue (the K padding columns of xcm stay zero from the tape's memset), input-gate GEMM:
// time-major segmented-row GEMMs
void run_train_front_end(const TrainPass& p) {
    const Dims& m = p.m; const TDims& t = p.t; const TTape& tl = p.tl; const int Bp = p.Bp, T = p.T;
    gemm_nt(p.st, p.TP + tl.xnp, t.Cq, t.Cq, (long)Bp * t.Cq, p.P + p.pl.w0r, t.K0, p.P + p.pl.b0, p.TP + tl.c0, t.C3p, t.F0 * Bp, t.C3, t.K0, 0, p.fws);
    gemm_nt(p.st, p.TP + tl.c0, t.C3p, t.C3p, (long)m.ks * Bp * t.C3p, p.P + p.pl.w1r, t.K1, p.P + p.pl.b1, p.TP + tl.xcm, t.C9p, T * Bp, t.C9, t.K1, 0,
            p.fws, EpiMask{p.TP + tl.cmask, p.B, Bp, T});
    gemm_nt(p.st, p.TP + tl.xcm, t.C9p, t.C9p, 0, p.P + p.pl.wix, t.C9p, p.P + p.pl.cfold_t, p.S + p.sl.gi, m.H3, T * Bp, m.H3, t.C9p, 0, p.fws);
}

// flag words of the forward recurrences; their status word behind the flags (FWD_LL: the first word), or the sink; the phase
// counters of block 0 with the option train_prof
inline unsigned* fwd_flags(const TrainPass& p) { return (unsigned*)(p.S + p.sl.tflags); }
inline int* fwd_status(const TrainPass& p, bool ll = false) {
    return cx().status_sink ? cx().status_sink : (int*)(fwd_flags(p) + (ll ? 0 : (size_t)(p.Bp / 16) * (p.m.H / 8)));
}
inline long long* prof_words(const TrainPass& p) { return opt(OPT_TRAIN_PROF) ? (long long*)(p.S + p.sl.tprof) : nullptr; }

// at most three rows: fp32 FMAs, one word per unit and row exchanged (cvae_train_ll.h).  KERNEL ORDER: clang emits the instances in the
// order it resolves their names; <1>, <2> inside the inner conditional, the pointer assigned first below, keep the code object's order
hipError_t fwd_ll(const TrainPass& p) {
    const Dims& m = p.m;
    TrainFwdLLParams q;
    q.xbuf = p.S + p.sl.llx; q.nonce = (cx().ll_train_launch.fetch_add(1u) & 0xffffu) << 16; q.backoff = p.pn.fwd_backoff;
    q.wrec_t = p.P + p.pl.wrec_t; q.gi = p.S + p.sl.gi; q.bhn = p.P + p.pl.bhn; q.gmask = p.TP + p.tl.gmask; q.tape = p.TP + p.tl.gates;
    q.hrow = p.TP + p.tl.hrow; q.orow = p.TP + p.tl.orow; q.wyT = p.P + p.pl.wyT; q.dy = p.S + p.sl.dy; q.Co = m.Co; q.B = p.B; q.Bp = p.Bp;
    q.H = m.H; q.T = p.T; q.status = fwd_status(p, true); const size_t lds = (size_t)(2 * 64 * 49 + 4 * 48) * sizeof(float);
    return cvae_launch_coop(p.B <= 2 ? (p.B == 1 ? k_train_fwd_steps_ll<1> : k_train_fwd_steps_ll<2>) : k_train_fwd_steps_ll<3>, dim3(m.H / 4),
                            dim3(256), lds, p.st, q);
}

// the 16-row-tile exact forms (16- and 8-unit blocks): exchanged h in limb triples, the feedback mask as bits
TrainFwd3hParams fwd3h(const TrainPass& p, const float* w3) {
    const Dims& m = p.m; const int Bp = p.Bp, T = p.T;
    hipLaunchKernelGGL((k_train_x3h_slot0), dim3(nblk((long)Bp * m.H, 256)), dim3(256), 0, p.st, (const float*)(p.TP + p.tl.hrow),
                       p.S + p.sl.hx3, Bp, m.H);
    hipLaunchKernelGGL((k_train_x3h_maskbits), dim3(nblk((long)T * (Bp / 16) * 2048, 256)), dim3(256), 0, p.st,
                       (const float*)(p.TP + p.tl.gmask), (unsigned char*)(p.S + p.sl.ox3), T, p.B, Bp, m.H, m.H == 1024 ? 8 : 1);
    TrainFwd3hParams q;
    q.hx = p.S + p.sl.hx3; q.mbits = (const unsigned char*)(p.S + p.sl.ox3); q.w3 = w3; q.gi = p.S + p.sl.gi; q.bhn = p.P + p.pl.bhn;
    q.gmask = p.TP + p.tl.gmask; q.tape = p.TP + p.tl.gates; q.hrow = p.TP + p.tl.hrow; q.orow = p.TP + p.tl.orow; q.wyT = p.P + p.pl.wyT;
    q.dy = p.S + p.sl.dy; q.Co = m.Co; q.B = p.B; q.Bp = Bp; q.H = m.H; q.T = T; q.rts = p.pn.fwd_rts; q.flags = fwd_flags(p);
    q.status = fwd_status(p); q.backoff = p.pn.fwd_backoff; q.xmap = (int)(opt(OPT_TRAIN_XMAP) & 1); q.prof = prof_words(p);
    return q;
}

// exact operands, 16-unit blocks with the zero column tiles of [W_hh | F] dropped (cvae_train_w3.h)
hipError_t fwd_w3(const TrainPass& p) {
    const Dims& m = p.m; const TrainFwd3hParams q = fwd3h(p, p.P + p.pl.wfw3);
    const int nl1 = m.H == 1024 ? CVAE_FWDW_NL1 : (opt(OPT_BWD_W3_L1_H64) ? 2 : 0);
    const size_t lds = (size_t)(4 * 16 * 68) * sizeof(float) + 1280 + (size_t)4 * 6 * w3_gpw(m) * 512 + (size_t)4 * nl1 * 1024;
    void (*k)(TrainFwd3hParams) = k_train_fwd_steps_w3<8, 4, CVAE_FWDW_NL1>;      // (named first: KERNEL ORDER, see fwd_ll)
    if (m.H != 1024) k = nl1 == 2 ? k_train_fwd_steps_w3<1, 2, 2> : k_train_fwd_steps_w3<1, 2, 0>;
    return cvae_launch_coop(k, dim3((m.H / 16) * p.pn.fwd_rts), dim3(256), lds, p.st, q);
}

// exact operands as fp16 triples, 8-unit x 32-row-tile blocks (cvae_train_x3.h)
hipError_t fwd_x3(const TrainPass& p) {
    const Dims& m = p.m; const int Bp = p.Bp, T = p.T, kpw = x3_kpw(m);
    hipLaunchKernelGGL((k_train_x3_slot0), dim3(nblk((long)Bp * m.H, 256)), dim3(256), 0, p.st, (const float*)(p.TP + p.tl.hrow),
                       p.S + p.sl.hx3, p.mtot, Bp, m.H);
    hipLaunchKernelGGL((k_train_x3_maskbits), dim3(nblk((long)T * (Bp / 32) * 4096, 256)), dim3(256), 0, p.st,
                       (const float*)(p.TP + p.tl.gmask), (unsigned char*)(p.S + p.sl.ox3), T, p.B, Bp, m.H, kpw);
    TrainFwd3Params q;
    q.hx = p.S + p.sl.hx3; q.mbits = (const unsigned char*)(p.S + p.sl.ox3); q.mtot = p.mtot; q.w3 = p.P + p.pl.w3f; q.gi = p.S + p.sl.gi;
    q.bhn = p.P + p.pl.bhn; q.gmask = p.TP + p.tl.gmask; q.tape = p.TP + p.tl.gates; q.hrow = p.TP + p.tl.hrow; q.orow = p.TP + p.tl.orow;
    q.wyT = p.P + p.pl.wyT; q.dy = p.S + p.sl.dy; q.Co = m.Co; q.B = p.B; q.Bp = Bp; q.H = m.H; q.T = T; q.rts = p.pn.fwd_rts;
    q.flags = fwd_flags(p); q.status = fwd_status(p); q.xmap = (int)(opt(OPT_TRAIN_XMAP) & 1); q.prof = prof_words(p);
    const size_t lds = (size_t)(4 * 32 * 40 + 6 * 256) * sizeof(float) + 1280 + (size_t)4 * 2 * kpw * 1024;
    return cvae_launch_coop(m.H == 1024 ? k_train_fwd_steps_x3<16> : k_train_fwd_steps_x3<1>, dim3((m.H / 8) * p.pn.fwd_rts), dim3(256), lds,
                            p.st, q);
}

// the same with 16-row tiles
hipError_t fwd_x3h(const TrainPass& p) {
    const Dims& m = p.m; const TrainFwd3hParams q = fwd3h(p, p.P + p.pl.w3h);
    const size_t lds = (size_t)(4 * 16 * 36) * sizeof(float) + 640 + (size_t)(m.H == 1024 ? 4 : 2) * 4 * (m.H == 1024 ? 8 : 1) * 1024;
    return cvae_launch_coop(m.H == 1024 ? k_train_fwd_steps_x3h<8, 4> : k_train_fwd_steps_x3h<1, 2>, dim3((m.H / 8) * p.pn.fwd_rts), dim3(256),
                            lds, p.st, q);
}

// the matrix product on fp16 pairs (same form as the eval kernel) or on the fp32-input MFMA
hipError_t fwd_pair(const TrainPass& p, bool pair) {
    const Dims& m = p.m;
    TrainFwdParams q;
    q.hbuf = p.S + p.sl.hbuf; q.obuf = p.S + p.sl.obuf; q.mtot = p.mtot; q.hrow = p.TP + p.tl.hrow; q.orow = p.TP + p.tl.orow;
    q.wrec_t8 = pair ? p.P + p.pl.wrec_t8h : p.P + p.pl.wrec_t8; q.gi = p.S + p.sl.gi; q.bhn = p.P + p.pl.bhn; q.gmask = p.TP + p.tl.gmask;
    q.tape = p.TP + p.tl.gates; q.wyT = p.P + p.pl.wyT; q.dy = p.S + p.sl.dy; q.Co = m.Co; q.B = p.B; q.Bp = p.Bp; q.H = m.H; q.T = p.T;
    q.rts = p.pn.fwd_rts; q.flags = fwd_flags(p); q.status = fwd_status(p); q.prof = prof_words(p); q.backoff = p.pn.fwd_backoff;
    const size_t lds = (4 * 16 * 36 + 2 * 128) * sizeof(float);
    return cvae_launch_coop(pair ? (m.H == 1024 ? k_train_fwd_steps_h<16> : k_train_fwd_steps_h<1>)
                                 : (m.H == 1024 ? k_train_fwd_steps<32> : k_train_fwd_steps<2>),
                            dim3((m.H / 8) * p.pn.fwd_rts), dim3(256), lds, p.st, q);
}

// T per-step launches
void fwd_steps(const TrainPass& p) {
    const Dims& m = p.m;
    TrainStepParams sp;
    sp.hbuf = p.S + p.sl.hbuf; sp.obuf = p.S + p.sl.obuf; sp.mtot = p.mtot; sp.hrow = p.TP + p.tl.hrow; sp.orow = p.TP + p.tl.orow;
    sp.wrec_t = p.P + p.pl.wrec_t; sp.gi = p.S + p.sl.gi; sp.bhn = p.P + p.pl.bhn; sp.gmask = p.TP + p.tl.gmask; sp.tape = p.TP + p.tl.gates;
    sp.wyT = p.P + p.pl.wyT; sp.dy = p.S + p.sl.dy; sp.Co = m.Co; sp.B = p.B; sp.Bp = p.Bp; sp.H = m.H;
    for (int tt = 0; tt < p.T; ++tt) {
        sp.t = tt;
        if (p.pn.fwd_col_tiles == 1)
            hipLaunchKernelGGL((k_gru_step_train<1>), dim3(m.H / 4), dim3(256), 4 * 64 * 20 * sizeof(float), p.st, sp);
        else if (p.Bp >= 128)
            hipLaunchKernelGGL((k_gru_step_train<2, 8>), dim3(m.H / 8), dim3(256), 2 * 4 * 128 * 20 * sizeof(float), p.st, sp);
        else
            hipLaunchKernelGGL((k_gru_step_train<2>), dim3(m.H / 8), dim3(256), 2 * 4 * 64 * 20 * sizeof(float), p.st, sp);
    }
}

// The T dependent steps, in the form the plan chose (bracketed by HIP events with the option train_profile).  join: gmask was drawn
// on the side stream; the wait sits behind the front-end GEMMs and in front of the first launch that reads the mask.
int run_fwd_recurrence(const TrainPass& p, bool join) {
    if (join) CVAE_HIP_OK(hipStreamWaitEvent(p.st, cx().mask_join, 0));
    TrainProf tprof(p.st, TPROF_FWD, 0.0);
    const int iv = image_variants(p.P);
    if (p.pn.fwd_need & ~iv)
        return fail(-4, "the train image was prepared without the exact-operand kernels' weight images (cvae_net_prepare_train_v "
                        "variants %d) and this pass (B=%d, T=%d) needs them", iv, p.B, p.T);
    FwdForm form = p.pn.fwd;
    if ((form == FWD_PAIR && !(iv & TV_PAIR)) || (form == FWD_FP32 && !(iv & TV_FP32))) form = FWD_STEPS;   // (image without them)
    hipError_t e = hipSuccess;
    const char* what = nullptr;      // (the forms that return -3 when their launch is refused name themselves)
    switch (form) {
    case FWD_LL: e = fwd_ll(p); what = "small-batch forward training recurrence"; break;
    case FWD_W3: e = fwd_w3(p); what = "exact-operand forward training recurrence (16-unit blocks)"; break;
    case FWD_X3: e = fwd_x3(p); what = "exact-operand forward training recurrence"; break;
    case FWD_X3H: e = fwd_x3h(p); what = "exact-operand forward training recurrence (16-row tiles)"; break;
    case FWD_PAIR: case FWD_FP32:
        if (fwd_pair(p, form == FWD_PAIR) == hipSuccess) break;
        (void)hipGetLastError();     // (a grid that does not fit: the per-step launches)
        [[fallthrough]];
    case FWD_STEPS: fwd_steps(p); break;
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(-3, "%s failed to launch: %s", what, hipGetErrorString(e));
    }
    return 0;
}

// raw projection of the dropped states, then scale_out / clamp into [B][T][Co], the last projection and the last state
void run_train_projection(const TrainPass& p, int clamp_lat_dim, float* trj_out, float* y_last, float* h_last) {
    const Dims& m = p.m;
    gemm_nt(p.st, p.TP + p.tl.orow + (long)p.Bp * m.H, m.H, m.H, 0, p.P + p.pl.wo, m.H, p.P + p.pl.bo, p.TP + p.tl.ybuf + (long)p.Bp * m.Cop, m.Cop,
            p.T * p.Bp, m.Co, m.H, 0, p.fws);
    TrainEpiParams ep;
    ep.ybuf = p.TP + p.tl.ybuf; ep.hrow = p.TP + p.tl.hrow;
    ep.sout_w = p.d->has_scale_out ? p.P + p.pl.sout_w : nullptr;
    ep.sout_b = p.d->has_scale_out ? p.P + p.pl.sout_b : nullptr;
    ep.clamp_from = p.d->has_scale_out ? -1 : clamp_dim(clamp_lat_dim); ep.clamp_min = clamp_floor(clamp_lat_dim);
    ep.B = p.B; ep.Bp = p.Bp; ep.T = p.T; ep.Co = m.Co; ep.Cop = m.Cop; ep.H = m.H;
    ep.trj_out = trj_out; ep.y_last = y_last; ep.h_last = h_last;
    hipLaunchKernelGGL((k_train_epilogue), dim3(p.B * p.T), dim3(64), m.Co * sizeof(float), p.st, ep);
}

// side-stream GEMMs of an earlier backward may still read this scratch (dgi / dgh / gpart2): wait for the event recorded behind
// them; a scratch the table no longer knows (evicted) waits for everything the side stream has been given
int wait_for_side_scratch(const TrainPass& p) {
    if (!cx().side) return 0;
    bool known = false;
    for (int i = 0; i < 8; ++i)
        if (cx().side_done[i].scratch == p.S && cx().side_done[i].ev) {
            CVAE_HIP_OK(hipStreamWaitEvent(p.st, cx().side_done[i].ev, 0));
            known = true;
        }
    if (!known && cx().side_last) CVAE_HIP_OK(hipStreamWaitEvent(p.st, cx().side_last, 0));
    return 0;
}

// Everything from dyl on is backward scratch: zero it (padding frames of dc1p / dc0p, dh, dyfb, dead rows); the gate gradients dgi / dgh
// right in front of dyl as well, unless the reverse recurrence writes every row of them.  Then dyl from dout (scale_out^T or the clamp).
int run_bwd_dy(const TrainPass& p, const float* dout, int clamp_lat_dim) {
    const Dims& m = p.m;
    const long zero_from = p.pn.bwd_writes_gates ? p.sl.dyl : p.sl.dgi;
    CVAE_HIP_OK(hipMemsetAsync(p.S + zero_from, 0, (size_t)(p.sl.total - zero_from) * sizeof(float), p.st));
    // (the LDS form holds scale_out^T whole: beyond ~120 outputs it no longer fits 64 KB and the plain kernel takes over)
    if (p.d->has_scale_out && (size_t)(m.Co * m.Co + CVAE_BWD_DY_ROWS * m.Co) * sizeof(float) <= 64 * 1024)
        hipLaunchKernelGGL((k_bwd_dy_sout), dim3(nblk(p.M, CVAE_BWD_DY_ROWS)), dim3(256),
                           (size_t)(m.Co * m.Co + CVAE_BWD_DY_ROWS * m.Co) * sizeof(float), p.st, dout, (const float*)(p.P + p.pl.sout_w),
                           p.S + p.sl.dyl, p.B, p.Bp, p.T, m.Co, m.Cop);
    else
        hipLaunchKernelGGL((k_bwd_dy), dim3(nblk((long)p.M * m.Cop, 256)), dim3(256), 0, p.st, dout, (const float*)(p.TP + p.tl.ybuf),
                           p.d->has_scale_out ? (const float*)(p.P + p.pl.sout_w) : (const float*)nullptr,
                           p.d->has_scale_out ? -1 : clamp_dim(clamp_lat_dim), clamp_floor(clamp_lat_dim), p.S + p.sl.dyl, p.B, p.Bp, p.T, m.Co, m.Cop);
    return 0;
}

// at most three rows (cvae_train_ll.h): it writes the live rows of dgi / dgh only (instances named as in fwd_ll: KERNEL ORDER)
hipError_t bwd_ll(const TrainPass& p, int* status) {
    TrainBwdLLParams q;
    q.xbuf = p.S + p.sl.llx; q.nonce = (cx().ll_train_launch.fetch_add(1u) & 0xffffu) << 16; q.backoff = p.pn.bwd_backoff;
    q.wrec_t = p.P + p.pl.wrec_t; q.dovl = p.S + p.sl.dovl; q.tape = p.TP + p.tl.gates; q.hrow = p.TP + p.tl.hrow; q.gmask = p.TP + p.tl.gmask;
    q.dgi = p.S + p.sl.dgi; q.dgh = p.S + p.sl.dgh; q.B = p.B; q.Bp = p.Bp; q.H = p.m.H; q.T = p.T; q.status = status;
    const size_t lds = (size_t)(256 * 25 + 8 * 24) * sizeof(float);
    return cvae_launch_coop(p.B <= 2 ? (p.B == 1 ? k_train_bwd_steps_ll<1> : k_train_bwd_steps_ll<2>) : k_train_bwd_steps_ll<3>, dim3(p.m.H / 4),
                            dim3(256), lds, p.st, q);
}

// the row tiles of the pass in launches of pn.bwd_per_launch tiles (0: all in one)
hipError_t bwd_by_launch(const TrainPass& p, TrainBwdParams q, void (*k)(TrainBwdParams), dim3 g, size_t lds) {
    const int per = p.pn.bwd_per_launch, nt16 = p.Bp / 16;
    hipError_t e = hipSuccess;
    for (int lo = 0; lo < nt16 && e == hipSuccess; lo += per ? per : nt16) {
        q.tile_lo = lo;
        q.tile_n = per ? (nt16 - lo < per ? nt16 - lo : per) : 0;
        e = cvae_launch_coop(k, g, dim3(256), lds, p.st, q);
    }
    return e;
}

// exact operands, 16 units x 16-row tiles per block, zero rows dropped (cvae_train_w3.h)
hipError_t bwd_w3(const TrainPass& p, TrainBwdParams q) {
    const Dims& m = p.m; q.wbk = p.P + p.pl.wbw3;
    const int nl1 = m.H == 1024 ? CVAE_BWDW_NL1 : (opt(OPT_BWD_W3_L1_H64) ? 2 : 0);
    const size_t lds = (size_t)(4 * 16 * 36) * sizeof(float) + 5120 + (size_t)4 * 6 * w3_gpw(m) * 512 + (size_t)4 * nl1 * 1024;
    void (*k)(TrainBwdParams) = k_train_bwd_steps_w3<8, 4, CVAE_BWDW_NL1>;        // (named first: KERNEL ORDER, see fwd_ll)
    if (m.H != 1024) k = nl1 == 2 ? k_train_bwd_steps_w3<1, 2, 2> : k_train_bwd_steps_w3<1, 2, 0>;
    return bwd_by_launch(p, q, k, dim3((m.H / 16) * p.pn.bwd_rts), lds);
}

// exact operands as limb triples, 8-unit blocks (cvae_train_x3.h)
hipError_t bwd_x3(const TrainPass& p, TrainBwdParams q) {
    const Dims& m = p.m; q.wbk = p.P + p.pl.wbk3;
    const size_t lds = (size_t)(4 * 16 * 20) * sizeof(float) + 2560 + (size_t)4 * (m.H / 32) * 512;
    return bwd_by_launch(p, q, m.H == 1024 ? k_train_bwd_steps_x3<32> : k_train_bwd_steps_x3<2>, dim3((m.H / 8) * p.pn.bwd_rts), lds);
}

// fp16 pairs (cvae_train_bwd.h): the whole pass in one launch
hipError_t bwd_pair(const TrainPass& p, TrainBwdParams q) {
    q.wbk = p.P + p.pl.wbk;
    const size_t lds = (size_t)(4 * 16 * 20) * sizeof(float) + 2048;
    return cvae_launch_coop(p.m.H == 1024 ? k_train_bwd_steps<32> : k_train_bwd_steps<2>, dim3((p.m.H / 8) * p.pn.bwd_rts), dim3(256), lds, p.st, q);
}

// The persistent reverse recurrence.  dovl[t*Bp + b][k] = sum_c dyl[.][c] * out_1.w[c][k]: one GEMM for all steps; then the
// recurrence (one launch, or one per two tiles per block); d loss / d y_t = dyl_t + W_ih[:, C9:]^T dgi_{t+1} is formed with the
// weight gradients (WgradWork)
int run_bwd_recurrence(const TrainPass& p) {
    const Dims& m = p.m; const TScratch& sl = p.sl;
    gemm_nt(p.st, p.S + sl.dyl, m.Cop, m.Cop, 0, p.P + p.pl.woT, m.Cop, nullptr, p.S + sl.dovl, m.H, p.M, m.H, m.Cop, 0, p.bws);
    TrainBwdParams q;
    q.gx = p.S + sl.gx; q.flags = (unsigned*)(p.S + sl.bflags); q.tile_lo = 0; q.tile_n = 0;
    q.status = cx().status_sink ? cx().status_sink : (int*)(p.S + sl.bflags) + (p.Bp / 16) * (m.H / 8);
    q.dovl = p.S + sl.dovl; q.tape = p.TP + p.tl.gates; q.hrow = p.TP + p.tl.hrow; q.gmask = p.TP + p.tl.gmask; q.dgi = p.S + sl.dgi;
    q.dgh = p.S + sl.dgh; q.dhz = p.S + sl.dh; q.B = p.B; q.Bp = p.Bp; q.H = m.H; q.T = p.T; q.ovf = (float)opt(OPT_BWD_OVERFLOW_AT);
    q.prof = prof_words(p); q.rts = p.pn.bwd_rts; q.xmap = (int)((opt(OPT_TRAIN_XMAP) >> 1) & 1); q.backoff = p.pn.bwd_backoff;
    if (p.pn.bwd != BWD_LL) {
        const int need = p.pn.bwd == BWD_PAIR ? TV_PAIR : TV_EXACT, ivb = image_variants(p.P);
        if (!(ivb & need))
            return fail(-4, "the train image was prepared without the weight images of the persistent reverse recurrence "
                            "(cvae_net_prepare_train_v variants %d, needed %d; B=%d, T=%d)", ivb, need, p.B, p.T);
    }
    TrainProf tprof(p.st, TPROF_BWD, 0.0);
    hipError_t e = hipSuccess;
    switch (p.pn.bwd) {
    case BWD_LL: e = bwd_ll(p, q.status); break;
    case BWD_W3: e = bwd_w3(p, q); break;
    case BWD_X3: e = bwd_x3(p, q); break;
    default: e = bwd_pair(p, q); break;
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(-3, "persistent reverse recurrence failed to launch: %s", hipGetErrorString(e));
    }
    tprof.end();
    return 0;
}

// The reverse recurrence as 2T per-step launches on fp32 products
int run_bwd_steps(const TrainPass& p) {
    const Dims& m = p.m; const TScratch& sl = p.sl;
    const int Bp = p.Bp, nt16 = Bp / 16; const bool old_gemm = opt(OPT_TRAIN_OLD_GEMM) != 0;
    BwdStepParams bp;
    bp.dyl = p.S + sl.dyl; bp.dytot = p.S + sl.dytot; bp.dyfb = p.S + sl.dyfb; bp.wo = p.P + p.pl.wo; bp.dh = p.S + sl.dh;
    bp.tape = p.TP + p.tl.gates; bp.hrow = p.TP + p.tl.hrow; bp.gmask = p.TP + p.tl.gmask; bp.dgi = p.S + sl.dgi; bp.dgh = p.S + sl.dgh;
    bp.dgic = old_gemm ? nullptr : p.S + sl.dgic; bp.dghc = old_gemm ? nullptr : p.S + sl.dghc;
    bp.B = p.B; bp.Bp = Bp; bp.H = m.H; bp.Co = m.Co; bp.Cop = m.Cop; bp.part = nullptr; bp.nparts = 0;
    BwdGemmParams gq;
    gq.wbp = p.P + p.pl.wbp; gq.part = p.S + sl.bpart; gq.Bp = Bp; gq.H = m.H; gq.Co = m.Co; gq.Cop = m.Cop;
    const int NRTB = nt16 >= 4 ? 4 : (nt16 >= 2 ? 2 : 1);
    TrainProf tprof(p.st, TPROF_BWD, 0.0);
    for (int tt = p.T - 1; tt >= 0; --tt) {
        bp.t = tt;
        hipLaunchKernelGGL((k_gru_step_bwd), dim3(nblk(m.H, 256), Bp), dim3(256), m.Cop * sizeof(float), p.st, bp);
        if (tt > 0 && old_gemm) {
            // d loss / d h_{t-1} += W_hh^T dgh_t ;  d loss / d y_{t-1} = W_ih[:, C9:]^T dgi_t
            gemm_ks(p.st, p.S + sl.dgh + (long)tt * Bp * m.H3, m.H3, p.P + p.pl.whhT, m.H3, p.S + sl.dh, m.H, Bp, m.H, m.H3, 1);
            gemm_ks(p.st, p.S + sl.dgi + (long)tt * Bp * m.H3, m.H3, p.P + p.pl.wyT, m.H3, p.S + sl.dyfb, m.Cop, Bp, m.Co, m.H3, 0);
        } else if (tt > 0) {
            // both products as K-split partial sums in one launch; step tt-1 adds them up
            gq.dgh = p.S + sl.dghc;      // (the chunk-major copy k_gru_step_bwd just wrote)
            gq.dgi = p.S + sl.dgic;
            const int KSr = opt(OPT_BWD_KS) >= 1 && opt(OPT_BWD_KS) <= BWD_KS_MAX ? (int)opt(OPT_BWD_KS) : BWD_KS;
            // a block's BWD_NTN column tiles must lie on one side of the H boundary (it reads dgh OR dgi): any H / 16 with one tile
            if (m.nch % BWD_NTN)
                return fail(-1, "k_bwd_step_gemm with %d column tiles per block needs hidden / 16 to be a multiple of it, got hidden %d",
                            BWD_NTN, m.H);
            const dim3 g(nblk((m.H + m.Cop) / 16, BWD_NTN), KSr, nblk(nt16, NRTB));
            const size_t lds = (size_t)4 * BWD_NTN * NRTB * 16 * 20 * sizeof(float);
            if (NRTB == 4) hipLaunchKernelGGL((k_bwd_step_gemm<4, BWD_NTN>), g, dim3(256), lds, p.st, gq);
            else if (NRTB == 2) hipLaunchKernelGGL((k_bwd_step_gemm<2, BWD_NTN>), g, dim3(256), lds, p.st, gq);
            else hipLaunchKernelGGL((k_bwd_step_gemm<1, BWD_NTN>), g, dim3(256), lds, p.st, gq);
            bp.part = p.S + sl.bpart; bp.nparts = KSr;
        }
    }
    return 0;
}

// The weight-gradient work of one backward pass that nothing in the same backward reads (see cvae_set_side_stream): launched on
// the caller's stream, or on the side stream behind an event.
struct WgradWork {
    const TrainPass& p;
    cvae_net_grads g;
    int acc;
    // persistent reverse recurrence: d loss / d y_t = dyl_t + W_ih[:, C9:]^T dgi_{t+1} is formed here (one GEMM over all steps); only
    // the out_1 weight / bias gradients read it, so it belongs to the work that may run on the side stream
    const float* wyT;
    int cap;              // tile cap of the GEMMs when they run on the side stream (0: none)
};

// out[n] (+)= sum_m A[m*lda + n].  Operand contract: the two-stage kernel reads rows as float4 guarded on their first element, so
// every row must be readable to up(n, 4) columns (H3 / Cop / C9p / C3p in every caller); k_colsum reads exactly n.  The two-stage
// kernel writes `out` from the block that draws the last ticket, so it needs the work space: without one (no caller passes an
// empty SplitWs today) k_colsum runs.
static void colsum_launch(hipStream_t cs, SplitWs ws, const float* A, long lda, float* out, int rows, int n, int acc) {
    float* part = ws.part;
    if (!al4(lda) || !al16p(A) || opt(OPT_TRAIN_OLD_GEMM) || nblk(n, 64) > GEMM_CNT || !part || !ws.cnt) {
        gemm_ran(0, 0, 0, 1);
        hipLaunchKernelGGL((k_colsum), dim3(nblk(n, 16)), dim3(256), 16 * 17 * sizeof(float), cs, A, lda, out, rows, n, acc);
        return;
    }
    // two stages: row slices in parallel, then a fixed-order sum of the slices
    int rs = 1024 / nblk(n, 64);
    rs = rs > 64 ? 64 : (rs < 1 ? 1 : rs);
    const int mchunk = (int)up(nblk(rows, rs), 16), nz = nblk(rows, mchunk);
    gemm_ran(1, 0, 0, nz);
    // (the sum of the slices happens in the launch: the last block of each 64-column group adds them in slice order)
    hipLaunchKernelGGL((k_colsum_part), dim3(nblk(n, 64), nz), dim3(256), 16 * 17 * sizeof(f32x4), cs, A, lda, part, rows, n, mchunk,
                       ws.cnt, out, acc);
}

// parts: bit 0 = the light work (the dytot GEMM, dW_ih's feedback columns, dW_out, the three bias column sums), bit 1 = the two big
// contractions (dW_hh, dW_ih's input columns)
static void launch_wgrad(hipStream_t ws, SplitWs part, const WgradWork& w, int parts = 3) {
    const TrainPass& p = w.p; const Dims& m = p.m; const TScratch& sl = p.sl;
    if (parts & 2) {
        gemm_tn(ws, p.S + sl.dgh, m.H3, p.TP + p.tl.hrow, m.H, m.H, 0, w.g.w_hh, m.H, p.M, m.H3, m.H, w.acc, part);
        gemm_tn(ws, p.S + sl.dgi, m.H3, p.TP + p.tl.xcm, p.t.C9p, p.t.C9p, 0, w.g.w_ih, m.tot, p.M, m.H3, p.t.C9, w.acc, part);
    }
    if (!(parts & 1)) return;
    if (w.wyT) {
        (void)hipMemcpyAsync(p.S + sl.dytot, p.S + sl.dyl, (size_t)p.M * m.Cop * sizeof(float), hipMemcpyDeviceToDevice, ws);
        if (p.T > 1)
            gemm_nt(ws, p.S + sl.dgi + (long)p.Bp * m.H3, m.H3, m.H3, 0, w.wyT, m.H3, nullptr, p.S + sl.dytot, m.Cop, (p.T - 1) * p.Bp, m.Co, m.H3,
                    1, part);
    }
    gemm_tn(ws, p.S + sl.dgi, m.H3, p.TP + p.tl.ybuf, m.Cop, m.Cop, 0, w.g.w_ih + p.t.C9, m.tot, p.M, m.H3, m.Co, w.acc, part);
    gemm_tn(ws, p.S + sl.dytot, m.Cop, p.TP + p.tl.orow + (long)p.Bp * m.H, m.H, m.H, 0, w.g.out_w, m.H, p.M, m.Co, m.H, w.acc, part);
    colsum_launch(ws, part, p.S + sl.dgi, m.H3, w.g.b_ih, p.M, m.H3, w.acc);
    colsum_launch(ws, part, p.S + sl.dgh, m.H3, w.g.b_hh, p.M, m.H3, w.acc);
    colsum_launch(ws, part, p.S + sl.dytot, m.Cop, w.g.out_b, p.M, m.Co, w.acc);
}

// enqueue the work on the side stream, ordered after everything `st` has been given so far
static int launch_wgrad_side(hipStream_t st, const WgradWork& w, int parts = 3) {
    if (!cx().side_ready) CVAE_HIP_OK(hipEventCreateWithFlags(&cx().side_ready, hipEventDisableTiming));
    CVAE_HIP_OK(hipEventRecord(cx().side_ready, st));
    CVAE_HIP_OK(hipStreamWaitEvent(cx().side, cx().side_ready, 0));
    cx().side_cap = w.cap;
    launch_wgrad(cx().side, SplitWs{w.p.S + w.p.sl.gpart2, (unsigned*)(w.p.S + w.p.sl.bcnt2)}, w, parts);
    CVAE_HIP_OK(hipEventRecord(side_event_for(w.p.S), cx().side));
    if (!cx().side_last) CVAE_HIP_OK(hipEventCreateWithFlags(&cx().side_last, hipEventDisableTiming));
    CVAE_HIP_OK(hipEventRecord(cx().side_last, cx().side));
    return 0;
}

// Input side: W_ih[:, :C9]^T, conv_drop, conv1^T, conv0^T, scale_in^T: the chain that produces dx (the next backward pass of the
// caller's graph waits for it).  conv_drop's gradient in the epilogue; dc1's padding frames / columns stay zero from the scratch
// memset.  dc1 / dc0: the gradients at the outputs of conv1 / conv0, behind the padding frames of dc1p / dc0p.
inline float* bwd_dc1(const TrainPass& p) { return p.S + p.sl.dc1p + (long)(p.m.R - p.m.ks) * p.Bp * p.t.C9p; }
inline float* bwd_dc0(const TrainPass& p) { return p.S + p.sl.dc0p + (long)(p.m.ks - 1) * p.Bp * p.t.C3p; }
void run_input_chain(const TrainPass& p, float* dx) {
    const Dims& m = p.m; const TDims& t = p.t; const TScratch& sl = p.sl; const int Bp = p.Bp;
    gemm_nt(p.st, p.S + sl.dgi, m.H3, m.H3, 0, p.P + p.pl.wixT, m.H3, nullptr, bwd_dc1(p), t.C9p, p.M, t.C9, m.H3, 0, p.bws,
            EpiMask{p.TP + p.tl.cmask, p.B, Bp, p.T});
    gemm_nt(p.st, p.S + sl.dc1p + (long)m.ks * (m.ks - 1) * Bp * t.C9p, t.C9p, t.C9p, -(long)m.ks * Bp * t.C9p, p.P + p.pl.w1t,
            (long)m.ks * t.C9p, nullptr, bwd_dc0(p), t.C3p, t.F0 * Bp, t.C3, m.ks * t.C9p, 0, p.bws);
    if (!dx) return;
    gemm_nt(p.st, p.S + sl.dc0p + (long)(m.ks - 1) * Bp * t.C3p, t.C3p, t.C3p, -(long)Bp * t.C3p, p.P + p.pl.w0t, (long)m.ks * t.C3p,
            nullptr, p.S + sl.dxn, t.Cq, t.Tp * Bp, t.Cq, m.ks * t.C3p, 0, p.bws);
    // (scale_in^T is folded into w0t at prepare time: this launch only gathers time-major -> [B][T][C])
    hipLaunchKernelGGL((k_scale_in_bwd), dim3(nblk((long)p.B * p.T * m.C, 256)), dim3(256), 0, p.st, (const float*)(p.S + sl.dxn),
                       (const float*)nullptr, dx, p.B, Bp, p.T, m.C, t.Cq, m.pad);
}

// The two convolution weight gradients and their bias sums feed nothing in this backward: with a side stream (overlap) they run
// there, behind an event recorded after the input chain
int run_conv_wgrad(const TrainPass& p, const cvae_net_grads* g, int acc, bool overlap) {
    const Dims& m = p.m; const TDims& t = p.t;
    float *const dc1 = bwd_dc1(p), *const dc0 = bwd_dc0(p), *const tmpw = p.S + p.sl.tmpw;
    hipStream_t cs = p.st; SplitWs part = p.bws;
    if (overlap) {
        CVAE_HIP_OK(hipEventRecord(cx().side_ready, p.st));
        CVAE_HIP_OK(hipStreamWaitEvent(cx().side, cx().side_ready, 0));
        cs = cx().side;
        part = SplitWs{p.S + p.sl.gpart2, (unsigned*)(p.S + p.sl.bcnt2)};
    }
    gemm_tn(cs, dc1, t.C9p, p.TP + p.tl.c0, t.C3p, t.C3p, (long)m.ks * p.Bp * t.C3p, tmpw, t.K1, p.M, t.C9, t.K1, 0, part);
    hipLaunchKernelGGL((k_unpack_dw), dim3(nblk((long)t.C9 * t.C3 * m.ks, 256)), dim3(256), 0, cs, (const float*)tmpw, (long)t.K1, t.C3p,
                       g->conv1_w, t.C9, t.C3, m.ks, acc);
    colsum_launch(cs, part, dc1, t.C9p, g->conv1_b, p.M, t.C9, acc);
    gemm_tn(cs, dc0, t.C3p, p.TP + p.tl.xnp, t.Cq, t.Cq, (long)p.Bp * t.Cq, tmpw, t.K0, t.F0 * p.Bp, t.C3, t.K0, 0, part);
    hipLaunchKernelGGL((k_unpack_dw), dim3(nblk((long)t.C3 * m.C * m.ks, 256)), dim3(256), 0, cs, (const float*)tmpw, (long)t.K0, t.Cq,
                       g->conv0_w, t.C3, m.C, m.ks, acc);
    colsum_launch(cs, part, dc0, t.C3p, g->conv0_b, t.F0 * p.Bp, t.C3, acc);
    if (overlap) {
        CVAE_HIP_OK(hipEventRecord(side_event_for(p.S), cx().side));     // (re-recorded: now also behind this work)
        CVAE_HIP_OK(hipEventRecord(cx().side_last, cx().side));
    }
    return 0;
}

}  // namespace

extern "C" {

size_t cvae_train_image_bytes(cvae_ctx* ctx, const cvae_net_desc* d) {
    CVAE_ENTER_SZ(ctx);
    Dims m;
    if (make_train_dims(d, &m)) return 0;
    return (size_t)tprep_layout(m, d->has_scale_in != 0, d->has_scale_out != 0).total * sizeof(float);
}

int cvae_net_prepare_train(cvae_ctx* ctx, const cvae_net_desc* d, const cvae_net_weights* w, void* image, size_t image_bytes, float gru_drop_p,
                           void* stream) {
    CVAE_ENTER(ctx);
    return cvae_net_prepare_train_v(ctx, d, w, image, image_bytes, gru_drop_p, TV_ALL, stream);
}

int cvae_train_variants_needed(cvae_ctx* ctx, const cvae_net_desc* d, int B, int T) {
    CVAE_ENTER(ctx);
    Dims m;
    if (make_train_dims(d, &m) || B < 1 || T < 1) return TV_ALL;
    return plan_train_pass(m, B, T).variants;
}

int cvae_plan_train_pass(cvae_ctx* ctx, const cvae_net_desc* d, int B, int T, int32_t out[12]) {
    CVAE_ENTER(ctx);
    Dims m;
    if (int rc = make_train_dims(d, &m)) return rc;
    if (B < 1 || T < 1 || !out) return fail(-1, "bad arguments: B=%d T=%d out=%p", B, T, (void*)out);
    const TrainPlan pn = plan_train_pass(m, B, T);
    out[0] = pn.Bp; out[1] = pn.fwd; out[2] = pn.fwd_rts; out[3] = pn.fwd_tiles; out[4] = pn.fwd_col_tiles; out[5] = pn.fwd_full_writes;
    out[6] = pn.bwd; out[7] = pn.bwd_rts; out[8] = pn.bwd_per_launch; out[9] = pn.bwd_tiles; out[10] = pn.bwd_writes_gates;
    out[11] = pn.variants;
    return 0;
}

int cvae_net_prepare_train_v(cvae_ctx* ctx, const cvae_net_desc* d, const cvae_net_weights* w, void* image, size_t image_bytes, float gru_drop_p,
                             int variants, void* stream) {
    CVAE_ENTER(ctx);
    Dims m;
    if (int rc = make_train_dims(d, &m)) return rc;
    if (!w || !image) return fail(-1, "null argument");
    if (image_bytes < cvae_train_image_bytes(ctx, d)) return fail(-2, "train image too small");
    if (!(gru_drop_p >= 0.0f && gru_drop_p < 1.0f)) return fail(-1, "dropout probability %f outside [0,1)", (double)gru_drop_p);
    hipStream_t st = (hipStream_t)stream;
    const TDims t = make_tdims(m, 1);
    const TPrep pl = tprep_layout(m, d->has_scale_in != 0, d->has_scale_out != 0);
    float* P = (float*)image;
    // zero what relies on it (K / channel padding of the GEMM-form weights); the MFMA-order images (wrec_t .. wrec_t8h, wbp, wbk, ffold,
    // w3f, w3h, wbk3: ~300 MB at hu1024) are written in full by their kernels
    CVAE_HIP_OK(hipMemsetAsync(P, 0, (size_t)pl.wrec_t * sizeof(float), st));
    CVAE_HIP_OK(hipMemsetAsync(P + pl.bhn, 0, (size_t)(pl.wbp - pl.bhn) * sizeof(float), st));
    CVAE_HIP_OK(hipMemsetAsync(P + pl.wo, 0, (size_t)(pl.ffold - pl.wo) * sizeof(float), st));
    auto conv = [&](const float* src, float* dst, int mode, long n) {
        hipLaunchKernelGGL((k_prep_conv_train), dim3(nblk(n, 256)), dim3(256), 0, st, src, dst, mode, m.C, m.ks, t.Cq, t.C3p, t.C9p);
    };
    conv(w->conv0_w, P + pl.w0r, 0, (long)t.C3 * t.K0);
    if (d->has_scale_in)      // conv0^T with scale_in^T folded in: the dx GEMM then produces d loss / d x itself
        hipLaunchKernelGGL((k_prep_w0t_sin), dim3(nblk((long)t.Cq * m.ks * t.C3p, 256)), dim3(256), 0, st, w->conv0_w, w->scale_in_w,
                           P + pl.w0t, m.C, m.ks, t.Cq, t.C3p);
    else
        conv(w->conv0_w, P + pl.w0t, 1, (long)t.Cq * m.ks * t.C3p);
    conv(w->conv1_w, P + pl.w1r, 2, (long)t.C9 * t.K1);
    conv(w->conv1_w, P + pl.w1t, 3, (long)t.C3 * m.ks * t.C9p);
    hipLaunchKernelGGL((k_prep_wix), dim3(nblk((long)m.H3 * t.C9p + m.H3, 256)), dim3(256), 0, st, w->w_ih, w->b_ih, w->b_hh,
                       w->out_b, P + pl.wix, P + pl.cfold_t, t.C9, t.C9p, m.Co, m.tot, m.H);
    hipLaunchKernelGGL((k_prep_ffold), dim3(nblk((long)m.H3 * (m.H / 4), 256)), dim3(256), 0, st, w->w_ih, w->out_w, P + pl.ffold, t.C9,
                       m.Co, m.tot, m.H);
    hipLaunchKernelGGL((k_prep_wrec_train), dim3(nblk((long)(m.H / 4) * 2 * m.nch * 256, 256)), dim3(256), 0, st,
                       (const float*)(P + pl.ffold), w->w_hh, P + pl.wrec_t, m.H);
    image_variants_record(image, variants);
    const bool v_exact = (variants & TV_EXACT) != 0, v_pair = (variants & TV_PAIR) != 0, v_fp32 = (variants & TV_FP32) != 0;
    if (v_pair || v_fp32)
        hipLaunchKernelGGL((k_prep_wrec_t8), dim3(nblk((long)(m.H / 8) * 2 * 2 * m.nch * 256, 256)), dim3(256), 0, st,
                           (const float*)(P + pl.wrec_t), P + pl.wrec_t8, m.H);
    if (m.H % 32 == 0 && v_pair)
        hipLaunchKernelGGL((k_prep_wrec_t8h), dim3(nblk((long)(m.H / 8) * 2 * m.nch * 512, 256)), dim3(256), 0, st,
                           (const float*)(P + pl.wrec_t8), P + pl.wrec_t8h, m.H);
    if (persist_ok(m) && v_exact)
        hipLaunchKernelGGL((k_prep_wrec_x3), dim3(nblk((long)(m.H / 8) * 4 * 2 * x3_kpw(m) * 512, 256)), dim3(256), 0, st,
                           (const float*)(P + pl.ffold), w->w_hh, P + pl.w3f, m.H, x3_kpw(m), 1.0f / (1.0f - gru_drop_p));
    if (persist_ok(m) && v_exact)
        hipLaunchKernelGGL((k_prep_wrec_x3h), dim3(nblk((long)(m.H / 8) * 2 * 2 * (m.H / 32) * 512, 256)), dim3(256), 0, st,
                           (const float*)(P + pl.ffold), w->w_hh, P + pl.w3h, m.H, 1.0f / (1.0f - gru_drop_p));
    auto copy2d = [&](float* dst, long dld, const float* src, long sld, int rows, int cols) {
        hipLaunchKernelGGL((k_copy2d), dim3(nblk((long)rows * cols, 256)), dim3(256), 0, st, dst, dld, src, sld, rows, cols);
    };
    auto copy2d_t = [&](float* dst, const float* src, long sld, int rows, int cols) {
        hipLaunchKernelGGL((k_copy2d_t), dim3(nblk((long)rows * cols, 256)), dim3(256), 0, st, dst, src, sld, rows, cols);
    };
    copy2d(P + pl.bhn, m.H, w->b_hh + 2 * m.H, m.H, 1, m.H);
    copy2d_t(P + pl.whhT, w->w_hh, (long)m.H, m.H3, m.H);            // whhT[k][n] = W_hh[n][k]
    copy2d_t(P + pl.wyT, w->w_ih + t.C9, (long)m.tot, m.H3, m.Co);   // wyT[c][n]  = W_ih[n][C9 + c]
    hipLaunchKernelGGL((k_prep_wbp), dim3(nblk((long)(m.H + m.Cop) * m.H3, 256)), dim3(256), 0, st, (const float*)(P + pl.whhT),
                       (const float*)(P + pl.wyT), P + pl.wbp, m.H, m.Co, m.Cop);
    copy2d(P + pl.wo, m.H, w->out_w, m.H, m.Co, m.H);
    copy2d_t(P + pl.woT, P + pl.wo, (long)m.H, m.Cop, m.H);          // woT[k][c] = out_1.w[c][k], ld Cop (columns >= Co are zero)
    if (persist_ok(m) && v_pair)
        hipLaunchKernelGGL((k_prep_wbk), dim3(nblk((long)(m.H / 8) * 4 * (m.H / 32) * 512, 256)), dim3(256), 0, st,
                           (const float*)(P + pl.ffold), w->w_hh, P + pl.wbk, m.H, m.H / 32);
    if (persist_ok(m) && v_exact)
        hipLaunchKernelGGL((k_prep_wbk3), dim3(nblk((long)(m.H / 8) * 4 * (m.H / 32) * 512, 256)), dim3(256), 0, st,
                           (const float*)(P + pl.ffold), w->w_hh, P + pl.wbk3, m.H, m.H / 32);
    if (persist_ok(m) && v_exact)
        hipLaunchKernelGGL((k_prep_wfw3), dim3(nblk((long)(m.H / 16) * 4 * w3_gpw(m) * 6 * 512, 256)), dim3(256), 0, st,
                           (const float*)(P + pl.ffold), w->w_hh, P + pl.wfw3, m.H, w3_gpw(m), 1.0f / (1.0f - gru_drop_p));
    if (persist_ok(m) && v_exact)
        hipLaunchKernelGGL((k_prep_wbw3), dim3(nblk((long)(m.H / 16) * 4 * w3_gpw(m) * 6 * 512, 256)), dim3(256), 0, st,
                           (const float*)(P + pl.ffold), w->w_hh, P + pl.wbw3, m.H, w3_gpw(m));
    copy2d(P + pl.bo, m.Co, w->out_b, m.Co, 1, m.Co);
    copy2d_t(P + pl.wixT, w->w_ih, (long)m.tot, m.H3, t.C9);         // wixT[c][n] = W_ih[n][c], rows >= C9 stay zero
    copy2d(P + pl.b0, t.C3, w->conv0_b, t.C3, 1, t.C3);
    copy2d(P + pl.b1, t.C9, w->conv1_b, t.C9, 1, t.C9);
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

size_t cvae_train_tape_bytes(cvae_ctx* ctx, const cvae_net_desc* d, int B, int T) {
    CVAE_ENTER_SZ(ctx);
    Dims m;
    if (make_train_dims(d, &m) || B < 1 || T < 1) return 0;
    return (size_t)ttape_layout(m, B, T, plan_train_pass(m, B, T).Bp).total * sizeof(float);
}

size_t cvae_train_scratch_bytes(cvae_ctx* ctx, const cvae_net_desc* d, int B, int T) {
    CVAE_ENTER_SZ(ctx);
    Dims m;
    if (make_train_dims(d, &m) || B < 1 || T < 1) return 0;
    return (size_t)tscratch_layout(m, T, plan_train_pass(m, B, T).Bp).total * sizeof(float);
}

int cvae_gru_rnn_forward_train(cvae_ctx* ctx, const cvae_net_desc* d, const void* image, const float* x, const float* y_in, const float* h_in,
                               int B, int T, int clamp_lat_dim, const float* cmask, const float* gmask, uint64_t seed,
                               float p_drop, float* trj_out, float* y_last, float* h_last, void* tape, size_t tape_bytes,
                               void* scratch, size_t scratch_bytes, void* stream) {
    CVAE_ENTER(ctx);
    TrainPass p;
    if (int rc = make_train_dims(d, &p.m)) return rc;
    if (B < 1 || T < 1) return fail(-1, "empty batch: B=%d T=%d", B, T);
    if (!image || !x || !y_in || !trj_out || !tape || !scratch) return fail(-1, "null argument");
    if (!(p_drop >= 0.0f && p_drop < 1.0f)) return fail(-1, "dropout probability %f outside [0,1)", (double)p_drop);
    open_train_pass(p, d, image, B, T, tape, scratch, stream);
    if (tape_bytes < (size_t)p.tl.total * sizeof(float)) return fail(-2, "tape too small");
    if (scratch_bytes < (size_t)p.sl.total * sizeof(float)) return fail(-2, "scratch too small");
    // zero: input padding frames / batch padding rows / K padding columns all rely on it.  The state copies and the gate tape (90 %
    // of the tape's 170 MB at B = 64) are written in full by the persistent recurrences and need no memset then.
    CVAE_HIP_OK(hipMemsetAsync(p.TP, 0, (size_t)(p.pn.fwd_full_writes ? p.tl.zero_end : p.tl.total) * sizeof(float), p.st));
    const int join = draw_train_masks(p, cmask, gmask, seed, p_drop);
    if (join < 0) return join;
    run_train_prologue(p, x, y_in, h_in);
    run_train_front_end(p);
    if (int rc = run_fwd_recurrence(p, join != 0)) return rc;
    run_train_projection(p, clamp_lat_dim, trj_out, y_last, h_last);
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

int cvae_set_side_stream(cvae_ctx* ctx, void* stream) {
    CVAE_ENTER(ctx);
    cx().side = (hipStream_t)stream;
    return 0;
}

int cvae_join_side_stream(cvae_ctx* ctx, void* stream) {
    CVAE_ENTER(ctx);
    if (!cx().side) return 0;
    if (!cx().side_join) CVAE_HIP_OK(hipEventCreateWithFlags(&cx().side_join, hipEventDisableTiming));
    CVAE_HIP_OK(hipEventRecord(cx().side_join, cx().side));
    CVAE_HIP_OK(hipStreamWaitEvent((hipStream_t)stream, cx().side_join, 0));
    return 0;
}

int cvae_gru_rnn_backward(cvae_ctx* ctx, const cvae_net_desc* d, const void* image, const float* dout, int B, int T, int clamp_lat_dim,
                          const void* tape, void* scratch, size_t scratch_bytes, float* dx, const cvae_net_grads* g,
                          int accumulate, void* stream) {
    CVAE_ENTER(ctx);
    TrainPass p;
    if (int rc = make_train_dims(d, &p.m)) return rc;
    if (!image || !dout || !tape || !scratch || !g) return fail(-1, "null argument");
    if (!g->conv0_w || !g->conv0_b || !g->conv1_w || !g->conv1_b || !g->w_ih || !g->w_hh || !g->b_ih || !g->b_hh || !g->out_w ||
        !g->out_b)
        return fail(-1, "missing gradient pointer");
    open_train_pass(p, d, image, B, T, const_cast<void*>(tape), scratch, stream);
    if (scratch_bytes < cvae_train_scratch_bytes(ctx, d, B, T)) return fail(-2, "scratch too small");      // (0 for B or T < 1, as ever)
    const int acc = accumulate ? 1 : 0;
    const bool overlap = cx().side != nullptr && accumulate != 0;    // (fresh gradient buffers are read by the caller right away)
    if (int rc = wait_for_side_scratch(p)) return rc;
    if (int rc = run_bwd_dy(p, dout, clamp_lat_dim)) return rc;
    if (int rc = p.pn.bwd != BWD_STEPS ? run_bwd_recurrence(p) : run_bwd_steps(p)) return rc;
    // ---- parameter gradients: contractions over all (t, b) rows.  The four recurrent / projection ones and their bias sums feed nothing
    // in this backward: with a side stream they run there, in 64 x 64 tiles beside the 8-unit blocks of a persistent reverse recurrence
    // (several fit on a CU beside one); the 16-unit blocks leave half the chip to the side stream, and beside per-step launches
    // (hu2048: 169 vs 176 ms) small tiles only cost
    const WgradWork w{p, *g, acc, p.pn.bwd != BWD_STEPS ? p.P + p.pl.wyT : nullptr, p.pn.bwd == BWD_X3 || p.pn.bwd == BWD_PAIR ? 2 : 0};
    // Where the side-stream work starts (round 5, same-run A/B on MI355X, B = 64: 24.9 ms all at once / 24.8 all behind the chain /
    // 24.5 split): from 64 rows on, the light part at once -- it barely disturbs the data-gradient chain, which the NEXT backward pass
    // waits for --, the two big contractions behind the chain, where they run under the next pass's reverse recurrence (they fit
    // beside its blocks since CVAE_BWD_RING = 5; the recurrence slows by ~0.2 ms per pass, the chain gains ~0.3).  Passes of fewer
    // than 64 rows: everything at once (B = 8: 13.8 vs 13.9 ms, one utterance 5.33 vs 5.42).
    const bool big_behind_chain = overlap && p.Bp >= 64;
    if (overlap) {
        if (int rc = launch_wgrad_side(p.st, w, big_behind_chain ? 1 : 3)) return rc;
    } else {
        launch_wgrad(p.st, p.bws, w);
    }
    run_input_chain(p, dx);
    if (big_behind_chain)
        if (int rc = launch_wgrad_side(p.st, w, 2)) return rc;
    if (int rc = run_conv_wgrad(p, g, acc, overlap)) return rc;
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

int cvae_status_latch(cvae_ctx* ctx, int32_t* latch, void* stream) {
    CVAE_ENTER(ctx);
    if (!latch) return fail(-1, "null argument");
    if (!cx().status_sink) return 0;      // (no sink set: the kernels report into their workspaces, nothing to move)
    hipLaunchKernelGGL((k_status_latch), dim3(1), dim3(64), 0, (hipStream_t)stream, (int*)latch, (volatile int*)cx().status_sink);
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

int cvae_train_debug_counters(cvae_ctx* ctx, const cvae_net_desc* d, int B, int T, const void* scratch, long long out[8], void* stream) {
    CVAE_ENTER(ctx);
    Dims m;
    if (int rc = make_train_dims(d, &m)) return rc;
    if (!scratch || !out) return fail(-1, "null argument");
    const TScratch sl = tscratch_layout(m, T, plan_train_pass(m, B, T).Bp);
    CVAE_HIP_OK(hipMemcpyAsync(out, (const float*)scratch + sl.tprof, 8 * sizeof(long long), hipMemcpyDeviceToHost, (hipStream_t)stream));
    CVAE_HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

int cvae_adam_step(cvae_ctx* ctx, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1,
                   float beta2, float eps, int step, const int32_t* gate, void* stream) {
    CVAE_ENTER(ctx);
    if (!param || !grad || !exp_avg || !exp_avg_sq || step < 1) return fail(-1, "bad argument");
    if (n == 0) return 0;
    const float bc1 = 1.0f - powf(beta1, (float)step), bc2s = sqrtf(1.0f - powf(beta2, (float)step));
    hipLaunchKernelGGL((k_adam), dim3(nblk((long)n, 256)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq,
                       (long)n, lr, beta1, beta2, eps, bc1, bc2s, (const int*)gate);
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

int cvae_adam_step_counted(cvae_ctx* ctx, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1,
                           float beta2, float eps, int32_t* state, const int32_t* gate, void* stream) {
    CVAE_ENTER(ctx);
    if (!param || !grad || !exp_avg || !exp_avg_sq || !state) return fail(-1, "bad argument");
    if (n == 0) return 0;
    hipLaunchKernelGGL((k_adam_tick), dim3(1), dim3(64), 0, (hipStream_t)stream, (int*)state, beta1, beta2, (const int*)gate);
    hipLaunchKernelGGL((k_adam_counted), dim3(nblk((long)n, 256)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq,
                       (long)n, lr, beta1, beta2, eps, (const int*)state, (const int*)gate);
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

// ---- cvae_selftest_gemm: one GEMM / column sum through the wrappers above, for the tests (include/cyclevae_hip.h holds the contracts)
size_t cvae_selftest_gemm_work_bytes(cvae_ctx* ctx) {
    CVAE_ENTER_SZ(ctx);
    return (size_t)(GEMM_PART_FLOATS + GEMM_CNT) * sizeof(float);
}

int cvae_selftest_gemm(cvae_ctx* ctx, const cvae_gemm_case* c, void* work, size_t work_bytes, int32_t ran[4], void* stream) {
    CVAE_ENTER(ctx);
    static_assert(GEMM_CNT == CVAE_SELFTEST_GEMM_CNT, "header and library disagree about the counters");
    if (!c || !ran) return fail(-1, "selftest_gemm: null argument");
    if (!c->A || !c->C || (c->kind != CVAE_GEMM_COLSUM && !c->B)) return fail(-1, "selftest_gemm: null operand");
    const long M = c->M, N = c->N, K = c->K, lda = c->lda, ldb = c->ldb, ldc = c->ldc, ss = c->segstride, sl = c->seglen;
    if (M < 1 || N < 1 || (c->kind != CVAE_GEMM_COLSUM && K < 1)) return fail(-1, "selftest_gemm: extents must be >= 1");
    if (lda < 0 || ldb < 0 || ldc < 0) return fail(-1, "selftest_gemm: negative leading dimension");
    if (c->use_split) {
        if (!work || work_bytes < (size_t)(GEMM_PART_FLOATS + GEMM_CNT) * sizeof(float) || !al16p(work))
            return fail(-1, "selftest_gemm: work space missing, smaller than cvae_selftest_gemm_work_bytes() or not 16-byte aligned");
    }
    const bool old = opt(OPT_TRAIN_OLD_GEMM) != 0;
    const bool al_ab = al4(lda) && al16p(c->A) && (c->kind == CVAE_GEMM_COLSUM || (al4(ldb) && al16p(c->B)));
    // the floats the kernels may touch around A, B, C under the contract, against what the caller owns
    long a_lo = 0, a_hi = 0, b_lo = 0, b_hi = 0, c_hi = 0;
    switch (c->kind) {
    case CVAE_GEMM_NT: {
        if (sl < 1 || K % 16 || sl % 16) return fail(-1, "selftest_gemm nt: K (%ld) and seglen (%ld) must be multiples of 16", K, sl);
        if (K > sl && K % sl) return fail(-1, "selftest_gemm nt: K (%ld) must be a multiple of seglen (%ld) or fit one segment", K, sl);
        if (ldc < N) return fail(-1, "selftest_gemm nt: ldc < N");
        const long nseg = K <= sl ? 1 : K / sl, len = K < sl ? K : sl;
        const bool tiled = !old && al_ab && al4(ss);
        a_lo = (nseg - 1) * ss < 0 ? (nseg - 1) * ss : 0;
        a_hi = (M - 1) * lda + ((nseg - 1) * ss > 0 ? (nseg - 1) * ss : 0) + len;
        b_hi = (N - 1) * ldb + K;
        c_hi = (M - 1) * ldc + N;
        if (c->mask) {
            if (c->mask_B < 1 || c->mask_Bp < c->mask_B || c->mask_T < 1 || (long)c->mask_T * c->mask_Bp != M)
                return fail(-1, "selftest_gemm nt: the mask covers [B][T][N] with B <= Bp and M = T*Bp");
            if (!tiled) c_hi = M * ldc;      // (k_mul_mask_tm rewrites whole rows)
        }
        break;
    }
    case CVAE_GEMM_TN: {
        if (sl < 1) return fail(-1, "selftest_gemm tn: seglen must be >= 1");
        if (c->bias || c->mask) return fail(-1, "selftest_gemm tn: takes neither bias nor mask");
        if (ldc < K) return fail(-1, "selftest_gemm tn: ldc < N2");
        const bool tiled = !old && al_ab && al4(sl) && al4(ss);
        const long nseg = (K + sl - 1) / sl, q = tiled ? 4 : 1;
        a_hi = (M - 1) * lda + up(N, q);
        long lo = 0, hi = 0;
        for (long s : {0L, nseg - 2, nseg - 1}) {       // (s*ss is linear over the full segments: the ends decide)
            if (s < 0) continue;
            const long cnt = K - s * sl < sl ? K - s * sl : sl;
            if (s * ss < lo) lo = s * ss;
            if (s * ss + up(cnt, q) > hi) hi = s * ss + up(cnt, q);
        }
        b_lo = lo;
        b_hi = (M - 1) * ldb + hi;
        c_hi = (N - 1) * ldc + K;
        break;
    }
    case CVAE_GEMM_KS:
        if (K % 16) return fail(-1, "selftest_gemm ks: K (%ld) must be a multiple of 16", K);
        if (c->bias || c->mask) return fail(-1, "selftest_gemm ks: takes neither bias nor mask");
        if (ldc < N) return fail(-1, "selftest_gemm ks: ldc < N");
        a_hi = (M - 1) * lda + K;
        b_hi = (N - 1) * ldb + K;
        c_hi = (M - 1) * ldc + N;
        break;
    case CVAE_GEMM_COLSUM: {
        if (c->bias || c->mask) return fail(-1, "selftest_gemm colsum: takes neither bias nor mask");
        const bool two = !old && al_ab && c->use_split && nblk(N, 64) <= GEMM_CNT;
        a_hi = (M - 1) * lda + (two ? up(N, 4) : N);
        c_hi = N;
        break;
    }
    default:
        return fail(-1, "selftest_gemm: unknown kind %d", (int)c->kind);
    }
    if (c->a_lo > a_lo || c->a_hi < a_hi)
        return fail(-1, "selftest_gemm: the kernels may touch A at [%ld, %ld), the caller owns [%lld, %lld)", a_lo, a_hi, (long long)c->a_lo, (long long)c->a_hi);
    if (c->kind != CVAE_GEMM_COLSUM && (c->b_lo > b_lo || c->b_hi < b_hi))
        return fail(-1, "selftest_gemm: the kernels may touch B at [%ld, %ld), the caller owns [%lld, %lld)", b_lo, b_hi, (long long)c->b_lo, (long long)c->b_hi);
    if (c->c_hi < c_hi) return fail(-1, "selftest_gemm: the kernels may touch C at [0, %ld), the caller owns %lld floats", c_hi, (long long)c->c_hi);
    SplitWs ws;
    if (c->use_split) { ws.part = (float*)work; ws.cnt = (unsigned*)((float*)work + GEMM_PART_FLOATS); }
    hipStream_t st = (hipStream_t)stream;
    ran[0] = ran[1] = ran[2] = ran[3] = -1;
    cx().gemm_ran = ran;
    switch (c->kind) {
    case CVAE_GEMM_NT:
        gemm_nt(st, c->A, lda, (int)sl, ss, c->B, ldb, c->bias, c->C, ldc, (int)M, (int)N, (int)K, c->accumulate, ws,
                EpiMask{c->mask, c->mask_B, c->mask_Bp, c->mask_T});
        break;
    case CVAE_GEMM_TN: gemm_tn(st, c->A, lda, c->B, ldb, (int)sl, ss, c->C, ldc, (int)M, (int)N, (int)K, c->accumulate, ws); break;
    case CVAE_GEMM_KS: gemm_ks(st, c->A, lda, c->B, ldb, c->C, ldc, (int)M, (int)N, (int)K, c->accumulate); break;
    default: colsum_launch(st, ws, c->A, lda, c->C, (int)M, (int)N, c->accumulate); break;
    }
    cx().gemm_ran = nullptr;
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

}  // extern "C"
