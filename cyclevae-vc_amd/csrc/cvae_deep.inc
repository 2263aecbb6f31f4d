// Host side of the eval passes of a GRU_RNN with n_layers >= 2 GRU layers (kernels: cvae_deep.h; ABI: the *_deep entry points).
// Included at the end of cvae_lib.hip.  Its own: the deep part of the prepared image, the workspace layout (one state buffer per
// layer), plan_deep_pass, k_deep_slot0 and the two recurrences (k_gru_steps_deep3 / k_gru_steps_deep).  Everything else of a pass is
// the stages of cvae_lib.hip (check_cells, run_prologue, run_front_end_gemm, run_projection, run_last_states), called as one cell on
// the top layer.
//
// Prepared image = [ the one-layer image of cvae_net_prepare built from layer 0 (front-end fold, cfold, out_1 / scale images:
// everything of it that does not involve W_hh is used as it is) | the deep part below ].  n_layers == 1 delegates every entry point
// to its one-layer counterpart.

namespace {

struct DeepPrep {     // offsets in floats behind the one-layer image, every block 64-float aligned
    long ffold, wrec, wrec_ls, w3, w3_ls, gbias, bhn, total;
};

inline bool deep3_ok(const Dims& m) { return m.H == 1024 || m.H == 64; }

DeepPrep deep_prep_layout(const Dims& m, int L) {
    DeepPrep p;
    long o = 0;
    auto take = [&](long n) { long r = o; o += up(n, 64); return r; };
    p.ffold = take((long)m.H3 * m.H);                       // F = W_ih_l0[:, 9C:] . out_1.w (k_prep_ffold, fp64-accumulated)
    p.wrec_ls = up(2L * (m.H / 4) * m.nch * 256, 64);       // k_prep_wrec_deep, per layer
    p.wrec = take(p.wrec_ls * L);
    p.w3_ls = deep3_ok(m) ? up((long)(m.H / 8) * 4 * 2 * (m.H / 64) * 3 * 256, 64) : 0;   // k_prep_wrec_x3, per layer
    p.w3 = deep3_ok(m) ? take(p.w3_ls * L) : -1;
    p.gbias = take((long)(L - 1) * m.H3);
    p.bhn = take((long)L * m.H);
    p.total = o;
    return p;
}

// Which recurrence a pass of a deep network takes (the one place that decides; cvae_plan_pass_deep reports it):
//   RESIDENT  k_gru_steps_deep3: H = 1024 or 64, every (layer, octet) block resident (L * H/8 <= CUs: L = 2 at H = 1024 on 256 CUs),
//             at most four 32-row tiles per block
//   GENERIC   k_gru_steps_deep as ONE launch: any H % 16 == 0, any L, H/4 blocks resident (H <= 1024 on 256 CUs)
//   PER_STEP  the same kernel, one launch per sub-step: what is left (H = 2048; callers without CVAE_FLAG_PERSISTENT)
// The four-tile cap.  A resident block (layer l, octet c, tile set ti of `rts` sets in flight) takes the row tiles ti, ti + rts, ..
// of every frame, and keeps the state it carries from frame to frame -- h_{l,t-1} of its thread's (row, unit), per tile -- in the
// four registers hk0 .. hk3 of k_gru_steps_deep3.  So a block can own at most four tiles: ceil(Bp/32 / rts) <= 4, and a pass with
// more rows than 4 * rts * 32 takes the any-H kernel.  `tiles` is that largest count (block ti = 0 has it); cvae_plan_pass_deep_tiles
// reports the whole plan.
enum { DEEP_PER_STEP = 0, DEEP_GENERIC = 1, DEEP_RESIDENT = 2 };
struct DeepPlan {
    int path, Bp, rts;
    int tiles;      // RESIDENT: most 32-row tiles one block owns; else the 16-row tiles a block of k_gru_steps_deep walks, four a trip
};

DeepPlan plan_deep_pass(const Dims& m, int L, int B, int T, int flags) {
    DeepPlan pn;
    pn.Bp = (int)up(B, 32);
    pn.rts = 1;
    pn.path = DEEP_PER_STEP;
    pn.tiles = pn.Bp / 16;
    const int cus = cu_count();
    if (!(flags & CVAE_FLAG_PERSISTENT)) return pn;
    const int nrt32 = pn.Bp / 32, NB = m.H / 8;
    const long mtot = (long)(T + 1) * pn.Bp;
    if (!(flags & CVAE_FLAG_GENERIC_STEP) && deep3_ok(m) && cus >= L * NB && (long)L * m.nch * mtot * 80 < (1L << 31)) {
        const int rts = row_tiles_per_block(cus, L * NB, nrt32);
        if ((nrt32 + rts - 1) / rts <= 4) {      // hk0 .. hk3 (above)
            pn.path = DEEP_RESIDENT;
            pn.rts = rts;
            pn.tiles = (nrt32 + rts - 1) / rts;
            return pn;
        }
    }
    if (cus <= 0 || m.H / 4 <= cus) pn.path = DEEP_GENERIC;
    return pn;
}

struct DeepWork {     // offsets in floats
    long status, xnp, gx, dy, y, hb, hb_ls, hx, hx_ls, flags, total;
    int Bp, Tp;
    long mtot;
};

DeepWork deep_work_layout(const Dims& m, int L, int B, int T) {
    DeepWork w;
    w.Bp = (int)up(B, 32);
    w.Tp = T + 2 * m.pad;
    w.mtot = (long)(T + 1) * w.Bp;
    long o = 0;
    auto take = [&](long n) { long r = o; o += up(n, 64); return r; };
    w.status = take(64);      // int32[4] status + barrier counter at word 8
    w.xnp = take((long)B * w.Tp * m.Cp + 64L * m.KFW + 64);
    w.gx = take((long)B * w.Tp * m.H3);
    w.dy = take((long)w.Bp * m.Co);
    w.y = take((long)T * w.Bp * m.Cop);
    w.hb_ls = up((long)m.nch * w.mtot * 16, 64);
    w.hb = take(w.hb_ls * L);
    w.hx_ls = deep3_ok(m) ? (long)m.nch * (w.mtot / 32) * 640 : 0;     // exactly nch * tiles * 2560 B: the kernel addresses layers by chunk index
    w.hx = deep3_ok(m) ? take(w.hx_ls * L) : -1;
    w.flags = take((long)L * (w.Bp / 32) * (m.H / 8));
    w.total = o;
    return w;
}

int deep_layers_ok(int L) {
    if (L < 1 || L > CVAE_DEEP_MAX_LAYERS) return fail(-1, "n_layers must be 1..%d, got %d", CVAE_DEEP_MAX_LAYERS, L);
    return 0;
}

int run_pass_deep(const Dims& m, const cvae_net_desc* d, int L, const float* P, const cvae_pass_input* in, const float* y_in,
                  const float* h_in, int B, int T, int clamp_lat_dim, float* trj_out, float* y_last, float* h_last, float* ws,
                  int flags, hipStream_t st) {
    const Prep pl = prep_layout(m, d->has_scale_in != 0, d->has_scale_out != 0);
    const float* PD = P + pl.total;
    const DeepPrep dl = deep_prep_layout(m, L);
    const DeepWork wl = deep_work_layout(m, L, B, T);
    // an image whose weights do not fit the limb images (cvae_net_prepared_in_range) runs k_gru_steps_deep, on fp32 operands
    if (image_known_unfit(P)) flags |= CVAE_FLAG_GENERIC_STEP;
    const DeepPlan pn = plan_deep_pass(m, L, B, T, flags);
    int* status = cx().status_sink ? cx().status_sink : (int*)ws;
    unsigned* bar = (unsigned*)(ws + wl.status) + 8;
    float* xnp = ws + wl.xnp;
    float* gx = ws + wl.gx;
    float* dy = ws + wl.dy;
    float* hb = ws + wl.hb;
    float* hb_top = hb + (long)(L - 1) * wl.hb_ls;
    float* hx = pn.path == DEEP_RESIDENT ? ws + wl.hx : nullptr;
    unsigned* hflags = (unsigned*)(ws + wl.flags);
    // the pass as ONE cell of the one-layer stages, on the TOP layer: the feedback is out_1 of that layer's state, so dy comes from
    // its h_in and the projection reads its buffer; h_last is per layer (below)
    Cell cell = {in, y_in, h_in ? h_in + (long)(L - 1) * B * m.H : nullptr, trj_out, y_last, nullptr};
    const PassRows rows = {&cell, 1, B, T, wl.Bp, wl.mtot};
    if (int rc = check_cells(m, rows)) return rc;
    RangeSlot range;      // where k_deep_slot0 reports a carried-in state the limb form cannot hold
    {
        ProTargets o = {};      // no limb / pair / gx0 output: layer 0's input side is an fp32 GEMM, of the exchanged values only the
        o.slot0 = hb_top;       // carried-in states take the limb form (k_deep_slot0, which fills slot 0 of every layer)
        o.zero_words = hflags; o.nzero = L * (wl.Bp / 32) * (m.H / 8);
        o.zero_status = (int*)ws;      // the pass's own status words; a status sink stays sticky (the caller clears it)
        o.zero_status_n = 8;
        o.ws_status = (int*)ws; o.limbs = pn.path == DEEP_RESIDENT; o.new_call = true;
        o.shape = in->lat && in->n_draws > 1 ? PRO_DRAWS : PRO_ROWS; o.xnp = xnp; o.dy = dy;
        run_prologue(m, d, P, pl, rows, o, st, &range);
    }
    hipLaunchKernelGGL((k_deep_slot0), dim3(nblk((long)L * wl.Bp * m.H, 256)), dim3(256), 0, st, h_in, hb, wl.hb_ls, hx, wl.hx_ls,
                       wl.mtot, L, B, wl.Bp, m.H, h_in && hx ? range.word : (int*)nullptr, range.val, range.at);
    run_front_end_gemm(m, P, pl, xnp, gx, B, wl.Tp, st);      // layer 0's input side for all frames
    const bool prof = (flags & CVAE_FLAG_PROFILE) != 0;
    if (pn.path == DEEP_RESIDENT) {
        DeepStep3Params q;
        q.hx = hx; q.hx_ls = wl.hx_ls; q.hb = hb; q.hb_ls = wl.hb_ls; q.mtot = wl.mtot; q.w3 = PD + dl.w3; q.w3_ls = dl.w3_ls;
        q.gx = gx; q.gx_bstride = (long)wl.Tp * m.H3; q.gbias = PD + dl.gbias; q.bhn = PD + dl.bhn; q.wyT = P + pl.wyT; q.dy = dy;
        q.Co = m.Co; q.B = B; q.Bp = wl.Bp; q.H = m.H; q.T = T; q.L = L; q.rts = pn.rts; q.flags = hflags; q.status = status;
        const int kpw = m.H / 64;
        const size_t lds = (size_t)(4 * 32 * 40 + 256) * sizeof(float) + 1280 + (size_t)4 * 2 * kpw * 1024;
        const dim3 g((unsigned)((m.H / 8) * L * pn.rts));
        const bool pr = prof && prof_begin(st, B, m.C);
        const hipError_t e = m.H == 1024 ? cvae_launch_coop(k_gru_steps_deep3<16>, g, dim3(256), lds, st, q)
                                         : cvae_launch_coop(k_gru_steps_deep3<1>, g, dim3(256), lds, st, q);
        if (pr) prof_end(st);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(-3, "resident recurrent kernel of a %d-layer network failed to launch: %s", L, hipGetErrorString(e));
        }
    } else {
        DeepStepParams sp;
        sp.hb = hb; sp.hb_ls = wl.hb_ls; sp.mtot = wl.mtot; sp.wrec = PD + dl.wrec; sp.w_ls = dl.wrec_ls; sp.gx = gx;
        sp.gx_bstride = (long)wl.Tp * m.H3; sp.gbias = PD + dl.gbias; sp.bhn = PD + dl.bhn; sp.B = B; sp.Bp = wl.Bp; sp.H = m.H;
        sp.T = T; sp.L = L; sp.s0 = 0; sp.bar = bar; sp.status = status; sp.nwg = (unsigned)(m.H / 4);
        sp.wyT = P + pl.wyT; sp.dy = dy; sp.Co = m.Co;
        const size_t step_lds = 4 * 64 * 20 * sizeof(float);
        bool launched = false;
        if (pn.path == DEEP_GENERIC) {
            CVAE_HIP_OK(hipMemsetAsync(bar, 0, 8 * sizeof(unsigned), st));
            const bool pr = prof && prof_begin(st, B, m.C);
            const hipError_t e = cvae_launch_coop(k_gru_steps_deep<true>, dim3(sp.nwg), dim3(256), step_lds, st, sp);
            if (e == hipSuccess) {
                launched = true;
                if (pr) prof_end(st);
            } else {
                (void)hipGetLastError();      // (not resident after all: the per-sub-step launches below; the open bracket is reused)
            }
        }
        if (!launched)
            for (int s = 0; s < L * T; ++s) {     // one profile bracket per launch: the launch count of a pass is what a caller reads
                sp.s0 = s;
                const bool pr = prof && prof_begin(st, B, m.C);
                hipLaunchKernelGGL((k_gru_steps_deep<false>), dim3(sp.nwg), dim3(256), step_lds, st, sp);
                if (pr) prof_end(st);
            }
    }
    run_projection(m, d, P, pl, rows, plain_projection(m, y_last != nullptr), hb_top, ws + wl.y, clamp_lat_dim, st);
    for (int l = 0; h_last && l < L; ++l) {
        cell.h_last = h_last + (long)l * B * m.H;
        run_last_states(m, rows, hb + (long)l * wl.hb_ls, st);
    }
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

size_t cvae_net_prepared_bytes_deep(cvae_ctx* ctx, const cvae_net_desc* d, int n_layers) {
    CVAE_ENTER_SZ(ctx);
    Dims m;
    if (make_dims(d, &m) || deep_layers_ok(n_layers)) return 0;
    const size_t base = (size_t)prep_layout(m, d->has_scale_in != 0, d->has_scale_out != 0).total * sizeof(float);
    return n_layers == 1 ? base : base + (size_t)deep_prep_layout(m, n_layers).total * sizeof(float);
}

size_t cvae_net_prepare_scratch_bytes_deep(cvae_ctx* ctx, const cvae_net_desc* d, int n_layers) {
    if (deep_layers_ok(n_layers)) return 0;
    return cvae_net_prepare_scratch_bytes(ctx, d);
}

int cvae_net_prepare_deep(cvae_ctx* ctx, const cvae_net_desc* d, int n_layers, const cvae_net_weights* w, const cvae_gru_layer* upper,
                          void* prepared, size_t prepared_bytes, void* scratch, size_t scratch_bytes, void* stream) {
    CVAE_ENTER(ctx);
    Dims m;
    if (int rc = make_dims(d, &m)) return rc;
    if (int rc = deep_layers_ok(n_layers)) return rc;
    if (n_layers == 1) return cvae_net_prepare(ctx, d, w, prepared, prepared_bytes, scratch, scratch_bytes, stream);
    if (!w || !upper || !prepared || !scratch) return fail(-1, "null argument");
    for (int l = 1; l < n_layers; ++l)
        if (!upper[l - 1].w_ih || !upper[l - 1].w_hh || !upper[l - 1].b_ih || !upper[l - 1].b_hh)
            return fail(-1, "missing weight pointer of GRU layer %d", l);
    if (prepared_bytes < cvae_net_prepared_bytes_deep(ctx, d, n_layers)) return fail(-2, "prepared buffer too small");
    if (int rc = cvae_net_prepare(ctx, d, w, prepared, prepared_bytes, scratch, scratch_bytes, stream)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Prep pl = prep_layout(m, d->has_scale_in != 0, d->has_scale_out != 0);
    const DeepPrep dl = deep_prep_layout(m, n_layers);
    float* P = (float*)prepared;
    float* PD = P + pl.total;
    CVAE_HIP_OK(hipMemsetAsync(PD, 0, (size_t)dl.total * sizeof(float), st));
    hipLaunchKernelGGL((k_prep_ffold), dim3(nblk((long)m.H3 * (m.H / 4), 256)), dim3(256), 0, st, w->w_ih, w->out_w, PD + dl.ffold, m.cw,
                       m.Co, m.tot, m.H);
    for (int l = 0; l < n_layers; ++l) {
        const float* U = l == 0 ? PD + dl.ffold : upper[l - 1].w_ih;
        const float* whh = l == 0 ? w->w_hh : upper[l - 1].w_hh;
        hipLaunchKernelGGL((k_prep_wrec_deep), dim3(nblk(2L * (m.H / 4) * m.nch * 256, 256)), dim3(256), 0, st, U, whh,
                           PD + dl.wrec + (long)l * dl.wrec_ls, m.H, (int*)(P + pl.range));
        if (deep3_ok(m))
            hipLaunchKernelGGL((k_prep_wrec_x3), dim3(nblk((long)(m.H / 8) * 4 * 2 * (m.H / 64) * 512, 256)), dim3(256), 0, st, U, whh,
                               PD + dl.w3 + (long)l * dl.w3_ls, m.H, m.H / 64, 1.0f);
        if (l == 0)
            hipLaunchKernelGGL((k_copy2d), dim3(nblk(m.H, 256)), dim3(256), 0, st, PD + dl.bhn, (long)m.H, w->b_hh + 2 * m.H, (long)m.H,
                               1, m.H);
        else
            hipLaunchKernelGGL((k_prep_deep_bias), dim3(nblk(m.H3, 128)), dim3(128), 0, st, upper[l - 1].b_ih, upper[l - 1].b_hh,
                               PD + dl.gbias + (long)(l - 1) * m.H3, PD + dl.bhn + (long)l * m.H, m.H);
    }
    CVAE_HIP_OK(hipGetLastError());
    return 0;
}

size_t cvae_pass_workspace_bytes_deep(cvae_ctx* ctx, const cvae_net_desc* d, int n_layers, int B, int T) {
    CVAE_ENTER_SZ(ctx);
    Dims m;
    if (make_dims(d, &m) || deep_layers_ok(n_layers) || B < 1 || T < 1) return 0;
    if (n_layers == 1) return (size_t)work_layout(m, B, T).total * sizeof(float);
    return (size_t)deep_work_layout(m, n_layers, B, T).total * sizeof(float);
}

int cvae_plan_pass_deep(cvae_ctx* ctx, const cvae_net_desc* d, int n_layers, int B, int T, int flags) {
    CVAE_ENTER(ctx);
    Dims m;
    if (int rc = make_dims(d, &m)) return rc;
    if (int rc = deep_layers_ok(n_layers)) return rc;
    if (n_layers < 2 || B < 1 || T < 1) return fail(-1, "bad sizes: n_layers=%d B=%d T=%d", n_layers, B, T);
    return plan_deep_pass(m, n_layers, B, T, flags).path;
}

int cvae_plan_pass_deep_tiles(cvae_ctx* ctx, const cvae_net_desc* d, int n_layers, int B, int T, int flags, int32_t out[4]) {
    CVAE_ENTER(ctx);
    Dims m;
    if (int rc = make_dims(d, &m)) return rc;
    if (int rc = deep_layers_ok(n_layers)) return rc;
    if (n_layers < 2 || B < 1 || T < 1 || !out) return fail(-1, "bad arguments: n_layers=%d B=%d T=%d out=%p", n_layers, B, T, (void*)out);
    const DeepPlan pn = plan_deep_pass(m, n_layers, B, T, flags);
    out[0] = pn.path; out[1] = pn.Bp; out[2] = pn.rts; out[3] = pn.tiles;
    return 0;
}

int cvae_gru_rnn_forward_deep(cvae_ctx* ctx, const cvae_net_desc* d, int n_layers, const void* prepared, const cvae_pass_input* in,
                              const float* y_in, const float* h_in, int B, int T, int clamp_lat_dim, float* trj_out, float* y_last,
                              float* h_last, void* workspace, size_t workspace_bytes, int flags, void* stream) {
    CVAE_ENTER(ctx);
    Dims m;
    if (int rc = make_dims(d, &m)) return rc;
    if (int rc = deep_layers_ok(n_layers)) return rc;
    if (n_layers == 1)
        return cvae_gru_rnn_forward(ctx, d, prepared, in, y_in, h_in, B, T, clamp_lat_dim, trj_out, y_last, h_last, workspace,
                                    workspace_bytes, flags, stream);
    if (B < 1 || T < 1) return fail(-1, "empty batch: B=%d T=%d", B, T);
    if (!prepared || !in || !y_in || !trj_out || !workspace) return fail(-1, "null argument");
    if (!in->seg0.ptr || (in->seg1.width > 0 && !in->lat && !in->seg1.ptr)) return fail(-1, "null input segment");
    if (workspace_bytes < cvae_pass_workspace_bytes_deep(ctx, d, n_layers, B, T)) return fail(-2, "workspace too small");
    return run_pass_deep(m, d, n_layers, (const float*)prepared, in, y_in, h_in, B, T, clamp_lat_dim, trj_out, y_last, h_last,
                         (float*)workspace, flags, (hipStream_t)stream);
}

}  // extern "C"
