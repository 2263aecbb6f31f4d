// Eval-mode recurrence of a GRU_RNN with L >= 2 GRU layers (reference gru_vae.py:282-320 builds nn.GRU(tot_in_dim, H, hidden_layers);
// :364-394 steps it frame by frame, feeding y_{t-1} = out_1(h_{L-1,t-1}) back into layer 0).
//
// With the load-time folds of the one-layer path kept (conv front-end -> layer 0's input matrix, feedback F = W_ih_l0[:, 9C:] . out_1.w
// applied to the TOP layer's previous state) every (frame t, layer l) sub-step is one GRU cell over a 2H-long operand [h_{l,t-1} ; u]:
//     u = h_{L-1,t-1} for layer 0,   u = h_{l-1,t} for layer l >= 1
// with the weights [W_hh_l | U_l], U_0 = F, U_l = W_ih_l.  r and z use all 2H; the n gate keeps two accumulators (n_h over the first
// half, n_in over the second).  The L*T sub-steps form ONE serial chain (y_{t-1} comes from the top layer: no layer wavefront).
//
// Two kernels:
//   k_gru_steps_deep3  exact fp32 operands as three fp16 limbs (six v_mfma_f32_32x32x16_f16 per product, the arithmetic of
//                      k_gru_steps_v6 / k_train_fwd_steps_x3), ONE launch per pass, every block resident: block = (layer, 8 hidden
//                      units) x 32-row tiles, its 2H-wide weights resident for the whole launch (first two limbs in registers, third
//                      limbs in LDS: the budget of k_train_fwd_steps_x3, whose operand shape [W_hh | F] this is, without masks and
//                      tape).  Hand-off per (layer, row tile, octet) flag behind write-through publishes of the limb triples.  The
//                      h_{l,t-1} half of a product does not depend on the sub-step in flight: it is multiplied BEFORE the block
//                      waits for u.  Built for H = 1024 and H = 64 (the size the host-fiber emulator runs).
//   k_gru_steps_deep   any H % 16 == 0, any L: the any-H kernel (k_gru_steps) over the L*T chain, exact fp32 products on
//                      v_mfma_f32_16x16x4_f32, weights streamed from L2 every sub-step, a grid barrier between sub-steps; as ONE
//                      persistent launch while H/4 blocks are resident, else one launch per sub-step.
// Both leave every layer's states as fp32 in the chunk-major layout of the one-layer path (hb[l]: [H/16][(T+1)*Bp][16]), so the
// projection, the epilogue and k_hlast of the one-layer path run unchanged on the top layer's buffer.
#pragma once
#include <cvae_intrin.h>

#include <type_traits>

#define CVAE_DEEP_MAX_LAYERS 8

// bias of the input-side pre-activations of a layer >= 1: b_ih + (r, z: b_hh); the n gate's b_hh stays with n_h (bhn)
__global__ void k_prep_deep_bias(const float* bih, const float* bhh, float* gbias, float* bhn, int H) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n < 3 * H) {
        gbias[n] = bih[n] + (n < 2 * H ? bhh[n] : 0.0f);
        if (n >= 2 * H) bhn[n - 2 * H] = bhh[n];
    }
}

// wrec[path][g][c][col][kk] of one layer for k_gru_steps_deep: col = a*4 + u, unit j = 4g + u, k = 16c + kk
//   path 0 (operand h_{l,t-1}): a = 0: W_hr, 1: W_hz, 2: 0,   3: W_hn        path 1 (operand u): a = 0: U_r, 1: U_z, 2: U_n, 3: 0
// These are the values the layer's limb image (k_prep_wrec_x3, shared with the training images) splits: one that image cannot
// carry is flagged here (unfit: cvae_flag_unfit).
__global__ void k_prep_wrec_deep(const float* U, const float* whh, float* wrec, int H, int* unfit) {
    const int nch = H >> 4;
    const long per = (long)(H >> 2) * nch * 256, idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < 2 * per) {
        const int path = idx >= per ? 1 : 0;
        const long r = idx - (long)path * per;
        const int kk = (int)(r & 15), col = (int)((r >> 4) & 15);
        const int c = (int)((r >> 8) % nch), g = (int)((r >> 8) / nch);
        const int a = col >> 2, u = col & 3, j = 4 * g + u, k = 16 * c + kk;
        float w = 0.0f;
        if (path == 0) {
            if (a != 2) w = whh[(long)((a == 3 ? 2 : a) * H + j) * H + k];
        } else if (a < 3) {
            w = U[(long)(a * H + j) * H + k];
        }
        wrec[idx] = w;
        cvae_flag_unfit(unfit, w);
    }
}

// slot 0 of every layer: fp32 (chunk-major) and, when hx is given, the limb triples k_gru_steps_deep3 exchanges
// (layout of k_train_x3_slot0: 2560 B per (16-unit chunk, 32-row tile)); h_in [L][B][H] or null (zeros); rows >= B are zero
// range_word: null, or the word set to range_val when a state of the limb form leaves its range (ProParams::range_word)
__global__ void k_deep_slot0(const float* h_in, float* hb, long hb_ls, float* hx, long hx_ls, long mtot, int L, int B, int Bp, int H,
                             int* range_word, int range_val, float range_at) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (idx < (long)L * Bp * H) {
        const int k = (int)(idx % H), r = (int)((idx / H) % Bp), l = (int)(idx / ((long)H * Bp));
        const float v = h_in && r < B ? h_in[((long)l * B + r) * H + k] : 0.0f;
        hb[(long)l * hb_ls + ((long)(k >> 4) * mtot + r) * 16 + (k & 15)] = v;
        if (hx) {
            unsigned short l0, l1;
            unsigned char l2;
            cvae_split3_f16b8(v, l0, l1, l2);
            bad = cvae_out_of_range(v, range_at);
            unsigned char* h8 = (unsigned char*)(hx + (long)l * hx_ls) + ((long)(k >> 4) * (mtot >> 5) + (r >> 5)) * 2560;
            const int kh = (k >> 3) & 1, rr = r & 31, e = k & 7;
            ((unsigned short*)(h8 + kh * 512 + rr * 16))[e] = l0;
            ((unsigned short*)(h8 + 1024 + kh * 512 + rr * 16))[e] = l1;
            h8[2048 + kh * 256 + rr * 8 + e] = l2;
        }
    }
    if (range_word && !cvae_block_all(!bad) && threadIdx.x == 0) *range_word = range_val;
}

struct DeepStepParams {
    float* hb;            // [L] x hb_ls floats: fp32 states, chunk-major [H/16][mtot][16]; slot s (rows s*Bp ..) = state going INTO frame s
    long hb_ls, mtot;
    const float* wrec;    // [L] x w_ls floats (k_prep_wrec_deep)
    long w_ls;
    const float* gx;      // layer 0: [B][Tp][3H] folded front-end pre-activations (with cfold)
    long gx_bstride;
    const float* gbias;   // [L-1][3H]: layers >= 1 (k_prep_deep_bias)
    const float* bhn;     // [L][H]
    int B, Bp, H, T, L;
    int s0;               // per-sub-step launches: the sub-step s = t*L + l of this launch
    unsigned* bar;        // grid-barrier counter, zeroed before a persistent launch
    int* status;
    unsigned nwg;
    const float* wyT;     // W_ih_l0[:, 9C:] transposed [Co][3H]
    const float* dy;      // [rows][Co] frame-0 feedback correction (k_prologue, from the TOP layer's h_in)
    int Co;
};

// Block g owns hidden units 4g..4g+3 of EVERY layer: one 16-column MFMA tile (r, z, n_in, n_h of four units) per path; its 4 waves
// split K = H of both paths and reduce through LDS.  PERSIST: all L*T sub-steps in one launch, a grid barrier between them.
template <bool PERSIST>
__global__ __launch_bounds__(256) void k_gru_steps_deep(DeepStepParams p) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, kq = lane >> 4;
    const int g = blockIdx.x, H = p.H, nch = H >> 4;
    const int c_lo = (nch * wave) >> 2, c_hi = (nch * (wave + 1)) >> 2;
    float* red = (float*)CVAE_SMEM;  // [4 waves][64 rows][20]
    const int nrt = p.Bp >> 4;
    const int s_begin = PERSIST ? 0 : p.s0, s_end = PERSIST ? p.T * p.L : p.s0 + 1;
    const int row = tid >> 2, u = tid & 3, j = 4 * g + u;
    const long hcol = (long)(g >> 2) * p.mtot * 16 + (g & 3) * 4 + u;  // this thread's unit inside a layer's buffer
    const long wpath = (long)(H >> 2) * nch * 256;
    for (int s = s_begin; s < s_end; ++s) {
        const int t = s / p.L, l = s - t * p.L;
        float* hl = p.hb + (long)l * p.hb_ls;
        const float* hprev = hl + (long)t * p.Bp * 16;
        float* hnext = hl + (long)(t + 1) * p.Bp * 16;
        const float* uop = l == 0 ? p.hb + (long)(p.L - 1) * p.hb_ls + (long)t * p.Bp * 16
                                  : p.hb + (long)(l - 1) * p.hb_ls + (long)(t + 1) * p.Bp * 16;
        const float* wg = p.wrec + (long)l * p.w_ls + (long)g * nch * 256 + lr * 16 + kq * 4;
        for (int rt0 = 0; rt0 < nrt; rt0 += 4) {
            f32x4 acc[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            for (int path = 0; path < 2; ++path) {
                const float* op = path ? uop : hprev;
                const float* wp = wg + (long)path * wpath;
                for (int c = c_lo; c < c_hi; ++c) {
                    const float4 b4 = *(const float4*)(wp + (long)c * 256);
                    const float* hc = op + (long)c * p.mtot * 16 + lr * 16 + kq * 4;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (rt0 + i < nrt) {
                            const float4 a4 = *(const float4*)(hc + (long)(rt0 + i) * 256);
                            acc[i] = cvae_mfma_16x16x4(a4.x, b4.x, acc[i]);
                            acc[i] = cvae_mfma_16x16x4(a4.y, b4.y, acc[i]);
                            acc[i] = cvae_mfma_16x16x4(a4.z, b4.z, acc[i]);
                            acc[i] = cvae_mfma_16x16x4(a4.w, b4.w, acc[i]);
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[(wave * 64 + i * 16 + kq * 4 + r) * 20 + lr] = acc[i][r];
            __syncthreads();
            const int grow = rt0 * 16 + row;
            if (grow < p.Bp) {
                float sg[4];
#pragma unroll
                for (int a = 0; a < 4; ++a)
                    sg[a] = red[(0 * 64 + row) * 20 + a * 4 + u] + red[(1 * 64 + row) * 20 + a * 4 + u] +
                            red[(2 * 64 + row) * 20 + a * 4 + u] + red[(3 * 64 + row) * 20 + a * 4 + u];
                float hn = 0.0f;
                if (grow < p.B) {
                    float g0, g1, g2;
                    if (l == 0) {
                        const float* gxp = p.gx + (long)grow * p.gx_bstride + (long)t * 3 * H;
                        g0 = gxp[j]; g1 = gxp[H + j]; g2 = gxp[2 * H + j];
                        if (t == 0 && p.dy) cvae_t0_fix(p.wyT, p.dy, p.Co, H, j, grow, g0, g1, g2);
                    } else {
                        const float* gb = p.gbias + (long)(l - 1) * 3 * H;
                        g0 = gb[j]; g1 = gb[H + j]; g2 = gb[2 * H + j];
                    }
                    const float r = cvae_sigmoid(g0 + sg[0]);
                    const float z = cvae_sigmoid(g1 + sg[1]);
                    const float n = tanhf(g2 + sg[2] + r * (sg[3] + p.bhn[(long)l * H + j]));
                    const float hold = hprev[hcol + (long)grow * 16];
                    hn = n + z * (hold - n);
                }
                hnext[hcol + (long)grow * 16] = hn;
            }
            __syncthreads();
        }
        if (PERSIST && s + 1 < s_end) cvae_grid_barrier(p.bar, (unsigned)(s + 1) * p.nwg, p.status);
    }
}

struct DeepStep3Params {
    float* hx;            // [L] x hx_ls floats: exchanged states as limb triples, tile-planar per layer:
    long hx_ls;           //   [H/16][mtot/32]{ l0 [kh][32 rows][8 halves] | l1 | l2 [kh][32][8 B] } (2560 B each)
    float* hb;            // [L] x hb_ls floats: the same states as fp32, chunk-major (projection, h_last)
    long hb_ls, mtot;
    const float* w3;      // [L] x w3_ls floats: [H/8][4 waves][2 paths][KPW][3 limbs][64 lanes][8 halves] (k_prep_wrec_x3, oscale 1)
    long w3_ls;
    const float* gx;      // layer 0: [B][Tp][3H]
    long gx_bstride;
    const float* gbias;   // [L-1][3H]
    const float* bhn;     // [L][H]
    const float* wyT;
    const float* dy;
    int Co, B, Bp, H, T, L, rts;
    unsigned* flags;      // [L][Bp/32][H/8], zeroed before launch: flags[l][i][c] = t + 1 <=> octet c of row tile i of h_{l,t} is published
    int* status;
};

template <int KPW>   // 16-k steps per wave and path = H/64
__global__ __launch_bounds__(256, 1) void k_gru_steps_deep3(DeepStep3Params p) {
    constexpr int RS = 40, NS = 2 * KPW;
    constexpr float S1 = 1.0f / 2048.0f;
    constexpr int RD = KPW < 8 ? KPW : 8;              // operand ring: 16-k steps in flight per wave
    const int tid = threadIdx.x, wave = cvae_uniform(tid >> 6), lane = tid & 63, lc = lane & 31, kh = lane >> 5;
    const int H = p.H, NB = H >> 3, nrt = p.Bp >> 5, rts = p.rts, L = p.L;
    const int blk = (int)blockIdx.x;
    const int c = blk % NB, l = (blk / NB) % L, ti = blk / (NB * L);
    const int s_lo = wave * KPW;
    float* red = (float*)CVAE_SMEM;                    // [4 waves][32 rows][RS]
    float* val = red + 4 * 32 * RS;                    // h_t of the task: [32 rows][8 units]
    unsigned short* hl = (unsigned short*)(val + 256); // publish image: l0, l1 [32 rows][8 halves], l2 [32 rows][8 bytes]
    float* w2l = (float*)(hl + 640);                   // third limbs of the weights: [4 waves][NS][64 lanes][8 halves]
    const int row = tid >> 3, u = tid & 7, j = 8 * c + u;
    const unsigned nchunk = (unsigned)(H >> 4), tstride = (unsigned)(p.mtot >> 5);
    const cvae_buf hxb = cvae_make_buf(p.hx, (unsigned)((long)L * p.hx_ls * 4));
    const unsigned lay_own = (unsigned)l * nchunk, lay_u = (unsigned)(l == 0 ? L - 1 : l - 1) * nchunk;
    const unsigned voff = (unsigned)kh * 512u + (unsigned)lc * 16u, voff2 = 2048u + (unsigned)kh * 256u + (unsigned)lc * 8u;
    f32x4 w0[NS], w1[NS];                              // [0, KPW): W_hh_l (operand h_{l,t-1}), [KPW, 2 KPW): U_l (operand u)
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const float* src = p.w3 + (long)l * p.w3_ls + (((((long)c * 4 + wave) * 2 + s / KPW) * KPW + s % KPW) * 3) * 256 + lane * 4;
        w0[s] = *(const f32x4*)src;
        w1[s] = *(const f32x4*)(src + 256);
        *(f32x4*)(w2l + (wave * NS + s) * 256 + lane * 4) = *(const f32x4*)(src + 512);
    }
    __syncthreads();
    const float* w2w = w2l + wave * NS * 256 + lane * 4;
    const float bhn = p.bhn[(long)l * H + j];
    float* hbl = p.hb + (long)l * p.hb_ls;
    unsigned* fl_own = p.flags + (long)l * nrt * NB;
    unsigned* fl_u = p.flags + (long)(l == 0 ? L - 1 : l - 1) * nrt * NB;
    const int ntile = ti < nrt ? (nrt - ti + rts - 1) / rts : 0, ntask = p.T * ntile;
    float hk0 = 0.f, hk1 = 0.f, hk2 = 0.f, hk3 = 0.f;  // h_{l,t-1} of this thread's (row, unit) per tile of the block (at most four)
    // input-side pre-activations: requested one task ahead (layer 0: the front-end GEMM's rows; above: constants)
    float ng0 = 0.f, ng1 = 0.f, ng2 = 0.f;
    if (l > 0) {
        const float* gb = p.gbias + (long)(l - 1) * 3 * H;
        ng0 = gb[j]; ng1 = gb[H + j]; ng2 = gb[2 * H + j];
    }
    auto prefetch_next = [&](int kn) {
        if (l > 0 || kn >= ntask) return;
        const int tn = kn / ntile, in_ = ti + (kn % ntile) * rts, grn = in_ * 32 + row;
        if (grn < p.B) {
            const float* gxp = p.gx + (long)grn * p.gx_bstride + (long)tn * 3 * H;
            ng0 = gxp[j]; ng1 = gxp[H + j]; ng2 = gxp[2 * H + j];
        }
    };
    // every octet (two per 16-unit chunk) of this wave's K share of layer `fl`, row tile i, carries at least `need`
    auto wait_flags = [&](const unsigned* fl, int i, unsigned need) {
        unsigned spins = 0;
        for (;;) {
            unsigned f = need;
            if (lane < 2 * KPW && 2 * s_lo + lane < NB) f = cvae_atomic_load_agent(fl + (long)i * NB + 2 * s_lo + lane);
            if (cvae_wave_all(f >= need)) break;
            cvae_sleep();
            if (++spins > (1u << 22)) {
                p.status[0] = 3;
                break;
            }
        }
        cvae_compiler_fence();
    };
    prefetch_next(0);
    for (int kk = 0; kk < ntask; ++kk) {
        const int t = kk / ntile, tl = kk % ntile, i = ti + tl * rts;
        const unsigned tile_own = (unsigned)((t * p.Bp + i * 32) >> 5);                       // slot t of this layer
        const unsigned tile_u = tile_own + (l == 0 ? 0u : (unsigned)(p.Bp >> 5));            // slot t (top layer) / slot t+1 (layer below)
        const int grow = i * 32 + row;
        const bool live = grow < p.B;
        float g0 = ng0, g1 = ng1, g2 = ng2;
        float hold = tl == 0 ? hk0 : (tl == 1 ? hk1 : (tl == 2 ? hk2 : hk3));
        if (live && t == 0) {
            if (l == 0 && p.dy) cvae_t0_fix(p.wyT, p.dy, p.Co, H, j, grow, g0, g1, g2);
            hold = hbl[((long)(c >> 1) * p.mtot + grow) * 16 + (c & 1) * 8 + u];
        }
        f32x16 a0 = cvae_zero16_t(), a1 = cvae_zero16_t(), a2 = cvae_zero16_t(), a3 = cvae_zero16_t();   // S0 | S1 | S2 (two chains)
        f32x4 hc[2 * RD];
        f32x2 hb2[RD];
        // one path of the product: KPW 16-k steps of this wave's K share, operands through a ring of RD steps
        auto run_path = [&](auto pc, unsigned lay, unsigned tile0) {
            constexpr int PATH = decltype(pc)::value;
            auto load_op = [&](int s) {
                const unsigned so = ((lay + (unsigned)(s_lo + s)) * tstride + tile0) * 2560u;
                hc[2 * (s % RD)] = cvae_buf_load_f4(hxb, voff, so);
                hc[2 * (s % RD) + 1] = cvae_buf_load_f4(hxb, voff, so + 1024u);
                hb2[s % RD] = cvae_buf_load_f2(hxb, voff2, so);
            };
#pragma unroll
            for (int s = 0; s < RD; ++s) load_op(s);
#pragma unroll
            for (int s = 0; s < KPW; ++s) {
                const f32x4 l0 = hc[2 * (s % RD)], l1 = hc[2 * (s % RD) + 1];
                const f32x4 l2 = cvae_bf8x8_to_h8(hb2[s % RD]);
                const f32x4 w2 = *(const f32x4*)(w2w + (PATH * KPW + s) * 256);
                a0 = cvae_mfma_32x32x16_f16(l0, w0[PATH * KPW + s], a0);
                a1 = cvae_mfma_32x32x16_f16(l0, w1[PATH * KPW + s], a1);
                a2 = cvae_mfma_32x32x16_f16(l1, w1[PATH * KPW + s], a2);
                a3 = cvae_mfma_32x32x16_f16(l0, w2, a3);
                a1 = cvae_mfma_32x32x16_f16(l1, w0[PATH * KPW + s], a1);
                a2 = cvae_mfma_32x32x16_f16(l2, w0[PATH * KPW + s], a2);
                cvae_sched_fence();
                if (s + RD < KPW) load_op(s + RD);
            }
        };
        // the h_{l,t-1} half first: it was published a whole sub-step round ago, so this product runs while the layer that
        // produces u is still working
        if (t > 0) wait_flags(fl_own, i, (unsigned)t);
        run_path(std::integral_constant<int, 0>(), lay_own, tile_own);
        if (l > 0) wait_flags(fl_u, i, (unsigned)(t + 1));
        else if (t > 0) wait_flags(fl_u, i, (unsigned)t);
        run_path(std::integral_constant<int, 1>(), lay_u, tile_u);
        prefetch_next(kk + 1);
        cvae_sched_fence();
#pragma unroll
        for (int q = 0; q < 16; ++q)
            red[(wave * 32 + (q & 3) + 8 * (q >> 2) + 4 * kh) * RS + lc] = a0[q] + (a1[q] + (a2[q] + a3[q]) * S1) * S1;
        __syncthreads();
        {
            float hn = 0.f;
            if (live) {
                float sg[4];
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    sg[g] = red[(0 * 32 + row) * RS + g * 8 + u] + red[(1 * 32 + row) * RS + g * 8 + u] +
                            red[(2 * 32 + row) * RS + g * 8 + u] + red[(3 * 32 + row) * RS + g * 8 + u];
                const float rg = cvae_sigmoid(g0 + sg[0]);
                const float zg = cvae_sigmoid(g1 + sg[1]);
                const float ng = tanhf(g2 + sg[2] + rg * (sg[3] + bhn));
                hn = ng + zg * (hold - ng);
            }
            if (tl == 0) hk0 = hn; else if (tl == 1) hk1 = hn; else if (tl == 2) hk2 = hn; else hk3 = hn;
            val[row * 8 + u] = hn;
            unsigned short l0, l1;          // the split happens once per value, by the thread that produced it
            unsigned char l2;
            cvae_split3_f16b8(hn, l0, l1, l2);
            hl[row * 8 + u] = l0;
            hl[256 + row * 8 + u] = l1;
            ((unsigned char*)(hl + 512))[row * 8 + u] = l2;
        }
        __syncthreads();
        if (tid < 64) {   // wave 0 publishes the image into slot t+1 of its layer (write-through), drains, raises the octet's flag
            const unsigned so = ((lay_own + (unsigned)(c >> 1)) * tstride + tile_own + (unsigned)(p.Bp >> 5)) * 2560u;
            cvae_buf_store_f4_sc1(hxb, (unsigned)(c & 1) * 512u + (unsigned)(tid & 31) * 16u, so + (unsigned)(tid >> 5) * 1024u,
                                  *(const f32x4*)(hl + tid * 8));
            if (tid < 32)
                cvae_buf_store_f2_sc1(hxb, 2048u + (unsigned)(c & 1) * 256u + (unsigned)tid * 8u, so, *(const f32x2*)(hl + 512 + tid * 4));
            cvae_drain_vmem();
            cvae_wave_barrier();
            if (tid == 0) cvae_atomic_store_agent(fl_own + (long)i * NB + c, (unsigned)(t + 1));
        } else if (tid < 128) {   // wave 1: the fp32 copy the projection and k_hlast read after this launch (plain 16-byte stores)
            const int r = (tid - 64) >> 1, half = tid & 1;
            const f32x4 v = *(const f32x4*)(val + r * 8 + half * 4);
            *(f32x4*)(hbl + ((long)(c >> 1) * p.mtot + (long)(t + 1) * p.Bp + i * 32 + r) * 16 + (c & 1) * 8 + half * 4) = v;
        }
    }
}
