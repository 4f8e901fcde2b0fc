// decode_ln_kernels.hip -- the greedy decode of layer_n models (LSTMCore with nn.LayerNorm on i2h(x), h2h(h) and c',
// src/captioning/nets.py:92-96,102-104,126-127), for every supported width E, R in {128, 256, 384, 512}
// (DESIGN.md "Layer-norm models").
// Not a translation unit of its own: decode_kernel.hip #includes this file behind decode_wide_kernels.hip, whose
// window helpers (wide_tile, wide_store_block / wide_load_block, st4, WD_WIN_BYTES) it uses.
//
// The structure is the wide kernel's: one workgroup = one member (both signs) x one slab of <= 128 rows, wave w = sign
// (w >> 2) x 32-row group (w & 3), every step in one launch, products as chains of 128-k windows through the two 32-row
// LDS stage buffers, h', c and x in lane-private global scratch. The image projection, the logit phase, the token rule
// and the early exit are the wide kernel's, line for line. The cell is what differs: a layer norm needs the whole row
// of 5R gate pre-activations before any of them can be used, so the cell runs in phases:
//   (a) the 5R / 32 gate tiles in ascending row order; the i2h chain (over x) and the h2h chain (over h_t) of a tile
//       are kept apart, stored to the lane's ai / ah windows, and added into the lane's two running sums;
//   (b) the statistics of both chains: one __shfl_xor(., 32) per sum joins the two lanes of a batch row; the centred
//       second pass re-reads the lane's own windows;
//   (c) per 32-unit block the fold: normalise the five gate tiles of both chains (gamma, beta formed +- from theta and
//       the member's noise row when affine), add, activations; c' to the c windows (un-normalised: it is the state),
//       sigmoid(o) to the o windows, the sum of c' accumulates;
//   (d) the statistics of c', then h' = o * tanh(LN_c(c')) to the other-parity h' windows.
// The pre-activations are stored (10 R / 128 windows), not recomputed in a second tile pass. A lane reloads only what
// it stored itself: no other lane's store has to be visible, no workgroup waits for another, there is no spin loop.
// The arithmetic of a statistic is nicnes_math.h's (nn_ln_*): per lane a sequential sum over its units in ascending
// order, the two lane sums added once.
//
// Lane scratch of a wave, in windows of 16 KiB (decode_wide_kernels.hip): c (R / 128) | h' even | h' odd |
// x (E / 128) | ai (5 R / 128) | ah (5 R / 128) | sigmoid(o) (R / 128) | the row's unfinished flag (64 floats).
struct LnArgs {
    int32_t E, R;
    int32_t affine;                   // 1: elementwise gamma, beta (layer_n_affine), at the offsets below
    uint32_t off_i2h_g, off_i2h_b;    // core.i2h_ln.weight, .bias [5R] (theta offsets, floats)
    uint32_t off_h2h_g, off_h2h_b;    // core.h2h_ln.weight, .bias [5R]
    uint32_t off_c_g, off_c_b;        // core.c_ln.weight, .bias [R]
};

__host__ __device__ static inline size_t ln_wave_floats(int E, int R) {
    return (size_t)(14 * (R >> 7) + (E >> 7)) * (WD_WIN_BYTES / 4) + 64;
}

// what a wave's threads share through the phases of a step
struct LnCtx {
    rsrc_t theta_r, noise_r, scr_r;
    float* lds;
    int tid, lane, hh, sgn;
    int E, R, nE, nR;
    uint32_t C_AT, H_AT, X_AT, AI_AT, AH_AT, O_AT, U_AT;
};

__device__ __forceinline__ LnCtx ln_ctx(const DecodeParams& p, const LnArgs& la, uint64_t nidx, float* wave_scratch,
                                        float* lds, int tid, int sgn) {
    LnCtx c;
    c.theta_r = make_rsrc(p.theta, 4u * (uint32_t)p.D);
    c.noise_r = make_rsrc(p.noise + nidx, 4u * (uint32_t)p.D);
    c.scr_r = make_rsrc(wave_scratch, (uint32_t)(4 * ln_wave_floats(la.E, la.R)));
    c.lds = lds;
    c.tid = tid; c.lane = tid & 63; c.hh = c.lane >> 5; c.sgn = sgn;
    c.E = la.E; c.R = la.R; c.nE = la.E >> 7; c.nR = la.R >> 7;
    c.C_AT = 0u;
    c.H_AT = WD_WIN_BYTES * (uint32_t)c.nR;
    c.X_AT = WD_WIN_BYTES * (uint32_t)(3 * c.nR);
    c.AI_AT = WD_WIN_BYTES * (uint32_t)(3 * c.nR + c.nE);
    c.AH_AT = WD_WIN_BYTES * (uint32_t)(8 * c.nR + c.nE);
    c.O_AT = WD_WIN_BYTES * (uint32_t)(13 * c.nR + c.nE);
    c.U_AT = WD_WIN_BYTES * (uint32_t)(14 * c.nR + c.nE);
    return c;
}

// a phase of ntile tiles, double-buffered, as the wide kernel's run_tiles: tile n + 1 is loaded before tile n's MFMAs
// and stored after them; every iteration ends on a barrier, so both buffers are free when the next phase starts
template <class Desc, class Body>
__device__ __forceinline__ void ln_run_tiles(const LnCtx& c, int ntile, Desc&& desc, Body&& body) {
    StageRegs sr;
    {
        const TileDesc d0 = desc(0);
        stage_load(c.theta_r, c.noise_r, d0, c.tid, sr);
        stage_store(c.lds, d0, c.tid, sr);
    }
    __syncthreads();
#pragma unroll 1
    for (int n = 0; n < ntile; ++n) {
        TileDesc dn = desc(n + 1 < ntile ? n + 1 : n);
        if (n + 1 < ntile) stage_load(c.theta_r, c.noise_r, dn, c.tid, sr);
        const float* buf = c.lds + (n & 1) * STAGE_FLOATS;
        body(n, buf + c.sgn * SIGN_FLOATS, buf + 2 * SIGN_FLOATS + 32 * c.sgn);
        if (n + 1 < ntile) stage_store(c.lds + ((n + 1) & 1) * STAGE_FLOATS, dn, c.tid, sr);
        __syncthreads();
    }
}

// the lane's 16 values of a parameter vector at rows row0 + 8 a + 4 hh .. + 3 (a = 0..3), as W0 +- delta
__device__ __forceinline__ f32x16 ln_vec16(const LnCtx& c, uint32_t off, int row0) {
    f32x16 v;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const uint32_t o = 4u * (off + (uint32_t)(row0 + 8 * a + 4 * c.hh));
        const f32x4 w0 = ld4(c.theta_r, o), delta = ld4(c.noise_r, o);
        const f32x4 q = c.sgn ? (w0 - delta) : (w0 + delta);
        v[4 * a] = q[0]; v[4 * a + 1] = q[1]; v[4 * a + 2] = q[2]; v[4 * a + 3] = q[3];
    }
    return v;
}

// the lane's second pass over ntl blocks of the vector at base: the sequential sum of (a - mean)^2
__device__ __forceinline__ float ln_sumsq(const LnCtx& c, uint32_t base, int ntl, float mean) {
    float q = 0.f;
#pragma unroll 1
    for (int n = 0; n < ntl; ++n) {
        const f32x16 v = wide_load_block(c.scr_r, base, n, c.lane);
#pragma unroll
        for (int r = 0; r < 16; ++r) q = nn_ln_sq(q, v[r], mean);
    }
    return q;
}

// One LSTM cell with layer norm over x (the X windows) and h_t (the h' windows at Hc): c' to the C windows (read from
// there when has_c, else c = 0), h' to the h' windows at Hn. Every thread of the workgroup calls it.
__device__ __forceinline__ void ln_cell(const DecodeParams& p, const LnArgs& la, const LnCtx& c, uint32_t Hc,
                                        uint32_t Hn, bool has_c) {
    const int E = c.E, R = c.R, nE = c.nE, nR = c.nR, lane = c.lane, hh = c.hh;
    const int per = nE + nR, ntl = (5 * R) >> 5, nblk = R >> 5;
    // ---- (a) the gate tiles, rows 32 q .. + 31 of the [5R] pre-activations: E / 128 windows over x, R / 128 over h_t
    float si = 0.f, sh = 0.f;
    {
        f32x16 ai, ah;
        ln_run_tiles(c, ntl * per,
                     [&](int n) {
                         TileDesc d;
                         const int q = n / per, wi = n - q * per;
                         const bool x = wi < nE;
                         d.w_off = (uint32_t)(x ? p.off_i2h_w : p.off_h2h_w); d.ld = x ? E : R;
                         d.row0 = 32 * q; d.nvalid = 32; d.k0 = 128 * (x ? wi : wi - nE);
                         d.b_off = (uint32_t)(x ? p.off_i2h_b : p.off_h2h_b); d.pad_bias = 0.f;
                         return d;
                     },
                     [&](int n, const float* wt, const float* bias) __attribute__((always_inline)) {
                         const int q = n / per, wi = n - q * per;
                         if (wi == 0) ai = bias_init(bias, hh);
                         if (wi == nE) ah = bias_init(bias, hh);
                         if (wi < nE) ai = wide_tile(ai, wt, c.scr_r, c.X_AT + WD_WIN_BYTES * (uint32_t)wi, lane);
                         else ah = wide_tile(ah, wt, c.scr_r, Hc + WD_WIN_BYTES * (uint32_t)(wi - nE), lane);
                         if (wi == nE - 1) {
                             wide_store_block(c.scr_r, c.AI_AT, q, lane, ai);
#pragma unroll
                             for (int r = 0; r < 16; ++r) si = si + ai[r];
                         }
                         if (wi == per - 1) {
                             wide_store_block(c.scr_r, c.AH_AT, q, lane, ah);
#pragma unroll
                             for (int r = 0; r < 16; ++r) sh = sh + ah[r];
                         }
                     });
    }
    // ---- (b) the statistics of the two chains over the row's 5R values (this lane's and lane ^ 32's) ----
    const float mi = nn_ln_mean(si, __shfl_xor(si, 32), 5 * R);
    const float mh = nn_ln_mean(sh, __shfl_xor(sh, 32), 5 * R);
    const float qi = ln_sumsq(c, c.AI_AT, ntl, mi);
    const float qh = ln_sumsq(c, c.AH_AT, ntl, mh);
    const float di = nn_ln_den(qi, __shfl_xor(qi, 32), 5 * R);
    const float dh = nn_ln_den(qh, __shfl_xor(qh, 32), 5 * R);
    // ---- (c) the fold, a 32-unit block at a time ----
    // gate chunk ch (i, f, o, g1, g2 = 0..4, nets.py:110-121) of block j: s = LN(i2h(x)) + LN(h2h(h))
    auto gate = [&](int ch, int j) __attribute__((always_inline)) {
        const int tq = ch * nblk + j;
        const f32x16 vi = wide_load_block(c.scr_r, c.AI_AT, tq, lane);
        const f32x16 vh = wide_load_block(c.scr_r, c.AH_AT, tq, lane);
        f32x16 s;
        if (la.affine) {
            const f32x16 gi = ln_vec16(c, la.off_i2h_g, 32 * tq), bi = ln_vec16(c, la.off_i2h_b, 32 * tq);
            const f32x16 gh = ln_vec16(c, la.off_h2h_g, 32 * tq), bh = ln_vec16(c, la.off_h2h_b, 32 * tq);
#pragma unroll
            for (int r = 0; r < 16; ++r)
                s[r] = nn_ln_affine(nn_ln_y(vi[r], mi, di), gi[r], bi[r]) + nn_ln_affine(nn_ln_y(vh[r], mh, dh), gh[r], bh[r]);
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = nn_ln_y(vi[r], mi, di) + nn_ln_y(vh[r], mh, dh);
        }
        return s;
    };
    float sc = 0.f;
#pragma unroll 1
    for (int j = 0; j < nblk; ++j) {
        const f32x16 g1 = gate(3, j), g2 = gate(4, j), gin = gate(0, j), gf = gate(1, j);
        f32x16 cp = wide_load_block(c.scr_r, c.C_AT, j, lane);
        f32x16 cn;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            cn[r] = nn_lstm_cell_ln_c(gin[r], gf[r], g1[r], g2[r], has_c ? cp[r] : 0.f);
            sc = sc + cn[r];
        }
        wide_store_block(c.scr_r, c.C_AT, j, lane, cn);
        f32x16 og = gate(2, j);
#pragma unroll
        for (int r = 0; r < 16; ++r) og[r] = CELL_SIG(og[r]);
        wide_store_block(c.scr_r, c.O_AT, j, lane, og);
    }
    // ---- (d) the statistic of c' over the row's R values, then h' = o * tanh(LN_c(c')) ----
    const float mc = nn_ln_mean(sc, __shfl_xor(sc, 32), R);
    const float qc = ln_sumsq(c, c.C_AT, nblk, mc);
    const float dc = nn_ln_den(qc, __shfl_xor(qc, 32), R);
#pragma unroll 1
    for (int j = 0; j < nblk; ++j) {
        const f32x16 cn = wide_load_block(c.scr_r, c.C_AT, j, lane);
        const f32x16 og = wide_load_block(c.scr_r, c.O_AT, j, lane);
        f32x16 hn;
        if (la.affine) {
            const f32x16 gc = ln_vec16(c, la.off_c_g, 32 * j), bc = ln_vec16(c, la.off_c_b, 32 * j);
#pragma unroll
            for (int r = 0; r < 16; ++r)
                hn[r] = nn_lstm_cell_ln_h(og[r], nn_ln_affine(nn_ln_y(cn[r], mc, dc), gc[r], bc[r]));
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) hn[r] = nn_lstm_cell_ln_h(og[r], nn_ln_y(cn[r], mc, dc));
        }
        wide_store_block(c.scr_r, Hn, j, lane, hn);
    }
}

// grid (members, slabs)
__global__ __launch_bounds__(NTHREADS) void nicnes_decode_ln_kernel(DecodeParams p, LnArgs la) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int sgn = wave >> 2, grp = wave & 3;
    const int member = blockIdx.x, slab = blockIdx.y, wg = member * gridDim.y + slab;
    const int b = slab * 128 + grp * 32 + (lane & 31);
    const bool row_valid = row_ok(p, b, sgn);
    const int E = la.E, R = la.R, nE = E >> 7, nR = R >> 7, nK = p.F >> 7;
    const LnCtx c = ln_ctx(p, la, p.noise_idx[member], p.scratch + ((size_t)wg * 8 + wave) * ln_wave_floats(E, R), lds,
                           tid, sgn);
    const rsrc_t scr_r = c.scr_r;
    const uint32_t lo = 4u * (uint32_t)lane;

    // ---- x of t = 0: img_embed(fc) (nets.py:194-195), unit block by unit block; h = 0, every row unfinished ----
    {
        const float* fcm = p.fc + (p.member_batch ? (size_t)p.member_batch[member] * p.B_img * p.F : 0);
        const rsrc_t fc_r = make_rsrc(fcm, 4u * (uint32_t)p.B_img * (uint32_t)p.F);
        const int fr = row_valid ? (b + sgn * p.sign_off) / p.rpi : 0;      // the lane's fc row (its image)
        f32x16 acc;
        ln_run_tiles(c, (E >> 5) * nK,
                     [&](int n) {
                         TileDesc d;
                         d.w_off = (uint32_t)p.off_img_w; d.ld = p.F; d.row0 = 32 * (n / nK); d.nvalid = 32;
                         d.k0 = 128 * (n % nK); d.b_off = (uint32_t)p.off_img_b; d.pad_bias = 0.f;
                         return d;
                     },
                     [&](int n, const float* wt, const float* bias) __attribute__((always_inline)) {
                         const int U = n / nK, kc = n - U * nK;
                         if (kc == 0) acc = bias_init(bias, hh);
                         acc = mfma_tile_fc(acc, wt, fc_r, 4u * (uint32_t)(fr * p.F + 128 * kc + 4 * hh), lane);
                         if (kc == nK - 1) wide_store_block(scr_r, c.X_AT, U, lane, acc);
                     });
        const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
        for (int g = 0; g < 16 * nR; ++g) st4(scr_r, 16u * (uint32_t)lane, c.H_AT + WD_GRP_BYTES * (uint32_t)g, z4);
        st1(scr_r, lo, c.U_AT, 1.0f);
        if (tid == 0) p.alive[wg] = 1;
    }

    const int nvt = 2 * ((p.V1 + 63) >> 6);          // 32-row vocabulary tiles, two per 64-row stage (the fused loop's)
    auto logit_desc = [&](int n) {
        TileDesc d;
        const int v = n / nR;
        d.w_off = (uint32_t)p.off_log_w; d.ld = R; d.row0 = 32 * v; d.nvalid = min(32, max(p.V1 - 32 * v, 0));
        d.k0 = 128 * (n - v * nR); d.b_off = (uint32_t)p.off_log_b; d.pad_bias = NEG_INF;
        return d;
    };
    int cur = 0;                                     // h_t is the h' copy of this parity
#pragma unroll 1
    for (int t = -1; t <= p.T; ++t) {
        const uint32_t Hc = c.H_AT + WD_WIN_BYTES * (uint32_t)(cur * nR);
        int it = 0;                                  // token fed to the next cell (0 = BOS at t = 0)
        if (t > 0) {
            // ---- logits of step t over h_t, the greedy state stage by stage (nets.py:202,208) ----
            const float unf_prev = ld1(scr_r, lo, c.U_AT);
            RowState st;
            row_state_init(st);
            f32x16 acc, P0;
            ln_run_tiles(c, nvt * nR, logit_desc, [&](int n, const float* wt, const float* bias) __attribute__((always_inline)) {
                const int v = n / nR, win = n - v * nR;
                if (win == 0) acc = bias_init(bias, hh);
                acc = wide_tile(acc, wt, scr_r, Hc + WD_WIN_BYTES * (uint32_t)win, lane);
                if (win == nR - 1) {
                    if (v & 1) epilogue64<false>(st, P0, acc, 32 * (v - 1) + 4 * hh);
                    else P0 = acc;
                }
            });
            // ---- greedy token (nets.py:208-209): the fused kernel's rule with the exact lse ----
            const float m_o = __shfl_xor(st.m, 32);
            const float s_o = __shfl_xor(st.s, 32);
            const float m = fmaxf(st.m, m_o);
            const float stot = st.s * __builtin_amdgcn_exp2f((st.m - m) * LOG2E) +
                               s_o * __builtin_amdgcn_exp2f((m_o - m) * LOG2E);
            const TieWindow w = tie_window(stot, false, p.lse_margin);
            const float lse = w.lse;
            int tok = 0x7fffffff;
            const float cv[4] = {st.r0v, st.r1v, __shfl_xor(st.r0v, 32), __shfl_xor(st.r1v, 32)};
            const int ci[4] = {st.r0i, st.r1i, __shfl_xor(st.r0i, 32), __shfl_xor(st.r1i, 32)};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (win_state(cv[k], m, w) == 1 && ci[k] < tok) tok = ci[k];
            const bool ovf = p.force_exact || win_state(st.ev, m, w) != 0 || win_state(__shfl_xor(st.ev, 32), m, w) != 0;
            if (__syncthreads_or(ovf ? 1 : 0)) {
                // rare: more records than tracked fall in the tie window -> the first id in the window, by a second sweep
                int best = 0x7fffffff;
                const int nv32 = (p.V1 + 31) >> 5;
                ln_run_tiles(c, nv32 * nR, logit_desc,
                             [&](int n, const float* wt, const float* bias) __attribute__((always_inline)) {
                    const int v = n / nR, win = n - v * nR;
                    if (win == 0) acc = bias_init(bias, hh);
                    acc = wide_tile(acc, wt, scr_r, Hc + WD_WIN_BYTES * (uint32_t)win, lane);
                    if (win == nR - 1) logit_epilogue_exact(best, acc, 32 * v + 4 * hh, m, lse);
                });
                tok = min(best, __shfl_xor(best, 32));
                if (tid == 0) atomicAdd(p.stats + 0, 1);
            }
            // no candidate only when every logit is NaN: end the caption instead of emitting an out-of-vocabulary id
            if (tok >= p.V1) tok = 0;
            const bool unfinished = unf_prev != 0.f && tok > 0;      // finished mask (nets.py:236-243)
            it = (unfinished || p.no_mask) ? tok : 0;
            st1(scr_r, lo, c.U_AT, unfinished ? 1.f : 0.f);
            if (hh == 0 && row_valid) {
                const size_t o = (((size_t)member * 2 + sgn) * p.B + b) * p.T + (t - 1);
                p.seq[o] = it;
                if (p.lp) p.lp[o] = -lse;            // seq_logprobs[:, t-1] = max lp = fp32((m - m) - lse)
            }
            const int any = __syncthreads_or(((unfinished && row_valid) || p.no_exit) ? 1 : 0);
            if (tid == 0) p.alive[wg] = any;
            if (!any) break;                         // the reference stops here (nets.py:242-243)
        }
        if (t >= p.T) break;

        // ---- LSTM cell of step t + 1 (nets.py:98-134, layer_n) ----
        if (t >= 0) {                                // x = embed(it) (nets.py:196-199): the lane's k subset, +- delta
            const uint32_t eo = 4u * ((uint32_t)p.off_emb_w + (uint32_t)it * (uint32_t)E + 4u * (uint32_t)hh);
            for (int g = 0; g < 16 * nE; ++g) {      // group g: k = 128 (g / 16) + 32 ((g / 4) % 4) + 8 (g % 4) + 4 hh ..
                const uint32_t ko = eo + 4u * (uint32_t)(128 * (g >> 4) + 32 * ((g >> 2) & 3) + 8 * (g & 3));
                const f32x4 w0 = ld4(c.theta_r, ko), delta = ld4(c.noise_r, ko);
                st4(scr_r, 16u * (uint32_t)lane, c.X_AT + WD_GRP_BYTES * (uint32_t)g, sgn ? (w0 - delta) : (w0 + delta));
            }
        }
        ln_cell(p, la, c, Hc, c.H_AT + WD_WIN_BYTES * (uint32_t)((cur ^ 1) * nR), t >= 0);
        cur ^= 1;
    }
}

// ========== test entry (nicnes_test_ln_cell): one cell of theta itself on given rows ==================================
// One workgroup of the decode's shape. xin [rows, E], hin [rows, R], cin [rows, R] (unit order) are spread to the eight
// waves' lane scratch in the decode's layout (wave w: sign w >> 2, rows 32 (w & 3) .. + 31; both signs the same rows,
// the noise row is zero), ln_cell runs once, and the waves of sign 0 write h' and c' back in unit order.
__global__ __launch_bounds__(NTHREADS) void nicnes_test_ln_cell_kernel(DecodeParams p, LnArgs la, const float* xin,
                                                                       const float* hin, const float* cin, int rows,
                                                                       float* hout, float* cout) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int sgn = wave >> 2, row = (wave & 3) * 32 + (lane & 31);
    const bool ok = row < rows;
    const LnCtx c = ln_ctx(p, la, 0, p.scratch + (size_t)wave * ln_wave_floats(la.E, la.R), lds, tid, sgn);
    // group g of a vector's windows holds units 128 (g / 16) + 32 ((g / 4) % 4) + 8 (g % 4) + 4 hh .. + 3
    auto unit_of = [&](int g) { return 128 * (g >> 4) + 32 * ((g >> 2) & 3) + 8 * (g & 3) + 4 * hh; };
    auto spread = [&](const float* in, int n, uint32_t at) {
        for (int g = 0; g < n >> 3; ++g) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (ok) v = *reinterpret_cast<const f32x4*>(in + (size_t)row * n + unit_of(g));
            st4(c.scr_r, 16u * (uint32_t)lane, at + WD_GRP_BYTES * (uint32_t)g, v);
        }
    };
    spread(xin, la.E, c.X_AT);
    spread(hin, la.R, c.H_AT);
    spread(cin, la.R, c.C_AT);
    const uint32_t Hn = c.H_AT + WD_WIN_BYTES * (uint32_t)c.nR;
    ln_cell(p, la, c, c.H_AT, Hn, true);
    if (ok && sgn == 0)
        for (int g = 0; g < la.R >> 3; ++g) {
            const size_t o = (size_t)row * la.R + unit_of(g);
            *reinterpret_cast<f32x4*>(hout + o) = ld4(c.scr_r, 16u * (uint32_t)lane, Hn + WD_GRP_BYTES * (uint32_t)g);
            *reinterpret_cast<f32x4*>(cout + o) = ld4(c.scr_r, 16u * (uint32_t)lane, c.C_AT + WD_GRP_BYTES * (uint32_t)g);
        }
}

extern "C" size_t nicnes_ln_scratch_floats(int64_t workgroups, int E, int R) {
    return (size_t)workgroups * 8 * ln_wave_floats(E, R);
}

// per device, once per handle (nicnes_create): the kernels' dynamic LDS is above 64 KB
extern "C" hipError_t nicnes_decode_ln_init() {
    hipError_t e = hipFuncSetAttribute((const void*)nicnes_decode_ln_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)LDS32);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void*)nicnes_test_ln_cell_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)LDS32);
}

static bool ln_args_ok(const LnArgs& la) {
    const auto okw = [](int w) { return w == 128 || w == 256 || w == 384 || w == 512; };
    // every lane offset is a 32-bit byte offset into its wave's scratch, theta or the member's noise row
    return okw(la.E) && okw(la.R) && 4 * ln_wave_floats(la.E, la.R) < ((size_t)1 << 31);
}

static LnArgs ln_args(int E, int R, const int64_t* tail6) {
    LnArgs la{};
    la.E = E; la.R = R; la.affine = tail6 ? 1 : 0;
    if (tail6) {
        la.off_i2h_g = (uint32_t)tail6[0]; la.off_i2h_b = (uint32_t)tail6[1];
        la.off_h2h_g = (uint32_t)tail6[2]; la.off_h2h_b = (uint32_t)tail6[3];
        la.off_c_g = (uint32_t)tail6[4]; la.off_c_b = (uint32_t)tail6[5];
    }
    return la;
}

// The layer-norm greedy decode of member_count members x nslabs 128-row slabs (p->G == 4, p->S == 1; p->scratch holds
// nicnes_ln_scratch_floats(member_count * nslabs, E, R) floats): one launch. tail6: the theta offsets of the six affine
// tensors (nicnes_param_offsets_ln), NULL without affine. evs / kinds / n_launch as nicnes_launch_decode.
extern "C" hipError_t nicnes_launch_decode_ln(const DecodeParams* p, int E, int R, const int64_t* tail6,
                                              int member_count, int nslabs, hipStream_t stream, hipEvent_t* evs,
                                              int* kinds, int* n_launch) {
    const LnArgs la = ln_args(E, R, tail6);
    if (!ln_args_ok(la) || p->G != 4 || p->S != 1 || p->coop || p->sample_u) return hipErrorInvalidValue;
    if (evs) (void)hipEventRecord(evs[0], stream);
    hipLaunchKernelGGL(nicnes_decode_ln_kernel, dim3(member_count, nslabs), dim3(NTHREADS), LDS32, stream, *p, la);
    if (evs) {
        kinds[1] = DK_STEPS;
        (void)hipEventRecord(evs[1], stream);
    }
    if (n_launch) *n_launch = evs ? 2 : 0;
    return hipGetLastError();
}

// test entry (nicnes_test_ln_cell): p->noise holds D zeros, p->scratch one workgroup's lane scratch; rows <= 128
extern "C" hipError_t nicnes_launch_test_ln_cell(const DecodeParams* p, int E, int R, const int64_t* tail6,
                                                 const float* xin, const float* hin, const float* cin, int rows,
                                                 float* hout, float* cout, hipStream_t stream) {
    const LnArgs la = ln_args(E, R, tail6);
    if (!ln_args_ok(la) || rows < 1 || rows > 128) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nicnes_test_ln_cell_kernel, dim3(1), dim3(NTHREADS), LDS32, stream, *p, la, xin, hin, cin, rows,
                       hout, cout);
    return hipGetLastError();
}
