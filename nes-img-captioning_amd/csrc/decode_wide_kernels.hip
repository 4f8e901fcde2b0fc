// decode_wide_kernels.hip -- the greedy decode of models wider than 128 units, E = input_encoding_size and R = rnn_size
// each in {128, 256, 384, 512} (DESIGN.md "Wide models"): the step-loop frame every such decode runs in (wide_decode),
// the plain LSTM cell (wide_cell) and the host side of both kernels built on the frame. The layer-norm cell
// (decode_ln_kernels.hip) is #included below, between the frame and the host side.
// Not a translation unit of its own: decode_kernel.hip #includes this file ahead of its last kernel (the Makefile lists
// it as a dependency), so the library keeps its five code objects and this file uses that unit's tile helpers
// (TileDesc, stage_load / stage_store, bias_init, mfma_tile_fc, RowState, epilogue64, tie_window / win_state).
//
// One workgroup = one member (both signs) x one slab of <= 128 rows; wave w = sign (w >> 2) x 32-row group (w & 3), as
// on the fused path; every step t = -1 .. T in one launch, the image projection in front of them. Every dense product
// over K in {F, E, R} is a chain of K / 128 tiles of 32 rows x 128 k (windows ascending, nn_kperm's order inside a
// window) into one accumulator that starts at the bias: the oracle's gemv_chain. The tiles of a phase run through the
// two 32-row LDS stage buffers (W0 +- delta for both signs, formed once).
//
// The B operand. After a tile the 32x32 accumulator holds, per lane, 16 of the 32 units of its batch row, in the order
// the next product's MFMAs consume them (nn_kperm), so a lane needs as B operand exactly the units it produced itself.
// R / 2 values of h per lane do not fit the register file at R = 512, so h', c and x live in lane-private global
// scratch and a tile streams its 64-value window from there, four values per load (wide_tile, as mfma_tile_fc streams
// the fc row). A lane reloads only what it stored: no other lane's store has to be visible, no workgroup waits for
// another. h' has two copies by step parity (the cell of step t + 1 reads all of h_t while it writes h_{t+1} block by
// block); c is updated in place (block j of c is read only when block j folds).
//
// Lane scratch of a wave, in windows of 16 KiB = [16 groups][64 lanes][4 floats] (a group is the four values of one
// 16-byte load; unit block j = window j / 4, groups 4 (j % 4) .. + 3): c (R / 128 windows) | h' even | h' odd |
// x (E / 128) | the cell's private windows (none for the plain cell) | the row's unfinished flag (64 floats). The
// engine sizes it from (E, R) and the cell: nicnes_wide_scratch_floats.
//
// The frame and its cell. wide_decode owns everything but the recurrence: the image projection, h = 0, the logit
// sweep, the token rule, the seq / lp / alive stores, the early exit and the embedding gather. Once per step it calls
// cell(Hc, Hn, has_c), which every thread of the workgroup runs: read x from the X windows and h_t from the h' windows
// at Hc, read c from the C windows when has_c (else c = 0), write c' to the C windows and h' to the h' windows at Hn.
// A cell runs its tiles through wide_run_tiles, may keep what it likes in its private windows (WideCtx::P_AT; their
// count is the extra_windows of wide_ctx and of the host side), and must leave the stage buffers free (wide_run_tiles
// does) and every other window alone.
//
// Exact exp-sum only (epilogue64<false>): no pair bound, no screening, no step queue, no coop or split shape.
#define WD_WIN_BYTES 16384u
#define WD_GRP_BYTES 1024u

struct WideArgs {
    int32_t E, R;
};

// floats of a wave's lane scratch; extra_windows: the cell's private windows
__host__ __device__ static inline size_t wide_wave_floats(int E, int R, int extra_windows) {
    return (size_t)(3 * (R >> 7) + (E >> 7) + extra_windows) * (WD_WIN_BYTES / 4) + 64;
}

__device__ __forceinline__ void st4(rsrc_t r, uint32_t byte_off, uint32_t soff, const f32x4& v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, (int)byte_off, (int)soff, 0);
}

// acc += W_tile(32 x 128, LDS) . B(128 x 32): the B window at win_off of the wave's lane scratch, read per 32-k block
__device__ __forceinline__ f32x16 wide_tile(f32x16 acc, const float* w, rsrc_t scr_r, uint32_t win_off, int lane) {
    const float* row = w + (lane & 31) * LDS_ROW + (lane >> 5) * 16;
    const uint32_t lo = 16u * (uint32_t)lane;
#pragma unroll
    for (int T = 0; T < 4; ++T) {
        f32x4 a[4], bq[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            a[c] = *reinterpret_cast<const f32x4*>(row + T * 32 + 4 * c);
            bq[c] = ld4(scr_r, lo, win_off + WD_GRP_BYTES * (uint32_t)(4 * T + c));
        }
#pragma unroll
        for (int jj = 0; jj < 16; ++jj)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[jj >> 2][jj & 3], bq[jj >> 2][jj & 3], acc, 0, 0, 0);
    }
    return acc;
}

// the accumulator of unit block j of a vector whose windows start at base: groups 4 (j % 4) .. + 3 of window j / 4
__device__ __forceinline__ uint32_t wide_block_off(uint32_t base, int j) {
    return base + WD_WIN_BYTES * (uint32_t)(j >> 2) + WD_GRP_BYTES * (uint32_t)(4 * (j & 3));
}
__device__ __forceinline__ void wide_store_block(rsrc_t scr_r, uint32_t base, int j, int lane, const f32x16& v) {
    const uint32_t o = wide_block_off(base, j);
#pragma unroll
    for (int a = 0; a < 4; ++a)
        st4(scr_r, 16u * (uint32_t)lane, o + WD_GRP_BYTES * (uint32_t)a,
            f32x4{v[4 * a], v[4 * a + 1], v[4 * a + 2], v[4 * a + 3]});
}
__device__ __forceinline__ f32x16 wide_load_block(rsrc_t scr_r, uint32_t base, int j, int lane) {
    const uint32_t o = wide_block_off(base, j);
    f32x16 v;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const f32x4 q = ld4(scr_r, 16u * (uint32_t)lane, o + WD_GRP_BYTES * (uint32_t)a);
        v[4 * a] = q[0]; v[4 * a + 1] = q[1]; v[4 * a + 2] = q[2]; v[4 * a + 3] = q[3];
    }
    return v;
}
// the first of the four units that group g of a vector's windows holds for the lanes of half hh
__device__ __forceinline__ int wide_group_unit(int g, int hh) {
    return 128 * (g >> 4) + 32 * ((g >> 2) & 3) + 8 * (g & 3) + 4 * hh;
}

// what a wave's threads share through the phases of a step
struct WideCtx {
    rsrc_t theta_r, noise_r, scr_r;
    float* lds;
    int tid, lane, hh, sgn;
    int E, R, nE, nR;
    uint32_t C_AT, H_AT, X_AT, P_AT, U_AT;    // window bases (bytes): c | h' x 2 | x | the cell's private windows | flag
};

// The scratch resource spans the whole wave scratch, the cell's extra_windows private windows included, and the
// unfinished flag stays behind them: an offset past the end reads zero, it does not fault.
__device__ __forceinline__ WideCtx wide_ctx(const DecodeParams& p, int E, int R, int extra_windows, uint64_t nidx,
                                            float* wave_scratch, float* lds, int tid, int sgn) {
    WideCtx c;
    c.theta_r = make_rsrc(p.theta, 4u * (uint32_t)p.D);
    c.noise_r = make_rsrc(p.noise + nidx, 4u * (uint32_t)p.D);
    c.scr_r = make_rsrc(wave_scratch, (uint32_t)(4 * wide_wave_floats(E, R, extra_windows)));
    c.lds = lds;
    c.tid = tid; c.lane = tid & 63; c.hh = c.lane >> 5; c.sgn = sgn;
    c.E = E; c.R = R; c.nE = E >> 7; c.nR = R >> 7;
    c.C_AT = 0u;
    c.H_AT = WD_WIN_BYTES * (uint32_t)c.nR;
    c.X_AT = WD_WIN_BYTES * (uint32_t)(3 * c.nR);
    c.P_AT = WD_WIN_BYTES * (uint32_t)(3 * c.nR + c.nE);
    c.U_AT = WD_WIN_BYTES * (uint32_t)(3 * c.nR + c.nE + extra_windows);
    return c;
}

// the context of a decode workgroup's thread: grid (members, slabs), wave w of workgroup wg on the w-th wave scratch of wg
__device__ __forceinline__ WideCtx wide_decode_ctx(const DecodeParams& p, int E, int R, int extra_windows, float* lds) {
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wg = blockIdx.x * gridDim.y + blockIdx.y;
    return wide_ctx(p, E, R, extra_windows, p.noise_idx[blockIdx.x],
                    p.scratch + ((size_t)wg * 8 + wave) * wide_wave_floats(E, R, extra_windows), lds, tid, wave >> 2);
}

// a phase: ntile tiles, double-buffered; tile n + 1 is loaded before tile n's MFMAs and stored after them. Every
// iteration ends on a barrier, so both buffers are free when the next phase starts
template <class Desc, class Body>
__device__ __forceinline__ void wide_run_tiles(const WideCtx& c, int ntile, Desc&& desc, Body&& body) {
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

// The decode of one member x one slab around `cell` (the file header says what a cell must do); c: wide_decode_ctx's
template <class Cell>
__device__ __forceinline__ void wide_decode(const DecodeParams& p, const WideCtx& c, Cell&& cell) {
    const int tid = c.tid, lane = c.lane, hh = c.hh, sgn = c.sgn;
    const int grp = __builtin_amdgcn_readfirstlane(tid >> 6) & 3;
    const int member = blockIdx.x, slab = blockIdx.y, wg = member * gridDim.y + slab;
    const int b = slab * 128 + grp * 32 + (lane & 31);
    const bool row_valid = row_ok(p, b, sgn);
    const int E = c.E, R = c.R, nE = c.nE, nR = c.nR, nK = p.F >> 7;
    const rsrc_t scr_r = c.scr_r;
    const uint32_t lo = 4u * (uint32_t)lane;

    // ---- x of t = 0: img_embed(fc) (nets.py:194-195), unit block by unit block; h = 0, every row unfinished ----
    {
        const float* fcm = p.fc + (p.member_batch ? (size_t)p.member_batch[member] * p.B_img * p.F : 0);
        const rsrc_t fc_r = make_rsrc(fcm, 4u * (uint32_t)p.B_img * (uint32_t)p.F);
        const int fr = row_valid ? (b + sgn * p.sign_off) / p.rpi : 0;      // the lane's fc row (its image)
        f32x16 acc;
        wide_run_tiles(c, (E >> 5) * nK,
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
            wide_run_tiles(c, nvt * nR, logit_desc,
                           [&](int n, const float* wt, const float* bias) __attribute__((always_inline)) {
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
                wide_run_tiles(c, nv32 * nR, logit_desc,
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

        // ---- LSTM cell of step t + 1 (nets.py:98-134) ----
        if (t >= 0) {                                // x = embed(it) (nets.py:196-199): the lane's k subset, +- delta
            const uint32_t eo = 4u * ((uint32_t)p.off_emb_w + (uint32_t)it * (uint32_t)E);
            for (int g = 0; g < 16 * nE; ++g) {
                const uint32_t ko = eo + 4u * (uint32_t)wide_group_unit(g, hh);
                const f32x4 w0 = ld4(c.theta_r, ko), delta = ld4(c.noise_r, ko);
                st4(scr_r, 16u * (uint32_t)lane, c.X_AT + WD_GRP_BYTES * (uint32_t)g, sgn ? (w0 - delta) : (w0 + delta));
            }
        }
        cell(Hc, c.H_AT + WD_WIN_BYTES * (uint32_t)((cur ^ 1) * nR), t >= 0);
        cur ^= 1;
    }
}

// The plain LSTM cell: gate sums s = (b_i2h + Wi.x) + (b_h2h + Wh.h) (nets.py:109-111), a 32-unit gate tile at a time
// in the fold order g1, g2, i, f, o of each unit block: E / 128 windows over x, then R / 128 over h_t
__device__ __forceinline__ void wide_cell(const DecodeParams& p, const WideCtx& c, uint32_t Hc, uint32_t Hn, bool has_c) {
    const int E = c.E, R = c.R, nE = c.nE, lane = c.lane, hh = c.hh;
    const rsrc_t scr_r = c.scr_r;
    const int per = nE + c.nR;
    f32x16 ai, ah, hold;
    wide_run_tiles(c, (R >> 5) * 5 * per,
                   [&](int n) {
                       TileDesc d;
                       const int q = n / per, wi = n - q * per, j = q / 5, gi = q - 5 * j;
                       const bool x = wi < nE;
                       d.w_off = (uint32_t)(x ? p.off_i2h_w : p.off_h2h_w); d.ld = x ? E : R;
                       d.row0 = tile_q(gi) * R + 32 * j; d.nvalid = 32; d.k0 = 128 * (x ? wi : wi - nE);
                       d.b_off = (uint32_t)(x ? p.off_i2h_b : p.off_h2h_b); d.pad_bias = 0.f;
                       return d;
                   },
                   [&](int n, const float* wt, const float* bias) __attribute__((always_inline)) {
                       const int q = n / per, wi = n - q * per, j = q / 5, gi = q - 5 * j;
                       // one running accumulator for both chains (the i2h chain is set aside when it ends): with two,
                       // the compiler copies 48 registers around every tile once the cell is a function of its own
                       if (wi == 0 || wi == nE) ah = bias_init(bias, hh);
                       ah = wide_tile(ah, wt, scr_r, wi < nE ? c.X_AT + WD_WIN_BYTES * (uint32_t)wi
                                                             : Hc + WD_WIN_BYTES * (uint32_t)(wi - nE), lane);
                       if (wi == nE - 1) ai = ah;
                       if (wi != per - 1) return;
                       const f32x16 s_ = ai + ah;     // i2h(x) + h2h(h)
                       if (gi == 0) {                 // g1
                           hold = s_;
                       } else if (gi == 1) {          // g = max(g1, g2)
#pragma unroll
                           for (int r = 0; r < 16; ++r) hold[r] = hold[r] > s_[r] ? hold[r] : s_[r];
                       } else if (gi == 2) {          // ig * g
#pragma unroll
                           for (int r = 0; r < 16; ++r) hold[r] = CELL_SIG(s_[r]) * hold[r];
                       } else if (gi == 3) {          // c' = f * c + ig * g (c = 0 before the first cell)
                           f32x16 cp = wide_load_block(scr_r, c.C_AT, j, lane);
#pragma unroll
                           for (int r = 0; r < 16; ++r) {
                               const float fcv = CELL_SIG(s_[r]) * (has_c ? cp[r] : 0.f);
                               hold[r] = fcv + hold[r];
                           }
                           wide_store_block(scr_r, c.C_AT, j, lane, hold);
                       } else {                       // h' = o * tanh(c')
                           f32x16 hn;
#pragma unroll
                           for (int r = 0; r < 16; ++r) hn[r] = CELL_SIG(s_[r]) * CELL_TANH(hold[r]);
                           wide_store_block(scr_r, Hn, j, lane, hn);
                       }
                   });
}

// grid (members, slabs)
__global__ __launch_bounds__(NTHREADS) void nicnes_decode_wide_kernel(DecodeParams p, WideArgs wa) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const WideCtx c = wide_decode_ctx(p, wa.E, wa.R, 0, lds);
    wide_decode(p, c, [&](uint32_t Hc, uint32_t Hn, bool has_c) __attribute__((always_inline)) {
        wide_cell(p, c, Hc, Hn, has_c);
    });
}

// the widths and the cell's windows a launch can take
static bool wide_dims_ok(int E, int R, int extra_windows) {
    const auto okw = [](int w) { return w == 128 || w == 256 || w == 384 || w == 512; };
    // every lane offset is a 32-bit byte offset into its wave's scratch, theta or the member's noise row
    return okw(E) && okw(R) && 4 * wide_wave_floats(E, R, extra_windows) < ((size_t)1 << 31);
}

// the layer-norm cell, its decode kernel and its test entry
#include "decode_ln_kernels.hip"

// ========== host side of both decode kernels ===========================================================================
extern "C" size_t nicnes_wide_scratch_floats(int64_t workgroups, int E, int R, int ln) {
    return (size_t)workgroups * 8 * wide_wave_floats(E, R, ln ? ln_extra_windows(R) : 0);
}

// per device, once per handle (nicnes_create): the kernels' dynamic LDS is above 64 KB
extern "C" hipError_t nicnes_decode_wide_init() {
    for (const void* k : {(const void*)nicnes_decode_wide_kernel, (const void*)nicnes_decode_ln_kernel,
                          (const void*)nicnes_test_ln_cell_kernel}) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS32);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The wide greedy decode of member_count members x nslabs 128-row slabs (p->G == 4, p->S == 1; p->scratch holds
// nicnes_wide_scratch_floats(member_count * nslabs, E, R, ln) floats): one launch, of the layer-norm kernel when ln.
// tail6: the theta offsets of the six affine tensors (nicnes_param_offsets_ln), NULL without affine (and without ln).
// evs / kinds / n_launch as nicnes_launch_decode.
extern "C" hipError_t nicnes_launch_decode_wide(const DecodeParams* p, int E, int R, int ln, const int64_t* tail6,
                                                int member_count, int nslabs, hipStream_t stream, hipEvent_t* evs,
                                                int* kinds, int* n_launch) {
    if (!wide_dims_ok(E, R, ln ? ln_extra_windows(R) : 0) || p->G != 4 || p->S != 1 || p->coop || p->sample_u)
        return hipErrorInvalidValue;
    if (evs) (void)hipEventRecord(evs[0], stream);
    const dim3 grid(member_count, nslabs);
    if (ln)
        hipLaunchKernelGGL(nicnes_decode_ln_kernel, grid, dim3(NTHREADS), LDS32, stream, *p, ln_args(E, R, tail6));
    else
        hipLaunchKernelGGL(nicnes_decode_wide_kernel, grid, dim3(NTHREADS), LDS32, stream, *p, WideArgs{E, R});
    if (evs) {
        kinds[1] = DK_STEPS;
        (void)hipEventRecord(evs[1], stream);
    }
    if (n_launch) *n_launch = evs ? 2 : 0;
    return hipGetLastError();
}
