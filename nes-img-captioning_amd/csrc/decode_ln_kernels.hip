// decode_ln_kernels.hip -- the greedy decode of layer_n models (LSTMCore with nn.LayerNorm on i2h(x), h2h(h) and c',
// src/captioning/nets.py:92-96,102-104,126-127), for every supported width E, R in {128, 256, 384, 512}
// (DESIGN.md "Layer-norm models").
// Not a translation unit of its own: decode_wide_kernels.hip #includes this file behind its frame (wide_decode, WideCtx,
// wide_run_tiles) and window helpers (wide_tile, wide_store_block / wide_load_block, st4, WD_WIN_BYTES) and ahead of
// the host side, which launches both decode kernels. Only what is layer norm is here: the cell, the decode kernel that
// hands it to the frame, and the cell's test entry.
//
// The decode is the frame's: workgroup and wave roles, the image projection, the logit phase, the token rule, the
// early exit and the embedding gather. The cell is what differs: a layer norm needs the whole row of 5R gate
// pre-activations before any of them can be used, so the cell runs in phases:
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
// The cell's private windows of the wave's lane scratch (decode_wide_kernels.hip), 11 R / 128 of them from
// WideCtx::P_AT: ai (5 R / 128) | ah (5 R / 128) | sigmoid(o) (R / 128).
struct LnArgs {
    int32_t E, R;
    int32_t affine;                   // 1: elementwise gamma, beta (layer_n_affine), at the offsets below
    uint32_t off_i2h_g, off_i2h_b;    // core.i2h_ln.weight, .bias [5R] (theta offsets, floats)
    uint32_t off_h2h_g, off_h2h_b;    // core.h2h_ln.weight, .bias [5R]
    uint32_t off_c_g, off_c_b;        // core.c_ln.weight, .bias [R]
};

// the cell's private windows: wide_ctx's and the host side's extra_windows
__host__ __device__ static inline int ln_extra_windows(int R) { return 11 * (R >> 7); }

// the lane's 16 values of a parameter vector at rows row0 + 8 a + 4 hh .. + 3 (a = 0..3), as W0 +- delta
__device__ __forceinline__ f32x16 ln_vec16(const WideCtx& c, uint32_t off, int row0) {
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
__device__ __forceinline__ float ln_sumsq(const WideCtx& c, uint32_t base, int ntl, float mean) {
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
__device__ __forceinline__ void ln_cell(const DecodeParams& p, const LnArgs& la, const WideCtx& c, uint32_t Hc,
                                        uint32_t Hn, bool has_c) {
    const int E = c.E, R = c.R, nE = c.nE, nR = c.nR, lane = c.lane, hh = c.hh;
    const int per = nE + nR, ntl = (5 * R) >> 5, nblk = R >> 5;
    const uint32_t AI_AT = c.P_AT, AH_AT = AI_AT + WD_WIN_BYTES * (uint32_t)(5 * nR),
                   O_AT = AH_AT + WD_WIN_BYTES * (uint32_t)(5 * nR);
    // ---- (a) the gate tiles, rows 32 q .. + 31 of the [5R] pre-activations: E / 128 windows over x, R / 128 over h_t
    float si = 0.f, sh = 0.f;
    {
        f32x16 ai, ah;
        wide_run_tiles(c, ntl * per,
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
                               wide_store_block(c.scr_r, AI_AT, q, lane, ai);
#pragma unroll
                               for (int r = 0; r < 16; ++r) si = si + ai[r];
                           }
                           if (wi == per - 1) {
                               wide_store_block(c.scr_r, AH_AT, q, lane, ah);
#pragma unroll
                               for (int r = 0; r < 16; ++r) sh = sh + ah[r];
                           }
                       });
    }
    // ---- (b) the statistics of the two chains over the row's 5R values (this lane's and lane ^ 32's) ----
    const float mi = nn_ln_mean(si, __shfl_xor(si, 32), 5 * R);
    const float mh = nn_ln_mean(sh, __shfl_xor(sh, 32), 5 * R);
    const float qi = ln_sumsq(c, AI_AT, ntl, mi);
    const float qh = ln_sumsq(c, AH_AT, ntl, mh);
    const float di = nn_ln_den(qi, __shfl_xor(qi, 32), 5 * R);
    const float dh = nn_ln_den(qh, __shfl_xor(qh, 32), 5 * R);
    // ---- (c) the fold, a 32-unit block at a time ----
    // gate chunk ch (i, f, o, g1, g2 = 0..4, nets.py:110-121) of block j: s = LN(i2h(x)) + LN(h2h(h))
    auto gate = [&](int ch, int j) __attribute__((always_inline)) {
        const int tq = ch * nblk + j;
        const f32x16 vi = wide_load_block(c.scr_r, AI_AT, tq, lane);
        const f32x16 vh = wide_load_block(c.scr_r, AH_AT, tq, lane);
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
        wide_store_block(c.scr_r, O_AT, j, lane, og);
    }
    // ---- (d) the statistic of c' over the row's R values, then h' = o * tanh(LN_c(c')) ----
    const float mc = nn_ln_mean(sc, __shfl_xor(sc, 32), R);
    const float qc = ln_sumsq(c, c.C_AT, nblk, mc);
    const float dc = nn_ln_den(qc, __shfl_xor(qc, 32), R);
#pragma unroll 1
    for (int j = 0; j < nblk; ++j) {
        const f32x16 cn = wide_load_block(c.scr_r, c.C_AT, j, lane);
        const f32x16 og = wide_load_block(c.scr_r, O_AT, j, lane);
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
    const WideCtx c = wide_decode_ctx(p, la.E, la.R, ln_extra_windows(la.R), lds);
    wide_decode(p, c, [&](uint32_t Hc, uint32_t Hn, bool has_c) __attribute__((always_inline)) {
        ln_cell(p, la, c, Hc, Hn, has_c);
    });
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
    const int xw = ln_extra_windows(la.R);
    const WideCtx c = wide_ctx(p, la.E, la.R, xw, 0, p.scratch + (size_t)wave * wide_wave_floats(la.E, la.R, xw), lds,
                               tid, sgn);
    auto spread = [&](const float* in, int n, uint32_t at) {
        for (int g = 0; g < n >> 3; ++g) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (ok) v = *reinterpret_cast<const f32x4*>(in + (size_t)row * n + wide_group_unit(g, hh));
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
            const size_t o = (size_t)row * la.R + wide_group_unit(g, hh);
            *reinterpret_cast<f32x4*>(hout + o) = ld4(c.scr_r, 16u * (uint32_t)lane, Hn + WD_GRP_BYTES * (uint32_t)g);
            *reinterpret_cast<f32x4*>(cout + o) = ld4(c.scr_r, 16u * (uint32_t)lane, c.C_AT + WD_GRP_BYTES * (uint32_t)g);
        }
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

// test entry (nicnes_test_ln_cell): p->noise holds D zeros, p->scratch one workgroup's lane scratch; rows <= 128
extern "C" hipError_t nicnes_launch_test_ln_cell(const DecodeParams* p, int E, int R, const int64_t* tail6,
                                                 const float* xin, const float* hin, const float* cin, int rows,
                                                 float* hout, float* cout, hipStream_t stream) {
    const LnArgs la = ln_args(E, R, tail6);
    if (!wide_dims_ok(E, R, ln_extra_windows(R)) || rows < 1 || rows > 128) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nicnes_test_ln_cell_kernel, dim3(1), dim3(NTHREADS), LDS32, stream, *p, la, xin, hin, cin, rows,
                       hout, cout);
    return hipGetLastError();
}
