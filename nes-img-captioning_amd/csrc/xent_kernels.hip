// xent_kernels.hip -- the teacher-forced forward: log-probs of given label rows under theta +- delta (NICNES_FITNESS_XENT,
// nicnes_split_xent). DESIGN.md "Teacher-forced cross-entropy" has the definition (self-critical.pytorch's
// FCModel._forward + LanguageModelCriterion over the reference's modules).
// Not a translation unit of its own: decode_kernel.hip #includes this file behind decode_wide_kernels.hip and ahead of
// its last kernel (the Makefile lists it as a dependency), so the library keeps its five code objects and this file uses
// that unit's tile helpers (TileDesc, stage_load / stage_store through wide_run_tiles, bias_init, mfma_tile_fc, the exact
// branch of epilogue64) and, at E = R = 128, the wide frame's lane-scratch windows and its plain LSTM cell (wide_tile,
// wide_cell): every dense product is the transposed 32x32x2 fp32 MFMA chain in nn_kperm's k order, W0 +- delta formed
// once per staged element for both signs, in LDS only.
//
// One workgroup = one member (both signs) x one slab of <= 128 label rows; wave w = sign (w >> 2) x 32-row group (w & 3),
// as on the fused path. Against the greedy step loop:
//   - the next input token is the row's label (u_0 = BOS, u_s = w[s - 1]): no pick, no records, no tie rule, and the
//     exp-sum is always the exact one;
//   - during the logit sweep the lane that owns (row, w[s]) in the accumulator layout keeps that logit; the row's two
//     lane halves combine it after the last stage, beside the exp-sum;
//   - a row reads its image through the row -> image map (built from img_ref_start when the batch or split is set); the
//     image projection is done per row;
//   - the workgroup leaves the loop once every one of its rows is past its last target (a workgroup-uniform vote).
// Lane-private scratch only (x, h', c of the wide frame's windows: a lane reloads only what it stored), no workgroup
// waits for another, no spin loop; every buffer resource has its exact byte size, so an offset past an end reads zero.
//
// Rows. Batches (img_ref_start set): member k's rows are the label rows of its batch, grid (members, slabs of the
// largest batch); a slab past the batch's rows returns at once. A flat range (img_ref_start NULL: theta itself over the
// zero noise slice): pseudo-member k takes rows row0 + 256 k + (0..127) as its sign + and the next 128 as its sign -.
// grid (members, slabs)
__global__ __launch_bounds__(NTHREADS) void nicnes_xent_kernel(DecodeParams p, XentArgs xa) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), sgn = wave >> 2, grp = wave & 3;
    const int member = blockIdx.x, slab = blockIdx.y, wg = member * gridDim.y + slab;
    const int T = p.T, b = grp * 32 + (lane & 31);
    // ---- the lane's label row ----
    int first, left;                 // the workgroup's first row (always a row of the range), rows from the wave's sign on
    size_t orow;
    if (xa.img_ref_start) {
        const int k = p.member_batch ? p.member_batch[member] : 0;
        const int a = xa.img_ref_start[k * p.B_img], e = xa.img_ref_start[(k + 1) * p.B_img];
        first = a + slab * 128;
        if (first >= e) return;      // the whole workgroup: this batch has fewer slabs than the grid
        left = e - first;
        orow = ((size_t)member * 2 + sgn) * (size_t)xa.max_rows + (size_t)(slab * 128 + b);
    } else {
        first = xa.row0 + member * 256;
        left = xa.row1 - first - sgn * 128;
        orow = (size_t)(member * 256 + sgn * 128 + b);
    }
    const bool valid = b < left;
    const int grow = valid ? first + (xa.img_ref_start ? 0 : sgn * 128) + b : first;
    const int32_t* lab = xa.labels + (size_t)grow * T;
    int last = 0, ntok = 1;          // the last counted target; the counted targets (s = 0 always counts)
    for (int t = 0; t < T; ++t)
        if (valid && lab[t] > 0) {
            last = t + 1;
            ++ntok;
        }

    const WideCtx c = wide_ctx(p, 128, 128, 0, p.noise_idx[member],
                               p.scratch + ((size_t)wg * 8 + wave) * wide_wave_floats(128, 128, 0), lds, tid, sgn);
    const rsrc_t scr_r = c.scr_r;
    // ---- x of the image step: img_embed(fc) of the row's image (FCModel._sample t = 0); h = 0 ----
    {
        // rows ascend with their images and every image has a row: the workgroup's <= 256 rows lie in <= 256 images
        const int img_lo = __builtin_amdgcn_readfirstlane(xa.row_img[first]);
        const int img_n = min(256, xa.n_img - img_lo);
        const rsrc_t fc_r = make_rsrc(p.fc + (size_t)img_lo * p.F, 4u * (uint32_t)img_n * (uint32_t)p.F);
        const int fr = xa.row_img[grow] - img_lo;
        const int nK = p.F >> 7;
        f32x16 acc;
        wide_run_tiles(c, 4 * nK,
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
        f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
        for (int g = 0; g < 16; ++g) st4(scr_r, 16u * (uint32_t)lane, c.H_AT + WD_GRP_BYTES * (uint32_t)g, z4);
        // a 16-byte store reads its data registers after issue (gfx950): the asm keeps the zeros' registers unwritten
        // for two wait states behind the last store (tests/test_isa_hazards.py scans for this)
        asm volatile("s_nop 1" : "+v"(z4));
    }
    wide_cell(p, c, c.H_AT, c.H_AT + WD_WIN_BYTES, false);      // its logits are discarded
    int cur = 1;                                                // h is the h' copy of this parity

    const int nvt = 2 * ((p.V1 + 63) >> 6);                     // 32-row vocabulary tiles, two per 64-row stage
    double sum = 0.0;
#pragma unroll 1
    for (int s = 0; s <= T; ++s) {
        // ---- x = embed(u_s) (+- delta): BOS, or the label before the target; an id outside the vocabulary reads as 0 ----
        const int prev = s == 0 ? 0 : lab[s - 1];
        {
            const int u = (s > 0 && (uint32_t)prev < (uint32_t)p.V1) ? prev : 0;
            const uint32_t eo = 4u * ((uint32_t)p.off_emb_w + (uint32_t)u * 128u);
            for (int g = 0; g < 16; ++g) {
                const uint32_t ko = eo + 4u * (uint32_t)wide_group_unit(g, hh);
                const f32x4 w0 = ld4(c.theta_r, ko), delta = ld4(c.noise_r, ko);
                st4(scr_r, 16u * (uint32_t)lane, c.X_AT + WD_GRP_BYTES * (uint32_t)g, sgn ? (w0 - delta) : (w0 + delta));
            }
        }
        const uint32_t Hn = c.H_AT + WD_WIN_BYTES * (uint32_t)(cur ^ 1);
        wide_cell(p, c, c.H_AT + WD_WIN_BYTES * (uint32_t)cur, Hn, true);
        cur ^= 1;
        // ---- logits over h: the exact exp-sum, and the target's logit kept by the lane that owns it ----
        const int tgt = (s < T && valid) ? lab[s] : 0;
        const bool own = ((tgt >> 2) & 1) == hh;
        const int tv = own ? (tgt >> 5) : -1, tr = (tgt & 3) + 4 * ((tgt & 31) >> 3);
        float xt = NEG_INF;
        RowState st;
        row_state_init(st);
        f32x16 acc, P0;
        wide_run_tiles(c, nvt,
                       [&](int n) {
                           TileDesc d;
                           d.w_off = (uint32_t)p.off_log_w; d.ld = 128; d.row0 = 32 * n; d.nvalid = min(32, max(p.V1 - 32 * n, 0));
                           d.k0 = 0; d.b_off = (uint32_t)p.off_log_b; d.pad_bias = NEG_INF;
                           return d;
                       },
                       [&](int n, const float* wt, const float* bias) __attribute__((always_inline)) {
                           acc = bias_init(bias, hh);
                           acc = wide_tile(acc, wt, scr_r, Hn, lane);
                           if (__any(n == tv)) {
#pragma unroll
                               for (int r = 0; r < 16; ++r) xt = (n == tv && r == tr) ? acc[r] : xt;
                           }
                           if (n & 1) epilogue64<false>(st, P0, acc, 32 * (n - 1) + 4 * hh);
                           else P0 = acc;
                       });
        const float m_o = __shfl_xor(st.m, 32), s_o = __shfl_xor(st.s, 32), x_o = __shfl_xor(xt, 32);
        const float m = fmaxf(st.m, m_o);
        const float stot = st.s * __builtin_amdgcn_exp2f((st.m - m) * LOG2E) + s_o * __builtin_amdgcn_exp2f((m_o - m) * LOG2E);
        const float lse = logf(stot);
        const float lp = ((own ? xt : x_o) - m) - lse;
        if (valid && (s == 0 || prev > 0)) {                    // the words plus one end token
            sum += (double)lp;
            if (hh == 0 && xa.lp_steps) xa.lp_steps[orow * (size_t)(T + 1) + s] = lp;
        }
        if (!__syncthreads_or((valid && s < last) ? 1 : 0)) break;
    }
    if (valid && hh == 0) {
        xa.lp_sum[orow] = sum;
        xa.n_tok[orow] = ntok;
    }
}

// loss of a candidate's rows: both sums in a fixed order in fp64 (thread i takes rows i, i + 256, .. in order, then a
// pairwise tree over the 256 partials), no atomics: the same rows give the same bits. One workgroup per candidate
// (member, sign), or the one flat range; fitness (nullable) = sum lp_sum / sum n_tok = -loss.
__global__ __launch_bounds__(256) void nicnes_xent_reduce_kernel(XentArgs xa, const int32_t* member_batch, int B_img,
                                                                 double* fitness, long long* tokens, double* loss2) {
    __shared__ double sl[256];
    __shared__ long long sn[256];
    const int cand = blockIdx.x, tid = threadIdx.x;
    int rows;
    size_t base;
    if (xa.img_ref_start) {
        const int k = member_batch ? member_batch[cand >> 1] : 0;
        rows = xa.img_ref_start[(k + 1) * B_img] - xa.img_ref_start[k * B_img];
        base = (size_t)cand * (size_t)xa.max_rows;
    } else {
        rows = xa.row1 - xa.row0;
        base = 0;
    }
    double a = 0.0;
    long long n = 0;
    for (int r = tid; r < rows; r += 256) {
        a += xa.lp_sum[base + r];
        n += xa.n_tok[base + r];
    }
    sl[tid] = a;
    sn[tid] = n;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            sl[tid] += sl[tid + w];
            sn[tid] += sn[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (fitness) fitness[cand] = sl[0] / (double)sn[0];
        if (tokens) tokens[cand] = sn[0];
        if (loss2) {                 // the flat range: loss and perplexity
            const double loss = -(sl[0] / (double)sn[0]);
            loss2[0] = loss;
            loss2[1] = exp(loss);
        }
    }
}

// row -> image map of label rows laid out image by image (img_ref_start [n_img + 1])
__global__ __launch_bounds__(256) void nicnes_xent_row_map_kernel(const int32_t* img_ref_start, int n_img, int32_t* row_img) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_img) return;
    for (int r = img_ref_start[i]; r < img_ref_start[i + 1]; ++r) row_img[r] = i;
}

// ========== host side ===================================================================================================
extern "C" size_t nicnes_xent_scratch_floats(int64_t workgroups) {
    return (size_t)workgroups * 8 * wide_wave_floats(128, 128, 0);
}

// per device, once per handle: the kernel's dynamic LDS is above 64 KB
extern "C" hipError_t nicnes_xent_init() {
    return hipFuncSetAttribute((const void*)nicnes_xent_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS32);
}

extern "C" hipError_t nicnes_launch_xent_row_map(const int32_t* img_ref_start, int n_img, int32_t* row_img, hipStream_t s) {
    if (n_img < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nicnes_xent_row_map_kernel, dim3((unsigned)((n_img + 255) / 256)), dim3(256), 0, s, img_ref_start,
                       n_img, row_img);
    return hipGetLastError();
}

// The forced-token forward of `members` members x nslabs slabs (batches), or of members pseudo-members of the flat
// range (nslabs 1), then the candidates' fitness (n_cand of them: 2 members, or 1). Reads theta, noise, noise_idx, fc,
// member_batch, B_img, scratch (nicnes_xent_scratch_floats(members * nslabs)), F, V1, T, D and the offsets of *p.
extern "C" hipError_t nicnes_launch_xent(const DecodeParams* p, const XentArgs* xent_args, int members, int nslabs,
                                         int n_cand, double* fitness, long long* tokens, double* loss2, hipStream_t s) {
    const XentArgs& xa = *xent_args;
    if (members < 1 || nslabs < 1 || n_cand < 1 || (!xa.img_ref_start && (nslabs != 1 || xa.row1 <= xa.row0)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(nicnes_xent_kernel, dim3(members, nslabs), dim3(NTHREADS), LDS32, s, *p, xa);
    hipLaunchKernelGGL(nicnes_xent_reduce_kernel, dim3(n_cand), dim3(256), 0, s, xa, p->member_batch, p->B_img, fitness,
                       tokens, loss2);
    return hipGetLastError();
}
