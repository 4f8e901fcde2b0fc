// The body of nicnes_decode_img_kernel<G> (decode_kernel.hip), included where `G` (row groups per slab), `p`
// (DecodeParams) and `lds` (the dynamic LDS) are in scope: once per __global__ entry, so that an entry added beside it
// leaves its machine code as it was.
    const SCtx<G> c = make_sctx<G>(p);
    const bool fused_path = G == 4 && p.S == 1;
    if (fused_path) PROF_MARK(80); else PROF_SPLIT(250);
    const float* fcm = p.fc + (p.member_batch ? (size_t)p.member_batch[c.member] * p.B_img * p.F : 0);
    const rsrc_t fc_r = make_rsrc(fcm, 4u * (uint32_t)p.B_img * (uint32_t)p.F);
    const int fr = c.row_valid ? (c.b + c.sgn * p.sign_off) / p.rpi : 0;      // the lane's fc row (its image)
    const uint32_t lo = 4u * c.lane;
    const bool mm = G == 4 || c.hf == 0;
    StageRegs sr;
    f32x16 accU[4];
    const int nK = p.F >> 7;
    const int nb = 4 / (int)gridDim.x, U0 = nb * c.q;
    const int ntile = nK * nb;
    auto desc = [&](int n) {
        TileDesc d;
        d.w_off = (uint32_t)p.off_img_w; d.ld = p.F; d.row0 = 32 * (U0 + n % nb); d.nvalid = 32; d.k0 = 128 * (n / nb);
        d.b_off = (uint32_t)p.off_img_b; d.pad_bias = 0.f;
        return d;
    };
    stage_load(c.theta_r, c.noise_r, desc(0), c.tid, sr);
    stage_store(lds, desc(0), c.tid, sr);
    __syncthreads();
    for (int kc = 0; kc < nK; ++kc) {
        const uint32_t frow = 4u * (uint32_t)(fr * p.F + 128 * kc + 4 * c.hh);
#pragma unroll
        for (int U = 0; U < 4; ++U) {
            if (U < nb) {
                const int n = kc * nb + U;
                if (n + 1 < ntile) stage_load(c.theta_r, c.noise_r, desc(n + 1), c.tid, sr);
                const float* buf = lds + (n & 1) * STAGE_FLOATS;
                if (mm) {
                    if (kc == 0) accU[U] = bias_init(buf + 2 * SIGN_FLOATS + 32 * c.sgn, c.hh);
                    accU[U] = mfma_tile_fc(accU[U], buf + c.sgn * SIGN_FLOATS, fc_r, frow, c.lane);
                }
                if (n + 1 < ntile) stage_store(lds + ((n + 1) & 1) * STAGE_FLOATS, desc(n + 1), c.tid, sr);
                __syncthreads();
            }
        }
    }
    if (mm) {
#pragma unroll
        for (int U = 0; U < 4; ++U)
            if (U < nb) {
#pragma unroll
                for (int r = 0; r < 16; ++r) st1(c.scr_r, lo, X_SLOT(16 * (U0 + U) + r), accU[U][r]);
            }
        st1(c.scr_r, lo, U_SLOT, 1.0f);
    }
    if (c.q == 0 && c.tid == 0) p.alive[c.wg] = 1;
    if (fused_path) PROF_MARK(81); else PROF_SPLIT(251);
