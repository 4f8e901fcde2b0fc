// The body of nicnes_screen_norm_kernel (decode_kernel.hip), included where `p` (DecodeParams), `sa` (ScreenArgs) and
// `red` (__shared__ float [4][8]) are in scope: once per __global__ entry (see decode_img64_body.inc).
    const int tid = threadIdx.x, q = tid & 31, member = blockIdx.x;
    const uint64_t nidx = p.noise_idx[member];
    const rsrc_t w_r = make_rsrc(p.theta + p.off_log_w, 4u * 128u * (uint32_t)p.V1);
    const rsrc_t z_r = make_rsrc(p.noise + nidx + p.off_log_w, 4u * 128u * (uint32_t)p.V1);
    const rsrc_t b_r = make_rsrc(p.theta + p.off_log_b, 4u * (uint32_t)p.V1);
    const rsrc_t bz_r = make_rsrc(p.noise + nidx + p.off_log_b, 4u * (uint32_t)p.V1);
    float m[4] = {0.f, 0.f, 0.f, 0.f};
    auto upd = [](float& mx, float x) { mx = (x > mx || x != x) ? x : mx; };
    for (int v = tid >> 5; v < p.V1; v += NTHREADS / 32) {
        const uint32_t off = 4u * (uint32_t)(128 * v + 4 * q);
        const f32x4 w = ld4(w_r, off), z = ld4(z_r, off);
        const f32x4 a = w + z, b = w - z;
        float ssp = 0.f, ssm = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            ssp += a[e] * a[e];
            ssm += b[e] * b[e];
        }
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) {
            ssp += __shfl_xor(ssp, d);
            ssm += __shfl_xor(ssm, d);
        }
        upd(m[0], ssp);
        upd(m[1], ssm);
    }
    for (int v = tid; v < p.V1; v += NTHREADS) {
        const float bw = ld1(b_r, 4u * (uint32_t)v), bz = ld1(bz_r, 4u * (uint32_t)v);
        upd(m[2], fabsf(bw + bz));
        upd(m[3], fabsf(bw - bz));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) upd(m[i], __shfl_xor(m[i], d));
        if ((tid & 63) == 0) red[i][tid >> 6] = m[i];
    }
    __syncthreads();
    if (tid < 4) {
        float r = red[tid][0];
        for (int w = 1; w < 8; ++w) upd(r, red[tid][w]);
        sa.norm[4 * member + tid] = r;
    }
