// trainset_kernels.hip -- the resident training set's draw (nicnes_draw_batches): two gathers by image index from the
// set's buffers into the handle's batch buffers. Plain copies; everything downstream of them (reference cooking, image
// tables, decode) is the code nicnes_set_batches runs.
// Not a translation unit of its own: engine.cpp #includes this file (the Makefile lists it as a dependency), so the
// library's code objects stay the five that tests/test_isa_hazards.py counts.
#include "trainset_kernels.h"

#define GATHER_WAVES 4     // rows per workgroup: one wave per destination row
#define GATHER_PIECES 8    // 16-byte pieces per lane in flight (a 2048-float row is 8 per lane: the whole row at once)

// Batch row r <- set row image_ix[r]. One wave per row, so the source row index is wave-uniform (one scalar load) and
// every wave-instruction moves 1 KiB of one row; F4 = F / 4 is a multiple of 32.
__global__ __launch_bounds__(64 * GATHER_WAVES) void nicnes_gather_fc_kernel(const float4* __restrict__ set_fc,
                                                                              const int32_t* __restrict__ image_ix,
                                                                              int n_rows, int F4,
                                                                              float4* __restrict__ out) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    const int r = (int)blockIdx.x * GATHER_WAVES + wave;
    if (r >= n_rows) return;
    const float4* __restrict__ src = set_fc + (size_t)image_ix[r] * (size_t)F4;
    float4* __restrict__ dst = out + (size_t)r * (size_t)F4;
    int c = 0;      // wave-uniform piece base
    // whole groups of GATHER_PIECES wave-wide pieces: every load issued before the first store
    for (; c + 64 * GATHER_PIECES <= F4; c += 64 * GATHER_PIECES) {
        float4 v[GATHER_PIECES];
#pragma unroll
        for (int u = 0; u < GATHER_PIECES; ++u) v[u] = src[c + 64 * u + lane];
#pragma unroll
        for (int u = 0; u < GATHER_PIECES; ++u) dst[c + 64 * u + lane] = v[u];
    }
    // the rest of the row (fewer than GATHER_PIECES pieces; the last may be half a wave wide)
    for (int k = c + lane; k < F4; k += 64) dst[k] = src[k];
}

// Image i's reference rows, and the batch's img_ref_start. One wave per image; rows of T int32 are not 16-byte
// aligned in general (T = 7: 28 bytes), so the copy runs dword by dword over the image's count * T contiguous words.
__global__ __launch_bounds__(64) void nicnes_gather_refs_kernel(const int32_t* __restrict__ set_refs,
                                                                const int32_t* __restrict__ set_start,
                                                                const int32_t* __restrict__ image_ix,
                                                                const int32_t* __restrict__ dst_start, int n_img, int T,
                                                                int32_t* __restrict__ out_refs,
                                                                int32_t* __restrict__ out_start) {
    const int i = (int)blockIdx.x;
    if (i >= n_img) return;
    const int d0 = dst_start[i], d1 = dst_start[i + 1];
    const int32_t* __restrict__ src = set_refs + (size_t)set_start[image_ix[i]] * (size_t)T;
    int32_t* __restrict__ dst = out_refs + (size_t)d0 * (size_t)T;
    const int words = (d1 - d0) * T;
    for (int w = (int)threadIdx.x; w < words; w += 64) dst[w] = src[w];
    if (threadIdx.x == 0) {
        out_start[i] = d0;
        if (i == n_img - 1) out_start[n_img] = d1;
    }
}

extern "C" hipError_t nicnes_launch_gather_fc(const float* set_fc, const int32_t* image_ix, int n_rows, int F, float* out,
                                              hipStream_t s) {
    if (n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(nicnes_gather_fc_kernel, dim3((unsigned)((n_rows + GATHER_WAVES - 1) / GATHER_WAVES)),
                       dim3(64 * GATHER_WAVES), 0, s, (const float4*)set_fc, image_ix, n_rows, F / 4, (float4*)out);
    return hipGetLastError();
}

extern "C" hipError_t nicnes_launch_gather_refs(const int32_t* set_refs, const int32_t* set_start, const int32_t* image_ix,
                                                const int32_t* dst_start, int n_img, int T, int32_t* out_refs,
                                                int32_t* out_start, hipStream_t s) {
    if (n_img <= 0) return hipSuccess;
    hipLaunchKernelGGL(nicnes_gather_refs_kernel, dim3((unsigned)n_img), dim3(64), 0, s, set_refs, set_start, image_ix,
                       dst_start, n_img, T, out_refs, out_start);
    return hipGetLastError();
}
