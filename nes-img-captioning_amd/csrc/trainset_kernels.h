// Internal (non-ABI) interface of the resident training set's gather kernels (trainset_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// out row r <- set row image_ix[r], r < n_rows; rows of F floats (F a multiple of 128: 16-byte pieces)
extern "C" hipError_t nicnes_launch_gather_fc(const float* set_fc, const int32_t* image_ix, int n_rows, int F, float* out,
                                              hipStream_t s);
// image i of the batch takes rows [set_start[image_ix[i]], + dst_start[i + 1] - dst_start[i]) of the set's reference
// rows (T int32 each) into out_refs rows [dst_start[i], ...); out_start [n_img + 1] <- dst_start
extern "C" hipError_t nicnes_launch_gather_refs(const int32_t* set_refs, const int32_t* set_start, const int32_t* image_ix,
                                                const int32_t* dst_start, int n_img, int T, int32_t* out_refs,
                                                int32_t* out_start, hipStream_t s);
