// Internal (non-ABI) interface of the SM-G-SUM sensitivity (sensitivity.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct SensParams {
    const float* theta;          // fp32 theta [D] (flat order)
    const float* fc;             // [Bs, F] unique-image fc rows
    int32_t* tok;                // [Bs, tok_stride] greedy tokens of logit steps 1..L-1 (unmasked)
    int32_t tok_stride;
    int32_t tok_internal;        // 1: the forward picks them itself (argmax of its log_softmax) and writes tok
    int32_t Bs, V1, E, R, F;
    int32_t L;                   // greedy steps (forward_for_sensitivity length = 5)
    int32_t split;               // vocabulary group size (100)
    int32_t K;                   // groups = V1 / split + 1 (the zero padding always adds split - V1 % split)
    int64_t D;
    int64_t off_img_w, off_img_b, off_emb_w, off_log_w, off_log_b, off_i2h_w, off_i2h_b, off_h2h_w, off_h2h_b;
    float underflow;             // > 0: clamp + divide as calc_sensitivity; <= 0: the raw sensitivity
    float* out;                  // [D]
};

// L * Bs at most (the embedding kernels' pair list, sorted in LDS): 819 rows at L = 5. nicnes_sens_run returns 1 above it.
#define NICNES_SENS_MAX_PAIRS 4096

// The paths a run took (nicnes_sens_last_paths, out[0]): a set bit is the fast path of DESIGN.md section 8's table.
#define SENS_PATH_LOGIT_FAST 1     // logit.weight square sums on sens_logit_sq (else the tile kernel's sq mode on DzA)
#define SENS_PATH_BWD_FUSED 2      // dX / dH of the backward recurrence in one sens_bsq launch per cell (else two gemms)
#define SENS_PATH_GATES_BSQ 4      // gate and image weight square sums on sens_bsq (else the tile kernel's sq mode)
#define SENS_PATH_EMB_TWO_PASS 8   // embedding rows on sens_emb_part + sens_emb_fin (else sens_emb_sq over EMB_KC ranges)

struct SensWork;
extern "C" SensWork* nicnes_sens_create();
extern "C" void nicnes_sens_destroy(SensWork* w);
// 0 on success; the work buffers grow to the largest (Bs, K) seen (K x D floats for the gradients)
extern "C" int nicnes_sens_run(SensWork* w, const SensParams* p, hipStream_t stream);
// out = {SENS_PATH_* bits, gemm launches with 16-byte operand loads, gemm launches with scalar loads} of the last run that
// enqueued every kernel; 1 before the first such run (host bookkeeping only: no kernel, no synchronisation)
extern "C" int nicnes_sens_last_paths(const SensWork* w, int32_t out[3]);
