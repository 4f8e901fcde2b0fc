/*
 * nicnes_math.h -- the engine's elementwise-math and indexing contract.
 *
 * Every function here is compiled twice: by hipcc for the gfx950 kernels and by
 * gcc for the CPU oracle (oracle/). Both builds use -ffp-contract=off and only
 * IEEE-exact primitives (fmaf, +, -, *, /, floorf, bit casts), so a given input
 * produces the same bits on the GPU and on the host. That is what makes the
 * GPU-vs-oracle greedy-token comparison bit-exact.
 *
 * What the reference uses instead (and why it is only margin-comparable):
 *   LSTMCore.forward  src/captioning/nets.py:98-134   torch.sigmoid / torch.tanh (Sleef, CPU)
 *   PolicyNet.evolve  src/algorithm/nets.py:101-113   torch.normal_ (global RNG; replaced by the
 *                                                     noise table + index rule below)
 */
#ifndef NICNES_MATH_H
#define NICNES_MATH_H

#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#define NN_FN __host__ __device__ static inline
#else
#define NN_FN static inline
#endif

/* ---- bit casts (union punning works in C and in clang/gcc C++) ---------------------- */
NN_FN float nn_i2f(int32_t i) { union { int32_t i; float f; } u; u.i = i; return u.f; }
NN_FN int32_t nn_f2i(float f) { union { int32_t i; float f; } u; u.f = f; return u.i; }

NN_FN float nn_floorf(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_floorf(x);
#else
    return __builtin_floorf(x);
#endif
}

/* 2^n as a float for n in [-126, 127] */
NN_FN float nn_pow2i(int32_t n) { return nn_i2f((n + 127) << 23); }

/*
 * nn_expf: e^x, <= ~1 ulp on the range the hot path uses. Cody-Waite reduction x = n ln2 + r,
 * |r| <= ln2/2, degree-7 Taylor in Horner form with fmaf, one scale by 2^n. The argument is
 * clamped to [-87, 88] so the scale stays a normal power of two (below -87 the result is e^-87
 * instead of a subnormal or 0: every caller adds it to 1 or multiplies a bounded value by it);
 * above 88.72 the result is +inf and NaN passes through. Branch-free (one instruction stream for
 * every lane of a wavefront).
 */
NN_FN float nn_expf_core(float xc) {                   /* xc in [-87, 88], not NaN */
    const float log2e = 1.44269502162933349609375f;
    const float ln2_hi = 0.693145751953125f;          /* 12 significant bits: n*ln2_hi exact */
    const float ln2_lo = 1.428606765330187045e-06f;
    float n = nn_floorf(xc * log2e + 0.5f);
    float r = fmaf(-n, ln2_hi, xc);
    r = fmaf(-n, ln2_lo, r);
    float p = 1.98412701138295233250e-4f;             /* 1/7! */
    p = fmaf(p, r, 1.38888892251998186111e-3f);       /* 1/6! */
    p = fmaf(p, r, 8.33333376795053482056e-3f);       /* 1/5! */
    p = fmaf(p, r, 4.16666679084300994873e-2f);       /* 1/4! */
    p = fmaf(p, r, 1.66666671633720397949e-1f);       /* 1/3! */
    p = fmaf(p, r, 0.5f);
    p = fmaf(p, r, 1.0f);
    p = fmaf(p, r, 1.0f);
    return p * nn_pow2i((int32_t)n);                  /* n in [-126, 127] */
}

NN_FN float nn_expf(float x) {
    const float xc = fminf(fmaxf(x, -87.0f), 88.0f);  /* NaN -> -87 (replaced below) */
    float y = nn_expf_core(xc);
    y = x > 88.72283935546875f ? nn_i2f(0x7f800000) : y;
    return x != x ? x : y;
}

/*
 * nn_rcp1f: 1/d for d in [1, 2^120], <= ~1 ulp: integer first guess (relative error < 12.5 %) and
 * three Newton steps e = 1 - d y, y += y e in fmaf (error squares each step: 1.6e-2, 2.4e-4,
 * 5.9e-8 before the last rounding). Deterministic IEEE operations only, so host and GPU agree.
 */
NN_FN float nn_rcp1f(float d) {
    float y = nn_i2f(0x7EF311C3 - nn_f2i(d));
    float e = fmaf(-d, y, 1.0f);
    y = fmaf(y, e, y);
    e = fmaf(-d, y, 1.0f);
    y = fmaf(y, e, y);
    e = fmaf(-d, y, 1.0f);
    return fmaf(y, e, y);
}

/* sigmoid as torch.sigmoid defines it (src/captioning/nets.py:117): 1 / (1 + e^-x); the argument is
 * clamped to [-80, 80] (sigmoid there is 1 - 2^-115 .. 2^-115 off its limit) so 1 + e^-x stays in the
 * reciprocal's range */
NN_FN float nn_sigmoidf(float x) {
    const float xc = fminf(fmaxf(x, -80.0f), 80.0f);   /* NaN -> -80 (replaced below) */
    const float y = nn_rcp1f(1.0f + nn_expf_core(-xc)); /* = nn_expf(-xc): -xc is in range */
    return x != x ? x : y;
}

/*
 * nn_tanhf: odd; |x| < 0.6 -> x * P(x^2) (least-squares fit of tanh(x)/x in double,
 * abs err 3.6e-10 before fp32 rounding), else 1 - 2/(e^{2|x|} + 1) (exactly 1 past 9.5).
 * Both branches are evaluated and one is selected (branch-free, as nn_expf).
 */
NN_FN float nn_tanhf(float x) {
    const float a = x < 0.0f ? -x : x;
    const float u = x * x;
    float p = 0.0022306744940578938f;
    p = fmaf(p, u, -0.008266338147222996f);
    p = fmaf(p, u, 0.021733924746513367f);
    p = fmaf(p, u, -0.05395231395959854f);
    p = fmaf(p, u, 0.13333244621753693f);
    p = fmaf(p, u, -0.3333333134651184f);
    p = fmaf(p, u, 1.0f);
    const float small = x * p;
    const float ac = fminf(a, 9.5f);                  /* e^19 + 1 < 2^28: in the reciprocal's range; */
    float y = 1.0f - 2.0f * nn_rcp1f(nn_expf_core(2.0f * ac) + 1.0f);   /* NaN -> 9.5, replaced below */
    /* past 9.5 the formula already gives exactly 1: 2 / (e^19 + 1) < ulp(1) / 2 below 1 */
    y = x < 0.0f ? -y : y;
    y = a < 0.6f ? small : y;
    return x != x ? x : y;
}

/*
 * LSTM cell element (src/captioning/nets.py:113-132 with vbn=layer_n=false):
 *   c' = f*c + i*max(g1,g2) ; h' = o * tanh(c')      (each product/sum rounded separately)
 * s_* are the pre-activation gate sums.
 */
NN_FN void nn_lstm_cell(float s_in, float s_forget, float s_out, float s_g1, float s_g2,
                        float c, float* c_new, float* h_new) {
    float ig = nn_sigmoidf(s_in);
    float fg = nn_sigmoidf(s_forget);
    float og = nn_sigmoidf(s_out);
    float g = s_g1 > s_g2 ? s_g1 : s_g2;     /* torch.max(a, b): NaN-free inputs */
    float fc = fg * c;                       /* both builds use -ffp-contract=off: the two */
    float igv = ig * g;                      /* products stay unfused, as in torch         */
    float cn = fc + igv;
    *c_new = cn;
    *h_new = og * nn_tanhf(cn);
}

/*
 * Layer norm of the N values of one batch row (nn.LayerNorm, src/captioning/nets.py:94-96: biased variance,
 * eps = 1e-5). In the 32x32 accumulator layout the row's values sit in two lanes, each holding the units it produced
 * (lane half hh owns unit u when ((u >> 2) & 1) == hh), and each lane sums its own values sequentially in ascending
 * unit order. A statistic is then finished from the two lane sums:
 *   mean = (sum_a + sum_b) / (float)N;   d = a - mean;   den = sqrtf((sumsq_a + sumsq_b) / (float)N + 1e-5f)
 * where sumsq is the lane's sequential sum of d * d in the same order (two passes: never E[x^2] - mean^2), and
 *   y = d / den,   with affine  y * gamma + beta  (a rounded product, then a rounded sum).
 * Only +, -, *, / and sqrtf, each IEEE-rounded and unfused (-ffp-contract=off), so host and GPU agree bit for bit.
 */
#define NN_LN_EPS 1e-5f
NN_FN float nn_ln_mean(float sum_a, float sum_b, int n) { return (sum_a + sum_b) / (float)n; }
NN_FN float nn_ln_sq(float acc, float a, float mean) {   /* one term of the centred second pass */
    const float d = a - mean;
    const float dd = d * d;
    return acc + dd;
}
NN_FN float nn_ln_den(float sumsq_a, float sumsq_b, int n) {
    const float var = (sumsq_a + sumsq_b) / (float)n;
    return sqrtf(var + NN_LN_EPS);
}
NN_FN float nn_ln_y(float a, float mean, float den) { return (a - mean) / den; }
NN_FN float nn_ln_affine(float y, float gamma, float beta) {
    const float t = y * gamma;
    return t + beta;
}

/*
 * LSTM cell element with layer_n (src/captioning/nets.py:102-130), in two halves around the row statistic of c':
 *   c' = f*c + i*max(g1,g2)  from the gate sums s = LN(i2h(x)) + LN(h2h(h)); c' is the state, un-normalised;
 *   h' = o * tanh(LN_c(c'))  with og = sigmoid(s_out) formed in the first half.
 */
NN_FN float nn_lstm_cell_ln_c(float s_in, float s_forget, float s_g1, float s_g2, float c) {
    const float ig = nn_sigmoidf(s_in);
    const float fg = nn_sigmoidf(s_forget);
    const float g = s_g1 > s_g2 ? s_g1 : s_g2;
    const float fc = fg * c;
    const float igv = ig * g;
    return fc + igv;
}
NN_FN float nn_lstm_cell_ln_h(float og, float c_normed) { return og * nn_tanhf(c_normed); }

/* ---- noise-table index rule (the contract that replaces shipping 11 MB noise vectors,
 *      src/algorithm/nic_nes/nic_nes_worker.py:156-161) ---------------------------------- */
NN_FN uint64_t nn_splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

#define NN_NOISE_ALIGN 64u   /* slice starts are multiples of 64 floats (256 B) */

/* idx = 64 * (splitmix64(seed ^ (iter<<32 | member)) mod n_slots), n_slots = floor((T-D)/64)+1 */
NN_FN uint64_t nn_noise_index(uint64_t seed, uint64_t iteration, uint64_t member,
                              uint64_t table_len, uint64_t dim) {
    uint64_t n_slots = (table_len - dim) / NN_NOISE_ALIGN + 1u;
    uint64_t h = nn_splitmix64(seed ^ ((iteration << 32) | (member & 0xffffffffull)));
    return (h % n_slots) * NN_NOISE_ALIGN;
}

/* ---- nic_es over ranks: the balanced split of a generation's n_pairs pairs (n_pairs >= world). The first
 *      n_pairs % world ranks take n_pairs / world + 1 pairs, the rest n_pairs / world; shards are contiguous and in
 *      rank order (the reference hands ESTasks to whichever worker is free, nic_es_master.py:68-90). */
NN_FN void nn_es_shard(int n_pairs, int rank, int world, int* begin, int* count) {
    const int q = n_pairs / world, r = n_pairs % world;
    *begin = rank * q + (rank < r ? rank : r);
    *count = q + (rank < r ? 1 : 0);
}

/*
 * Dot-product order ("k permutation"). The engine's dense products are fp32 fma chains
 * acc = fmaf(w[k], x[k], acc) started from the bias, visiting k in this order inside each
 * 32-wide chunk: for j = 0..15: k0 = (j&3) + 8*(j>>2), then k0 + 4.  It is the order in
 * which v_mfma_f32_32x32x2_f32 consumes an operand held in the 32x32 accumulator layout
 * (half 0 lanes: rows (r&3)+8(r>>2), half 1 lanes: +4), so the GPU needs no transpose.
 */
NN_FN int nn_kperm(int pos) {
    int chunk = pos >> 5, w = pos & 31, j = w >> 1, half = w & 1;
    return (chunk << 5) + (j & 3) + 8 * (j >> 2) + 4 * half;
}

/*
 * Screening bound ("bf16 screening"). A logit L is the fp32 chain above over w = fp32(W0 +/- delta),
 * h and the bias b. A screened logit l~ is the same sum taken by a bf16 MFMA: both operands rounded to bf16 (RNE,
 * unit roundoff 2^-8), products accumulated in fp32 from b in an order the hardware does not document.
 * nn_screen_eps bounds |l~ - L| for every row of a (member, sign) from three numbers: hnorm >= ||h||_2,
 * wnorm >= max_v ||w_v||_2, babs >= max_v |b_v|. With P = hnorm * wnorm >= sum_k |w_k h_k| (Cauchy-Schwarz):
 *   operand roundings   ((1 + 2^-8)^2 - 1) P = (2^-7 + 2^-16) P, taken as (2^-7 + 2^-15) P;
 *   accumulations       the MFMA's 128 products + bias, each add truncated (2^-23 of the partial sum, partial
 *                       sums <= |b| + (1 + 2^-7 + 2^-16) P): < 2^-15.9 (babs + P); the fp32 chain's 128 roundings
 *                       against the real sum: 2^-17 (babs + P); together < 2^-15.5 (babs + P), taken as 2^-13;
 *   subnormals          bf16 rounds a subnormal absolutely (2^-134), products and flushed operands lose at most
 *                       2^-126 each: < 2^-119 (1 + hnorm + wnorm), taken as 2^-116.
 * scale >= 1 widens the two relative terms (a test hook). A non-finite result sends the row to the exact pass.
 */
NN_FN float nn_screen_eps(float hnorm, float wnorm, float babs, float scale) {
    const float P = hnorm * wnorm;
    const float rel = 0.0078430175781250f * P + 0.0001220703125f * (babs + P);   /* 2^-7 + 2^-15, 2^-13 */
    return scale * rel + nn_pow2i(-116) * (1.0f + hnorm + wnorm);
}

/*
 * nn_screen_norm: an upper bound of ||x||_2 from the fp32 sum of squares ss (any summation order: n - 1 roundings
 * of non-negative terms, n <= 128, halve under the root; 2^-16 covers them, the root's and the roundings inside
 * nn_screen_eps) plus 2^-58 for squares that underflowed (below 2^-126 they may be flushed: 128 of them are less
 * than 2^-119 of ss, 2^-59.5 of the root).
 */
NN_FN float nn_screen_norm(float ss) { return sqrtf(ss) * 1.0000152587890625f + nn_pow2i(-58); }

#endif /* NICNES_MATH_H */
