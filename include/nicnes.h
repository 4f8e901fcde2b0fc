/*
 * nicnes.h -- C ABI of the MI355X NIC-NES population-evaluation engine (libnicnes.so).
 *
 * Plain C: status codes, raw pointers and sizes, no torch types. All array arguments are
 * DEVICE pointers on the handle's GPU unless the name ends in _host. `stream` is a
 * hipStream_t (NULL = the default stream); every call only enqueues work on it, except the
 * functions documented as synchronising. A handle is not thread-safe: one owner thread per
 * handle, one handle per GPU. Buffers passed to nicnes_set_* are borrowed (the caller keeps
 * them alive and unchanged until the handle is destroyed or the buffer is replaced); output
 * buffers are written by the enqueued work.
 *
 * Each entry point names the reference interface (rubencart/NES-img-captioning, file:line) it
 * replaces. Integration stubs for the reference side: INTEGRATION.md.
 */
#ifndef NICNES_H
#define NICNES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NICNES_OK 0
#define NICNES_ERR_INVALID 1       /* bad argument / wrong state */
#define NICNES_ERR_UNSUPPORTED 2   /* experiment option the engine does not implement */
#define NICNES_ERR_HIP 3           /* HIP runtime error (message in nicnes_last_error) */
#define NICNES_ERR_NOMEM 4
#define NICNES_ERR_FAULT 5         /* contained decode fault: NaN fitness, the optimizer step skipped (nicnes_stats) */

typedef struct nicnes_handle nicnes_handle;

/* Filled from the experiment JSON (src/algorithm/policies.py:31-41 ModelOptions,
 * src/captioning/experiment.py:27-30 vocab injection, src/algorithm/tools/utils.py:14-20 Config). */
typedef struct nicnes_config {
    int32_t vocab_size;           /* V; logits are V + 1 wide (src/captioning/nets.py:151-152) */
    int32_t input_encoding_size;  /* E: 128, 256, 384 or 512 */
    int32_t rnn_size;             /* R: 128, 256, 384 or 512, independently of E. A model with E or R above 128 is
                                   * "wide": every greedy decode (nicnes_evaluate*, nicnes_evaluate_theta,
                                   * nicnes_split_decode / _evaluate, with the materialised mutations) runs on the wide
                                   * path (nicnes_decode_path 3: 128-row slabs, one launch, one stream, the exact
                                   * exp-sum); the sampled fitness modes, nicnes_sum_sensitivity, nicnes_es_create (all
                                   * of nic_es), the beam decode, nicnes_test_logit_chain / _certify_items, a forced
                                   * split shape (nicnes_set_decode_split with S > 1 or G = 2) and more than one decode
                                   * stream return NICNES_ERR_UNSUPPORTED there. Test hook NICNES_DECODE_WIDE=1 (read
                                   * at create): E = R = 128 takes the wide path too */
    int32_t fc_feat_size;         /* F (multiple of 128) */
    int32_t seq_length;           /* 16 (src/captioning/nets.py:147) */
    int32_t max_batch;            /* max unique images per batch (config.batch_size) */
    int32_t max_refs;             /* max reference captions per batch */
    int32_t max_members;          /* max population members per nicnes_evaluate call */
    uint64_t noise_len;           /* entries of the shared Gaussian table */
    uint64_t noise_seed;          /* seed of the member -> table-offset rule */
    int32_t layer_n;              /* model_options.layer_n: LSTMCore with nn.LayerNorm on i2h(x), h2h(h) (each over 5R) and
                                   * on next_c (over R) in front of the tanh (src/captioning/nets.py:92-96,102-104,
                                   * 126-127). At every supported width such a handle decodes on the layer-norm path
                                   * (nicnes_decode_path 4): the wide path's shape and rules (128-row slabs, one launch,
                                   * one stream, the exact exp-sum, materialised mutations) on a kernel whose cell forms the
                                   * row statistics, and it ignores or refuses what a wide handle ignores or refuses
                                   * (see rnn_size above). 0: no normalisation */
    int32_t layer_n_affine;       /* model_options.layer_n_affine: the three LayerNorms carry weight and bias; theta
                                   * then holds six more tensors behind the nine (nicnes_param_offsets_ln), perturbed,
                                   * mutated and optimised like every other entry. Ignored without layer_n, as the
                                   * reference ignores it */
} nicnes_config;

/* flat parameter count D for a config (src/algorithm/nets.py:146-148 count_parameters) */
int64_t nicnes_param_count(const nicnes_config* cfg);
/* offsets of the 9 tensors in the flat theta (registration order) + D at [9] (with layer_n_affine D includes the six
 * layer-norm tensors behind them, so [9] is then the end of theta and not of core.h2h.bias) */
int nicnes_param_offsets(const nicnes_config* cfg, int64_t* out10_host);
/* layer_n with layer_n_affine: offsets of core.i2h_ln.weight, .bias [5R], core.h2h_ln.weight, .bias [5R],
 * core.c_ln.weight, .bias [R] (the reference's registration order: they follow core.h2h.bias) + D at [6].
 * NICNES_ERR_INVALID on a config without both flags. */
int nicnes_param_offsets_ln(const nicnes_config* cfg, int64_t* out7_host);

int nicnes_create(const nicnes_config* cfg, int device, nicnes_handle** out);
int nicnes_destroy(nicnes_handle* h);
const char* nicnes_last_error(const nicnes_handle* h);

/* Shared noise table (borrowed), replaces the per-worker torch.normal_ draw of
 * PolicyNet.evolve, src/algorithm/nets.py:101-102. The engine keeps a sigma-scaled copy
 * fp32(sigma * table) for the decode (noise_len floats of device memory), rebuilt by the first
 * evaluation after this call or after a change of sigma; call again if the table's contents change. */
int nicnes_set_noise_table(nicnes_handle* h, const float* table, uint64_t len);

/* Current parameters (copied into the engine's fp64 master + fp32 evaluation copy), replaces
 * Policy.set_model / set_from_parameter_vector, src/algorithm/policies.py:106-147.
 * is_fp32_origin = 1 keeps the reference's fp32-theta semantics for the first Adam step. */
int nicnes_set_theta(nicnes_handle* h, const double* theta64, int is_fp32_origin, void* stream);
int nicnes_get_theta(nicnes_handle* h, double* theta64_out, float* theta32_out, void* stream);
/* Adam state in the reference layout (src/algorithm/nic_nes/optimizers.py:85-107): m, v, t */
int nicnes_set_adam_state(nicnes_handle* h, const double* m, const double* v, int64_t t, void* stream);
int nicnes_get_adam_state(nicnes_handle* h, double* m_out, double* v_out, int64_t* t_out_host, void* stream);

/* One batch (src/captioning/dataloader.py:135-203 get_batch, deduplicated to unique images):
 * fc [B, F] fp32; ref_tokens [n_refs, seq_length] int32 zero-padded label rows;
 * img_ref_start [B + 1] (refs of image b are [img_ref_start[b], img_ref_start[b+1])).
 * Builds the reference-side CIDEr-D vectors on `stream`. */
int nicnes_set_batch(nicnes_handle* h, const float* fc, int32_t B, const int32_t* ref_tokens, int32_t n_refs,
                     const int32_t* img_ref_start, void* stream);

/* Several batches at once, for per-member batches (single_batch: false in the experiment JSON: each
 * reference worker draws its own batch for every member, src/algorithm/nic_nes/nic_nes_worker.py:
 * 121-128). fc [n_batches * B, F]; batch g holds images g * B .. g * B + B - 1, whose references are
 * ranges of img_ref_start [n_batches * B + 1] as in nicnes_set_batch (= this call with n_batches 1). */
int nicnes_set_batches(nicnes_handle* h, const float* fc, int32_t n_batches, int32_t B, const int32_t* ref_tokens,
                       int32_t n_refs, const int32_t* img_ref_start, void* stream);

/* Fixed document-frequency table (CiderD(df='coco-train-idxs'), src/captioning/policies.py:72):
 * sorted packed n-gram keys (n<<56 | t0<<42 | t1<<28 | t2<<14 | t3), df counts, and
 * ref_len = log(raw ref_len) as the scorer uses it. The engine keeps its own hashed copy, built
 * here (synchronising); the caller's arrays are borrowed as for every nicnes_set_* call. */
int nicnes_set_df_table(nicnes_handle* h, const uint64_t* keys, const double* df, int64_t n, double ref_len_log);

/* Noise-table offsets of members [member_begin, member_begin + count) at `iteration`. */
int nicnes_noise_indices(nicnes_handle* h, uint64_t iteration, int32_t member_begin, int32_t count, uint64_t* out,
                         void* stream);

/* Evaluate `count` members (each an antithetic pair theta +- sigma z): greedy decode of the
 * batch + CIDEr-D fitness. Replaces NESWorker.fitness (src/algorithm/nic_nes/nic_nes_worker.py:115-161)
 * for a whole population slice. fitness_out [count, 2] fp64 = (f+, f-) per member;
 * seq_out [count, 2, B, seq_length] int32 or NULL. */
int nicnes_evaluate(nicnes_handle* h, uint64_t iteration, int32_t member_begin, int32_t count, float sigma,
                    double* fitness_out, int32_t* seq_out, void* stream);

/* The perturbations themselves, delta_k = fp32(sigma * table[idx_k : idx_k + D]) for members
 * [member_begin, +count): out [count, D] fp32. What PolicyNet.evolve returns
 * (src/algorithm/nets.py:101-102, 118) and NESResult.evolve_noise carries to an unchanged reference
 * master (src/algorithm/nic_nes/nic_nes_worker.py:156-161); the engine's own master never needs them. */
int nicnes_noise_vectors(nicnes_handle* h, uint64_t iteration, int32_t member_begin, int32_t count, float sigma,
                         float* out, void* stream);

/* Safe / proportional mutations (PolicyNet.evolve, src/algorithm/nets.py:96-113; Mutation enum :16-21):
 * the member's noise becomes delta' = fp32(fp32(sigma * z) / vec) with mode NICNES_MUTATION_DIVIDE
 * (SM-G-SUM: vec = the sensitivity of src/algorithm/safe_mutations.py:34-117 after its underflow
 * clamp and scaling; SM-VECTOR: the loaded vector, :27-31) or fp32(fp32(sigma * z) * vec) with
 * NICNES_MUTATION_SCALE (SM-PROPORTIONAL: vec = |theta|, zeros replaced by mean |theta|).
 * vec [D] fp32 device (copied). Every later evaluate / grad_partial / noise_vectors uses delta':
 * an evaluation materialises it per member ([max_members, D] on the device, allocated at the first
 * mutated evaluation), the weighted noise sum transforms each delta on the fly.
 * NICNES_MUTATION_PLAIN turns it off. */
#define NICNES_MUTATION_PLAIN 0
#define NICNES_MUTATION_DIVIDE 1
#define NICNES_MUTATION_SCALE 2
int nicnes_set_mutation(nicnes_handle* h, int32_t mode, const float* vec, void* stream);
/* SM-PROPORTIONAL's vector from the handle's own fp32 theta (nets.py:108-112: |theta| with exact zeros replaced
 * by mean|theta|), formed on the device: vec[j] = theta32[j] == 0 ? mean_abs : |theta32[j]|, then mode SCALE.
 * mean_abs is the caller's fp32 mean of |theta| (the reference's torch mean, whose reduction order a device sum
 * would not reproduce). Replaces a host round trip of theta through nicnes_set_mutation(SCALE, vec). */
int nicnes_set_mutation_proportional(nicnes_handle* h, float mean_abs, void* stream);
/* How many entries of the handle's fp32 theta are exactly zero (either sign): when none, SM-PROPORTIONAL's
 * mean is not used and the caller can skip computing it. Synchronises the stream. */
int nicnes_theta_zeros(nicnes_handle* h, int64_t* count_out_host, void* stream);

/* Fitness criterion (Fitness enum + get_criterium, src/captioning/policies.py:22-61, applied at
 * :119-125): GREEDY = 100 * mean CIDEr-D; the greedy_* modes weight each step's probability of the
 * greedy token by the row's CIDEr-D (src/captioning/fitness.py:43-132). The sampled modes decode with
 * FCModel._sample(greedy=False) (src/captioning/nets.py:210-231: each row draws its token from the
 * softmax with one uniform per row and step) on the fused path: SAMPLE = 100 * mean CIDEr-D of the
 * sampled rows; SELF_CRITICAL = 100 * mean of (sampled row's score - greedy row's score), the greedy
 * decode of the same member run first (compute_ciders, policies.py:145-193); SC_LOSS =
 * LogFitnessCriterion (fitness.py:12-40) of the sampled log-probs with those differences as rewards.
 * Sampled rows are not deduplicated: pass the batch with its seq_per_img copies per image (the rows
 * the reference samples independently). */
#define NICNES_FITNESS_GREEDY 0
#define NICNES_FITNESS_GREEDY_LOGPROB 1   /* AltLogFitnessCriterion */
#define NICNES_FITNESS_GREEDY_EXPPROB 2   /* ExpFitnessCriterion */
#define NICNES_FITNESS_GREEDY_LINPROB 3   /* LinFitnessCriterion */
#define NICNES_FITNESS_GREEDY_AVGPROB 4   /* AvgLogFitnessCriterion */
#define NICNES_FITNESS_SAMPLE 5           /* 'sample' */
#define NICNES_FITNESS_SELF_CRITICAL 6    /* 'self_critical' */
#define NICNES_FITNESS_SC_LOSS 7          /* 'sc_loss': LogFitnessCriterion */
/* XENT (an extension: the reference's Fitness enum has no such member, its xent models come from upstream training):
 * the teacher-forced likelihood of the batch's label rows, the reference rows [n_refs, seq_length] of
 * nicnes_set_batch(es), each under its own image. The definition is self-critical.pytorch's FCModel._forward +
 * LanguageModelCriterion (misc/utils.py) over the reference's modules: the image step as FCModel._sample runs it at
 * t = 0 (its logits discarded); then for s = 0..T (T = seq_length, w[T] := 0) the cell over embed(u_s), u_0 = 0 (BOS),
 * u_s = w[s - 1], and lp_s = fl32(fl32(x[w[s]] - m) - lse) with the greedy decode's exact exp-sum. Target s counts
 * when s = 0 or w[s - 1] > 0 (the words plus one end token: 1..T + 1 targets per row). Per row n_tok = the counted
 * targets and lp_sum = the fp64 sum of their lp_s in step order; over rows loss = -sum lp_sum / sum n_tok (the
 * criterion's per-token mean), both sums in a fixed order in fp64 without floating atomics; the fitness of a candidate
 * is -loss over the label rows of its batch (higher is better). In this mode nicnes_evaluate / _lp / _batches return
 * that fitness for both signs of every member (seq_out and logprob_out must be NULL: nothing is decoded) and
 * nicnes_evaluate_theta returns it for theta. E = R = 128 models only: wide and layer_n handles, a mutation set by
 * nicnes_set_mutation* and nicnes_es_evaluate are NICNES_ERR_UNSUPPORTED with this mode, before anything is enqueued. */
#define NICNES_FITNESS_XENT 8
int nicnes_set_fitness_mode(nicnes_handle* h, int32_t mode);
/* After an evaluate in XENT mode: candidate cand's (member k sign s: 2 k + s; nicnes_evaluate_theta: 0) per-row
 * lp_sum_out [rows] fp64 and n_tok_out [rows] int32 (either nullable; host or device pointers, copied on the stream),
 * rows = the label rows of the candidate's batch (nicnes_xent_batch_rows). NICNES_ERR_INVALID without such an evaluate,
 * or with cand or rows outside it. */
int nicnes_xent_rows(nicnes_handle* h, int32_t cand, int32_t rows, double* lp_sum_out, int32_t* n_tok_out, void* stream);
/* rows_out_host[0] = the label rows of batch `batch` of the batches held. */
int nicnes_xent_batch_rows(nicnes_handle* h, int32_t batch, int32_t* rows_out_host);
/* Test entry, in the style of nicnes_test_score_rows: the XENT evaluate of members member_begin .. + count (theta_batch
 * < 0; member_batch_host as nicnes_evaluate_batches) or of theta itself on batch theta_batch (>= 0; count ignored),
 * returning every counted target's lp_s and 0 elsewhere: lp_out_dev [count, 2, stride, seq_length + 1] fp32 with
 * stride = the largest batch's label rows, or [rows of the batch, seq_length + 1] for theta. fitness_out_dev: [count, 2]
 * or [1]. */
int nicnes_test_xent_steps(nicnes_handle* h, uint64_t iteration, int32_t member_begin, int32_t count, float sigma,
                           const int32_t* member_batch_host, int32_t theta_batch, double* fitness_out_dev,
                           float* lp_out_dev, void* stream);

/* Rows per image of the sampled modes: each image of the batch is decoded n times (the reference's
 * seq_per_img copies, dataloader.py:175, which it samples independently), row r reading image r / n and
 * scored against its references; the rollout has B * n rows ([count, 2, B * n, seq_length] tokens). The
 * greedy modes decode one row per image (their copies are identical) and so does the self-critical
 * baseline. Default 1 (a caller may instead pass the copies as rows of the batch). */
int nicnes_set_rows_per_image(nicnes_handle* h, int32_t n);

/* Draws of the sampled modes (not a reference interface; the test hook that replays the reference's
 * numpy draws): the uniforms the next sampled evaluates use, u_host [count, 2, B, seq_length] fp64 (member,
 * sign, row, logit step), copied; n = 0 returns to the engine's own draws (a counter-based hash of the
 * noise seed, iteration, member, sign, row and step, 53-bit like RandomState.random_sample). */
int nicnes_set_sample_draws(nicnes_handle* h, const double* u_host, int64_t n);

/* nicnes_evaluate plus the per-step log-prob of each greedy token, FCModel._sample's seq_logprobs
 * (src/captioning/nets.py:191,208,241): logprob_out [count, 2, B, seq_length] fp32 or NULL. */
int nicnes_evaluate_lp(nicnes_handle* h, uint64_t iteration, int32_t member_begin, int32_t count, float sigma,
                       double* fitness_out, int32_t* seq_out, float* logprob_out, void* stream);

/* nicnes_evaluate_lp where member member_begin + k decodes and is scored on batch
 * member_batch_host[k] (a HOST array of count entries in [0, n_batches), copied before return) of
 * the batches set by nicnes_set_batches. NULL = every member on batch 0 (only with one batch held).
 * Greedy decodes without log-prob output may bound lse from an exp-sum over pair maxima instead of
 * summing every exp (same tokens; rows the bound leaves undecided take the exact pass). The engine
 * switches to the exact sum for the next 32 such decodes when a bounded decode needed >= 2 exact
 * passes (peaked logits of trained models); env NICNES_BOUNDED_LSE=0 / 1 forces never / always. */
int nicnes_evaluate_batches(nicnes_handle* h, uint64_t iteration, int32_t member_begin, int32_t count, float sigma,
                            const int32_t* member_batch_host, double* fitness_out, int32_t* seq_out, float* logprob_out,
                            void* stream);

/* CaptPolicy.rollout of theta itself (src/captioning/policies.py:86-128, called for the eval result
 * of nic_nes_worker.py:65-70 with the unperturbed parameters): fitness_out[0] = the fitness of the
 * batch (the one held, or batch `batch` of nicnes_set_batches), decoded ONCE. At sigma = 0 both
 * antithetic signs are theta, so sign + decodes the first ceil(B/2) images and sign - the rest and
 * the halves are scored as one rollout: seq_out [B, seq_length] int32 and logprob_out [B, seq_length]
 * (both nullable, rows 0..B-1 in batch order) and the fitness equal nicnes_evaluate_lp's sign-+
 * row of a sigma = 0 member bit for bit, at half its decode work. The sampled fitness modes draw from
 * the stream of `iteration` reserved for eval rollouts (member index 2^32 - 1 in the draw hash), so each
 * eval rollout draws afresh, as the reference's worker RNG does, and never shares an evolve member's
 * draws. */
int nicnes_evaluate_theta(nicnes_handle* h, int32_t batch, uint64_t iteration, double* fitness_out, int32_t* seq_out,
                          float* logprob_out, void* stream);

/* A resident evaluation split: the images a validation score is computed on (CaptPolicy.accuracy_on -> eval_split,
 * src/captioning/policies.py:130-143, src/captioning/eval_utils.py:110-180: a greedy decode of theta on the first
 * num_val_items images of a split, one row per image, scored by COCOEvalCap, eval_utils.py:60-107). Owned by the
 * handle (destroyed with it), and separate from everything the evaluates use: the training batches, the handle's df
 * table, the fitness mode, the mutation, rows_per_image and the sampled draws are neither read nor changed by the
 * nicnes_split_* calls.
 * nicnes_split_create copies its arrays before it returns (synchronising; each may be a host or a device pointer):
 * fc [N, F] fp32; ref_tokens [n_refs, seq_length] and img_ref_start [N + 1] in the layout of nicnes_set_batch;
 * the split's OWN document-frequency table in the layout of nicnes_set_df_table (COCOEvalCap's Cider takes its df
 * from the evaluated split's references, ref_len_log = log(N) then). n_refs = 0 makes a decode-only split (images
 * without references: nicnes_split_score / _evaluate return NICNES_ERR_INVALID on it). */
typedef struct nicnes_split nicnes_split;
int nicnes_split_create(nicnes_handle* h, const float* fc, int32_t N, const int32_t* ref_tokens, int32_t n_refs,
                        const int32_t* img_ref_start, const uint64_t* df_keys, const double* df, int64_t n_df,
                        double ref_len_log, nicnes_split** out, void* stream);
int nicnes_split_destroy(nicnes_handle* h, nicnes_split* split);
/* Greedy tokens of the handle's current theta itself (no mutation applies, no noise table is needed, as
 * nicnes_evaluate_theta) on images [first, first + count) of the split, any count in [1, N], in ONE enqueue: the
 * range's slabs are the halves of ceil(count / 256) pseudo-members over the zero noise slice, on the decode path
 * (fused / split / coop) the engine's shape rule picks for that many workgroups; the tail's rows are decoded and
 * dropped. seq_out [count, seq_length] int32: bit for bit nicnes_evaluate_theta's rows of the same images, whatever
 * the shape. logprob_out (nullable) [count, seq_length] fp32: the log-prob of every token up to and including the
 * row's end token and 0 after it (nicnes_evaluate_theta's rows also keep the later steps their batch still ran,
 * which depend on the batch's other rows). The work buffers grow with the largest range decoded (synchronising
 * then); more than 2^20 images in one range is NICNES_ERR_INVALID. */
int nicnes_split_decode(nicnes_handle* h, nicnes_split* split, int32_t first, int32_t count, int32_t* seq_out,
                        float* logprob_out, void* stream);
/* COCOEvalCap's java-free metrics of GIVEN token rows seq_dev [count, seq_length] as the captions of images
 * [first, first + count): a caption is its tokens before the first 0 (decode_sequence, eval_utils.py:13-27), the
 * references likewise; an empty caption scores 0 and has length 0. metrics_out_dev [6] fp64 = Bleu_1..4 (corpus
 * level, pycocoevalcap bleu_scorer with option 'closest'), ROUGE_L (mean over images, beta = 1.2), CIDEr (mean
 * CIDEr-D over images on the reference's scale, sigma = 6, the split's df table; no x 100). totals_out_dev [10]
 * int64 = the BLEU statistics correct[1..4], guess[1..4], testlen, reflen. row_cider_out_dev (nullable) [count]
 * fp64 = every image's CIDEr-D. Sums run in a fixed order (no floating atomics): the same bits on every run. On a
 * handle with a contained decode fault (nicnes_stats) the six metrics are NaN, as the fitness is. */
int nicnes_split_score(nicnes_handle* h, nicnes_split* split, int32_t first, int32_t count, const int32_t* seq_dev,
                       int64_t* totals_out_dev, double* metrics_out_dev, double* row_cider_out_dev, void* stream);
/* nicnes_split_decode + nicnes_split_score of its tokens; seq_out (nullable) [count, seq_length] receives them. */
int nicnes_split_evaluate(nicnes_handle* h, nicnes_split* split, int32_t first, int32_t count, int64_t* totals_out_dev,
                          double* metrics_out_dev, double* row_cider_out_dev, int32_t* seq_out, void* stream);

/* The teacher-forced cross-entropy (NICNES_FITNESS_XENT's definition) of the handle's current theta on the label rows
 * (the split's reference rows) of images [first, first + count), in ONE enqueue; no handle state is read but theta or
 * changed (the fitness mode, df table, batches and mutation stay as they are). out2_dev [2] fp64 = loss, perplexity
 * exp(loss); tokens_out_dev [1] int64 = sum n_tok; lp_sum_out_dev / n_tok_out_dev (nullable) [rows] = the range's
 * rows img_ref_start[first] .. img_ref_start[first + count). The same bits on every run, and those of
 * nicnes_evaluate_theta in XENT mode on a batch of the same images. NICNES_ERR_UNSUPPORTED on a decode-only split and
 * on wide / layer_n handles. */
int nicnes_split_xent(nicnes_handle* h, nicnes_split* split, int32_t first, int32_t count, double* out2_dev,
                      int64_t* tokens_out_dev, double* lp_sum_out_dev, int32_t* n_tok_out_dev, void* stream);

/* Beam-search decode of the handle's current theta on images [first, first + count) of the split, for evaluation, in
 * ONE enqueue with no host synchronisation (the work buffers grow with the largest (count, beam) seen, synchronising
 * then). beam in 1..8 (else NICNES_ERR_INVALID). A hypothesis is an LSTM state, its tokens and an fp64 score; at every
 * step the candidates (hypothesis b, word v) of an image, score_b + (double)logprob_b[v] with the greedy decode's
 * log-probs, are ordered by (score descending, b ascending, v ascending) and the first min(beam, candidates) taken;
 * one with v = 0, or taken at step seq_length, finishes, the others are the next step's hypotheses. The result is
 * the finished hypothesis of the largest score (ties: finished at the earlier step, then earlier in selection
 * order); an image stops once its best finished score is >= every live one. NO length normalisation is applied.
 * beam = 1 is the greedy decode. seq_out [count, seq_length] int32 zero-padded; score_out (nullable) [count] fp64.
 * One deviation from that order: each of a hypothesis's two vocabulary halves (ids with (v >> 2) even / odd) keeps its
 * beam best words by LOGIT before the log-probs exist, so where a kept and a dropped logit of one half round to the
 * same fp32 log-prob the larger logit is taken, not the smaller id (for beam = 1: the largest logit, where the greedy
 * decode takes the first id of its log-prob tie window). An image whose logits are not finite finishes nothing: its
 * tokens are zeros and its score -inf. */
int nicnes_split_decode_beam(nicnes_handle* h, nicnes_split* split, int32_t first, int32_t count, int32_t beam,
                             int32_t* seq_out, double* score_out, void* stream);
/* nicnes_split_decode_beam + nicnes_split_score of its tokens; seq_out (nullable) receives them. */
int nicnes_split_evaluate_beam(nicnes_handle* h, nicnes_split* split, int32_t first, int32_t count, int32_t beam,
                               int64_t* totals_out_dev, double* metrics_out_dev, double* row_cider_out_dev,
                               int32_t* seq_out, void* stream);

/* A resident training set: every image of the training split on the GPU, so that an iteration's batches are drawn by
 * image index with device copies instead of being read, stacked and uploaded by the host (replaces what
 * src/captioning/dataloader.py:148-203 get_batch assembles and nic_nes_worker.py:121-128 hands to every member's
 * rollout: fc_feats and gts of the drawn images). Owned by the handle (destroyed with it), several may exist at once.
 * nicnes_trainset_create copies its arrays before it returns (synchronising; each may be a host or a device pointer):
 * fc [N, F] fp32; ref_tokens [n_refs, seq_length] and img_ref_start [N + 1] in the layout of nicnes_set_batch. It
 * checks once what nicnes_set_batches checks per call (the ranges tile [0, n_refs), every image has >= 1 reference)
 * and that every token lies in [0, vocab_size], and keeps a host copy of every image's reference count. N <= 2^24.
 * fc may be NULL: the rows are then zeros until nicnes_trainset_write_fc writes them, so that a caller who reads the
 * split in chunks never holds it whole, on the host or in a second device buffer. */
typedef struct nicnes_trainset nicnes_trainset;
int nicnes_trainset_create(nicnes_handle* h, const float* fc, int32_t N, const int32_t* ref_tokens, int32_t n_refs,
                           const int32_t* img_ref_start, nicnes_trainset** out, void* stream);
/* Rows [first, first + count) of the set's fc <- fc [count, F] fp32 (a host or a device pointer, copied before return;
 * synchronises `stream` first): the chunked form of nicnes_trainset_create's fc argument (dataloader.py:209-243, one
 * image's fc feature at a time). A range outside [0, N) is NICNES_ERR_INVALID. */
int nicnes_trainset_write_fc(nicnes_handle* h, nicnes_trainset* ts, int32_t first, int32_t count, const float* fc,
                             void* stream);
int nicnes_trainset_destroy(nicnes_handle* h, nicnes_trainset* ts);
/* nicnes_set_batches for images image_ix_host [n_batches * B] of the set (a HOST array of indices in [0, N), copied
 * before return; batch g holds entries g * B .. g * B + B - 1; an image may occur any number of times): afterwards the
 * handle is in the state nicnes_set_batches leaves for the same images in the same order (fc, B, n_batches, the
 * reference ranges, the cooked reference vectors, the per-image n-gram tables), except that fc, the reference rows
 * and the starts live in buffers the handle owns, gathered there on `stream` (dataloader.py:148-203 get_batch without
 * the host: one gather of fc rows, one of label rows). n_refs, the starts and the largest reference count come from
 * the host's copy of the counts: the call only enqueues, with no copy back and no wait, unless a buffer has to grow
 * (B > max_batch, more references than max_refs, more images than the image capacity: as nicnes_set_batches,
 * synchronising). The indices and starts travel through pinned staging of the handle, a slot of which is reused only
 * after the copy that read it has run. NICNES_ERR_INVALID before anything is enqueued or changed (the batch held
 * before still evaluates): an index outside [0, N), B or n_batches outside nicnes_set_batches' limits, a set that is
 * not this handle's (or destroyed), no df table. nicnes_set_df_table invalidates a drawn batch as any other. */
int nicnes_draw_batches(nicnes_handle* h, nicnes_trainset* ts, const int32_t* image_ix_host, int32_t n_batches, int32_t B,
                        void* stream);
/* Test entry (no reference counterpart): the batch arrays the handle currently reads, whichever call set them
 * (nicnes_set_batches' borrowed buffers or a draw's own), copied to caller DEVICE buffers (each nullable): fc_out
 * [n_batches * B, F] fp32, refs_out [n_refs, seq_length] int32, starts_out [n_batches * B + 1] int32. Only enqueues. */
int nicnes_test_batch_state(nicnes_handle* h, float* fc_out, int32_t* refs_out, int32_t* starts_out, void* stream);

/* Centred ranks + antithetic weights over the WHOLE population, replaces
 * NESMaster.compute_centered_ranks and the weights line of gradient_estimate
 * (src/algorithm/nic_nes/nic_nes_master.py:170-205). fitness [P, 2] fp64 -> cr [P, 2] (or NULL),
 * w [P] fp32. */
int nicnes_rank_weights(nicnes_handle* h, const double* fitness, int32_t P, double* cr_out, float* w_out, void* stream);

/* gsum = sum over members [member_begin, +count) of w[i] * delta_i (fp32 result of an fp64 sum);
 * replaces batched_weighted_sum (nic_nes_master.py:207-221) without materialising delta.
 * `w` points at the weights of member_begin. Multi-GPU: all-reduce gsum between the call
 * and nicnes_adam_step. */
int nicnes_grad_partial(nicnes_handle* h, uint64_t iteration, int32_t member_begin, int32_t count, const float* w,
                        float sigma, float* gsum_out, void* stream);
/* The same sum on parameters [j0, j1) only (j0 a multiple of 64): gsum_out[j0 .. j1) written. Lets a
 * multi-GPU caller all-reduce one range while the next is summed (not a reference interface). */
int nicnes_grad_partial_range(nicnes_handle* h, uint64_t iteration, int32_t member_begin, int32_t count, const float* w,
                              float sigma, int64_t j0, int64_t j1, float* gsum_out, void* stream);

/* g = gsum / (2P); globalg = -g + l2coeff * theta; Adam step on the engine's theta
 * (nic_nes_master.py:126-137, optimizers.py:15-22,78-83). With ratio_out_host set it is
 * synchronising and returns the update ratio |step| / |theta_old| there; with NULL it only
 * enqueues, and nicnes_last_ratio reads the ratio later (so an iteration loop need not idle
 * the GPU once per step). */
int nicnes_adam_step(nicnes_handle* h, const float* gsum, int32_t P, double l2coeff, double stepsize, double beta1,
                     double beta2, double epsilon, double* ratio_out_host, void* stream);

/* The update ratio of the newest optimizer step (synchronising on `stream`). */
int nicnes_last_ratio(nicnes_handle* h, double* ratio_out_host, void* stream);

/* SGD with momentum in the same fused form (src/algorithm/nic_nes/optimizers.py:38-47). */
int nicnes_sgd_step(nicnes_handle* h, const float* gsum, int32_t P, double l2coeff, double stepsize, double momentum,
                    double* ratio_out_host, void* stream);

/* Optimizer.update(globalg) (optimizers.py:15-22) with a caller-provided globalg [D] widened to
 * fp64; globalg_fp32 = 1 when the caller's array was fp32 (numpy then keeps (1 - b) * globalg in
 * fp32). kind 0 = Adam (beta1, beta2, epsilon), 1 = SGD (beta1 = momentum). Synchronising (ratio). */
int nicnes_optimizer_update(nicnes_handle* h, int kind, const double* globalg, int globalg_fp32, double stepsize,
                            double beta1, double beta2, double epsilon, double* ratio_out_host, void* stream);

/* Multi-GPU data plane: one handle per GPU, one rank per handle. The reference
 * has no collective -- its master gathers every worker's 11.46 MB noise vector over redis and sums
 * them in gradient_estimate (src/dist.py:90-93,199-201, src/algorithm/nic_nes/nic_nes_master.py:
 * 92-123,170-182); the engine exchanges the (P, 2) fitness and one D-float noise sum over RCCL.
 * nicnes_comm_unique_id: rank 0 makes the 128-byte id and sends it to the other ranks out of band;
 * nicnes_comm_init: every rank joins (collective, blocking); nicnes_comm_attach borrows an
 * ncclComm_t the caller already owns (e.g. torch.distributed's); nicnes_comm_destroy releases.
 * nicnes_comm_count: the rank count and this rank's index as RCCL itself reports them
 * (ncclCommCount / ncclCommUserRank on the bound communicator; 1 and 0 with none bound) -- what a
 * multi-GPU bench line records to prove the collective saw N ranks (the reference's counterpart is
 * the number of live worker processes, src/main.py:144-153). */
#define NICNES_COMM_ID_BYTES 128
int nicnes_comm_unique_id(uint8_t* id_out_host);
int nicnes_comm_init(nicnes_handle* h, int32_t nranks, int32_t rank, const uint8_t* id_host);
int nicnes_comm_attach(nicnes_handle* h, void* nccl_comm);
int nicnes_comm_destroy(nicnes_handle* h);
int nicnes_comm_count(nicnes_handle* h, int32_t* nranks_out_host, int32_t* rank_out_host);
/* fit_all [P_local * nranks, 2] fp64 <- every rank's fit_local [P_local, 2], in rank order, so every
 * rank then ranks the whole population identically (compute_centered_ranks needs all 2P values). */
int nicnes_allgather_fitness(nicnes_handle* h, const double* fit_local, int32_t P_local, double* fit_all, void* stream);
/* gsum [D] fp32 summed in place over the ranks: the shards' nicnes_grad_partial results become the
 * whole population's noise sum before nicnes_adam_step (batched_weighted_sum, nic_nes_master.py:207-221). */
int nicnes_allreduce_grad(nicnes_handle* h, float* gsum, void* stream);

/* diagnostics since creation (synchronising): [0] = exact-pass fallbacks of the greedy tie rule,
 * [1] = sampled picks whose crossing stage's own sums stopped short of the threshold by rounding (its last id),
 * [2] = coop-path hand-off timeouts, [3] = sampled workgroups that found no free logit slot.
 * Decode faults ([2] or [3] nonzero: rows left undecoded) are sticky and contained on the device, in the
 * iteration that hit them, without a host wait: every fitness written from then on is NaN, nicnes_grad_partial
 * writes NaN everywhere (so an all-reduce carries the fault to every rank), and an optimizer step on this handle,
 * or on a noise sum whose first entry is NaN, leaves theta, m and v untouched. The error (NICNES_ERR_FAULT) is
 * returned by the next evaluate that finds the counters read back, and by the ratio read of the skipped step
 * (nicnes_adam_step / nicnes_sgd_step with ratio_out_host, nicnes_last_ratio); a skipped step is known by
 * the Adam kernel's own skip flag, so the NaN ratio of an applied step (0/0) is returned as a ratio, not an
 * error. The handle stays faulted until nicnes_clear_faults, or destroy it (the reference's worker process
 * dies and is restarted, main.py:107-141). */
/* out8_host [4..7], the screened decode's step queue (nicnes_set_decode_queue): [4] = tasks (member slab, step) run
 * and [5] = waits that ran past their bound, both over the handle's life; [6] = member slabs the last queue launch
 * counted finished, [7] = tasks it left in the ring (0 after a sound launch). A queue timeout also counts in [2]: it
 * is a hand-off timeout and is contained and reported as one. */
int nicnes_stats(nicnes_handle* h, int64_t* out8_host);

/* Clear a contained decode fault (synchronising on the device): out2_host (nullable) receives the fault
 * counters [2], [3] of nicnes_stats before they are zeroed; the logit-slot claim flags are reset. theta, m
 * and v are those from before the faulted iteration (its step was skipped), so a caller can re-run that
 * iteration on the same handle (nicnes.master.EngineMaster.run does, once). Not a reference interface: the
 * reference's recovery is a fresh worker process (main.py:107-141). */
int nicnes_clear_faults(nicnes_handle* h, int64_t* out2_host);

/* Kernel timing with HIP events recorded on the launch stream around the decode and CIDEr-D
 * launches of nicnes_evaluate (off by default). nicnes_kernel_times synchronises on the events
 * and returns the last call's [0] = decode ms, [1] = CIDEr-D ms. */
int nicnes_set_timing(nicnes_handle* h, int on);
int nicnes_kernel_times(nicnes_handle* h, float* out2_host);

/* Per-kernel split of the last timed decode (events between its launches), in ms: [0] img-embed
 * kernel, [1] the two cell-only launches (t = -1, 0; one-launch-per-step builds only), [2] fused
 * path: the steps kernel (every step t = -1..T in one launch; or the per-step launches summed),
 * [3] its launch count, [4] split-path logit launches summed, [5] their count, [6] split-path cell
 * launches summed (token merge + next cell, t = -1..T), [7] their count. The coop path's one launch
 * counts as [2] / [3]. Synchronising. */
int nicnes_decode_phase_times(nicnes_handle* h, float* out8_host);

/* Decode launch shape. Not a reference interface: the reference decodes one member per CPU process
 * (src/algorithm/nic_nes/nic_nes_worker.py:142-154); the engine spreads a member over S workgroups
 * when members x slabs cannot fill the GPU. S = 0 / G = 0 pick automatically (S from the CU count,
 * G = 2 -- 64-row slabs -- when B pads to fewer rows that way, e.g. mscoco_nes.json batch_size 64).
 * G = 4 with S = 1 is the fused path (one launch for every step). Tokens do not depend on the shape.
 * On a wide handle (nicnes_decode_path 3) the shape is always G = 4, S = 1: S = 0 or 1 with G = 0 or 4 is accepted
 * and changes nothing, S > 1 or G = 2 returns NICNES_ERR_UNSUPPORTED. */
int nicnes_set_decode_split(nicnes_handle* h, int32_t S, int32_t G);
/* the shape an evaluate of `count` members of a B-image batch would use: [0] G, [1] slabs, [2] S */
int nicnes_decode_shape(nicnes_handle* h, int32_t B, int32_t count, int32_t* out3_host);
/* Decode streams (not a reference interface): the evaluate's members split evenly over n streams, the
 * caller's and n - 1 engine streams joined back into the caller's before the CIDEr-D launch, so that one
 * part's launches fill the CUs the others' launch gaps leave idle. n = 0 picks automatically (2 on the
 * split path, 1 on the fused path), 1..4 forces; env NICNES_DECODE_STREAMS sets the initial value. A
 * multi-stream decode records no per-launch events (nicnes_decode_phase_times reports zeros).
 * Tokens do not depend on n. A wide handle decodes on one stream: n = 0 and 1 are accepted, n > 1 returns
 * NICNES_ERR_UNSUPPORTED. */
int nicnes_set_decode_streams(nicnes_handle* h, int32_t n);
/* Coop decode (not a reference interface): when the split shape has 128-row slabs, S = 2 or 4 and every
 * workgroup fits on the GPU at once (S x members x slabs <= the kernel's occupancy x CUs, from
 * hipOccupancyMaxActiveBlocksPerMultiprocessor: 64 or 128 members per GPU at B = 128), the whole decode runs
 * as one persistent launch (env NICNES_COOP_LAUNCH=1: a cooperative launch, whose runtime check refuses a grid
 * that cannot be resident at once; 0.4 % slower per iteration at P = 64) whose S workgroups per
 * member slab hand the partial greedy states and h' to each other (mode 1, the default; env
 * NICNES_DECODE_COOP=0/1 sets the initial value), instead of two launches per step (mode 0). Tokens do not
 * depend on it. A partner missing for 0.5 s is a decode fault (nicnes_stats).
 * On a wide handle (nicnes_decode_path 3) the call is accepted, because the worker and nic_es layers set it on every
 * engine of a shared device, and has no effect: there is no coop launch at wide dims, whatever the mode. */
int nicnes_set_decode_coop(nicnes_handle* h, int32_t mode);

/* SM-G-SUM sensitivity of the current theta on the first `rows` images of the batch held (batch 0):
 * replaces Sensitivity.calc_sensitivity / _calc_sum_sensitivity (src/algorithm/safe_mutations.py:34-117)
 * on CaptionModel.forward_for_sensitivity (src/captioning/nets.py:22-70; length 5, groups of 100).
 * out (device, D floats) = sqrt(sum_k J[k, :]^2) / rows, clamped to >= underflow and divided by it
 * (safe_mutations.py:63-65; underflow <= 0: the raw vector). The greedy tokens come from the engine's
 * bit-exact decode; the K = V1 / 100 + 1 backward passes run batched on the GPU, so the vector agrees
 * with the reference's to fp32 rounding (a stated tolerance), not bit for bit. Asynchronous on stream.
 * Limit: rows <= 819 (the embedding kernels list the 5 * rows token cells in LDS, 4096 at most), whatever
 * max_batch is: NICNES_ERR_UNSUPPORTED above it, before anything is enqueued. */
int nicnes_sum_sensitivity(nicnes_handle* h, int32_t rows, float underflow, float* out_dev, void* stream);
/* The kernels the last sensitivity run of this handle chose (nicnes_sum_sensitivity or nicnes_sensitivity_es, which
 * share the work buffers; after nicnes_sensitivity_es: its last slot's run). Host bookkeeping only: no kernel, no
 * synchronisation. out_host[0]: bit 0 logit.weight square sums on the LDS-resident kernel (rows <= 128), bit 1 the
 * backward recurrence fused into one launch per cell (i2h / h2h weights 16-byte aligned), bit 2 gate and image weight
 * square sums on the k-invariant-B kernel (K <= 96), bit 3 embedding rows in two passes (K <= 96); a clear bit is the
 * general tile / range kernel. out_host[1], out_host[2]: the run's tile products launched with 16-byte and with
 * scalar operand loads. NICNES_ERR_INVALID before the first run (and after one that failed while it enqueued). For tests and reports. */
int nicnes_sens_paths(nicnes_handle* h, int32_t* out_host);
/* the decode path an evaluate of `count` members of a B-image batch would take: 0 fused (one launch,
 * one workgroup per member slab), 1 split (two launches per step), 2 coop (the split shape in one launch), 3 wide (a
 * model with input_encoding_size or rnn_size above 128, or NICNES_DECODE_WIDE=1: one launch, one workgroup per member
 * and 128-row slab, whatever B and count), 4 ln (a layer_n model: the wide shape on the layer-norm kernel) */
int nicnes_decode_path(nicnes_handle* h, int32_t B, int32_t count, int32_t* out_host);
/* the log-sum-exp mode of the last greedy decode enqueued: 1 the pair-bounded lse (greedy-only decodes while the
 * engine's adaptive policy allows it), 0 the exact exp-sum (log-probs written, NICNES_BOUNDED_LSE=0, or the policy's
 * exact stretch after a bounded decode needed exact passes). Measurement bookkeeping for bench.py (which kernel
 * instantiation a line's PMC counters belong to); no reference counterpart. */
int nicnes_last_decode_lse(nicnes_handle* h, int32_t* bounded_host);
/* Screened decode (not a reference interface): mode 1 runs the logit loop of the fused greedy-only decode
 * (128-row slabs, one workgroup per member slab, pair-bounded lse, no log-probs, plain mutations) in bf16 and certifies
 * the candidate tokens it leaves with exact fp32 chains; mode 0 the fp32 loop; mode 2 (the default) screens when the
 * decode has at least as many workgroups (members x slabs) as the GPU has CUs, where it is faster. Tokens do not depend on it.
 * env NICNES_SCREEN=0/1/2 sets the initial value; test hook NICNES_SCREEN_EPS_SCALE (>= 1) widens the screening bound.
 * env NICNES_SCREEN_ROUNDS (1..64, default 2): the round budget R. A lane with more hits than one hit list holds (8 hit
 * weights, a crowded lane-stage weighs 4) certifies them in further rounds while it holds at most 8 R; above that its
 * step goes to the fp32 loop. R bounds the weight, not the number of rounds: packing weights of 4 into rounds of 8 can
 * take a lane one round more than R. 1: no round after the first.
 * On a wide handle (nicnes_decode_path 3) the call returns NICNES_OK and is ignored: the wide decode never screens, its
 * logit loop is fp32 with the exact exp-sum whatever the mode, and the screening counters of nicnes_stats stay 0. */
int nicnes_set_decode_screen(nicnes_handle* h, int32_t mode);
/* Step queue of the screened decode (not a reference interface: the reference decodes a member's caption in one
 * FCModel._sample call, src/captioning/nets.py:183-245, and has no dispatch of its own; DESIGN.md 5, "Step queue"): mode 1
 * runs the screened fused decode (nicnes_set_decode_screen) as `workers` persistent workgroups that take (member slab,
 * step) tasks from a FIFO ring on the device, so the launch ends within about a step of total work / workers instead of
 * with the CU whose member slabs sum longest; mode 0 one workgroup per member slab; mode 2 (the default) the queue when
 * the decode has more member slabs than workers. workers 0: the device's CU count. Tokens do not depend on it. env
 * NICNES_DECODE_QUEUE=0/1/2 and NICNES_DECODE_QUEUE_WORKERS=n set the initial values. A wait in the queue that lasts
 * 0.5 s is a decode fault (nicnes_stats).
 * On a wide handle (nicnes_decode_path 3) the call returns NICNES_OK and is ignored: the wide decode has no step queue
 * and always runs one workgroup per member and 128-row slab. */
int nicnes_set_decode_queue(nicnes_handle* h, int32_t mode, int32_t workers);
/* The rule behind it, without a handle (pure; for tests and tools): for a screened fused decode of members x slabs
 * member slabs on a device of n_cu CUs, out3_host = {1 when the queue kernel runs, its workgroups, the ring's slots (a
 * power of two >= members x slabs)}. mode < 0: mode and workers from the environment variables above (defaults 2, 0). */
int nicnes_decode_queue_plan(int32_t mode, int32_t workers, int32_t n_cu, int32_t members, int32_t slabs,
                             int32_t* out3_host);
/* the screened decodes' counters since create: [0] candidate ids captured, [1] rows the first certify round left
 * bad (before the certify rounds each sent its workgroup's step to the fp32 loop; nicnes_screen_reasons says what
 * became of them) */
int nicnes_screen_stats(nicnes_handle* h, int64_t* out2_host);
/* why rows were left bad, and what became of them, since create. Of the rows of nicnes_screen_stats' [1]: [0] with a
 * lane over the hit-list cap, [1] with a record between the inner and outer tie window, [2] with an evicted record in
 * the window, [3] with a non-finite bound (or NICNES_FORCE_EXACT); a row may have several. [4] rows that later certify
 * rounds settled, [5] rows that went to the fp32 loop, [6] workgroup steps that ran it. [7 + k], k < 8: over-cap rows
 * whose fuller lane holds 8 (k + 1) + 1 .. 8 (k + 2) hit weights (k = 7: or more), i.e. needs at least k + 2 rounds.
 * [15] waves that ran the fp32 loop, of the 8 of each workgroup step of [6] (the others held no bad row and sat it out) */
int nicnes_screen_reasons(nicnes_handle* h, int64_t* out16_host);
/* Test entry (no reference counterpart): every vocabulary logit of member `member` of `iteration` at sigma, sign
 * (0: +, 1: -), over 32 given rows of h (h_rows_dev [32, 128] fp32, unit order), computed twice: out_mfma_dev by the
 * 32-row fp32 MFMA tile path of the exact pass, out_chain_dev by the function the screened decode certifies with (one
 * lane's fmaf chain in the MFMA's k order, nicnes_math.h nn_kperm), both reading h from the engine's lane scratch in
 * the decode's layout (so no decode may run beside it), both [32, vocab_size + 1] fp32 on the device. The two are equal bit for bit: that is what
 * lets a screened decode certify a candidate's exact logit without staging a tile. Plain mutations
 * only. Asynchronous on stream. */
int nicnes_test_logit_chain(nicnes_handle* h, uint64_t iteration, int32_t member, float sigma, int32_t sign,
                            const float* h_rows_dev, float* out_mfma_dev, float* out_chain_dev, void* stream);
/* Test entry (no reference counterpart), layer_n handles only: one LSTM cell of theta itself (no perturbation) on
 * `rows` <= 128 given rows, x_dev [rows, input_encoding_size], h_dev and c_dev [rows, rnn_size] fp32 in unit order, by
 * the device function the layer-norm decode runs its cells with (the rows are spread to one workgroup's lane scratch
 * in the decode's layout, so no decode may run beside it); h_out_dev and c_out_dev [rows, rnn_size] receive h' and
 * the un-normalised c'. Asynchronous on stream. */
int nicnes_test_ln_cell(nicnes_handle* h, const float* x_dev, const float* h_dev, const float* c_dev, int32_t rows,
                        float* h_out_dev, float* c_out_dev, void* stream);
/* Test entry (no reference counterpart): given candidates through the screened decode's tile certify (DESIGN.md
 * 5). h_rows_dev [128, 128] fp32 (unit order) is laid out as the lane scratch of one decode workgroup's eight waves;
 * items_host [n_items, 2] int32 (HOST) holds (row in [0, 128), vocabulary id in [0, vocab_size]) pairs in any order,
 * repeats allowed. Each item is owned by the thread the decode gives that row of `sign` and goes through the same wave
 * item list, row staging, fp32 MFMA tile and result words as a decode's candidates; out_dev [n_items] fp32 receives
 * each item's exact logit of member `member` of `iteration` at sigma, bit for bit nicnes_test_logit_chain's. A row or
 * an id out of range is NICNES_ERR_INVALID and nothing runs. No decode may run beside it. Plain mutations only.
 * Synchronises the stream. */
int nicnes_test_certify_items(nicnes_handle* h, uint64_t iteration, int32_t member, float sigma, int32_t sign,
                              const float* h_rows_dev, const int32_t* items_host, int32_t n_items, float* out_dev,
                              void* stream);
/* The same with the items' owners chosen: owner_by_id = 0 gives every item to lane half 0 of its row (as above); 1
 * gives item (row, id) to lane row % 32 + 32 * ((id >> 2) & 1) of the row's wave, the lane a decode's hit lists put it
 * behind, each lane's ids in increasing order. The certify's results cross lane halves through LDS in general; only
 * this mode has owners in both. */
int nicnes_test_certify_items_owned(nicnes_handle* h, uint64_t iteration, int32_t member, float sigma, int32_t sign,
                                    int32_t owner_by_id, const float* h_rows_dev, const int32_t* items_host,
                                    int32_t n_items, float* out_dev, void* stream);
/* Test entry (no reference counterpart): the scorer of nicnes_evaluate* on GIVEN token rows instead of a decode's, so a
 * test can choose the hypotheses (caption lengths, repeats, ids at the key packing's top bit) that a decode of a random
 * theta never emits. seq_dev [n_cand, rows, seq_length] int32; candidates 2k and 2k + 1 are member k's, scored on batch
 * member_batch_host[k] (HOST, n_cand / 2 entries, copied; NULL = the one batch held; needs an even n_cand);
 * lp_dev [n_cand, rows, seq_length] fp32 (nullable: the criteria modes then give the mean form, as an evaluate without
 * log-probs cannot; the criteria stop a row's mask at its first 0, so rows given with log-probs are 0 from their first
 * 0 on, as a decode's are); base_dev [n_cand, rows / rpi] fp64 (nullable) = the self-critical modes' greedy row scores.
 * scores_out_dev [n_cand, rows] fp64 = every row's CIDEr-D, fitness_out_dev [n_cand] fp64 = the fitness of the handle's
 * current mode. Uses the handle's fitness mode, rows-per-image setting (rows must be B * rpi; rpi = 1 in the greedy
 * modes), held batches and df table; needs no theta and no noise table. It runs the dispatch the evaluates end with
 * (image tables when every image has <= 8 references, else the per-reference scan). NICNES_ERR_INVALID: no batch set,
 * rows != B * rpi, n_cand outside [1, 2 * max_members] (the row-score scratch), member_batch with an odd n_cand or an
 * entry outside [0, n_batches). Asynchronous on stream. */
int nicnes_test_score_rows(nicnes_handle* h, const int32_t* seq_dev, int32_t n_cand, int32_t rows,
                           const int32_t* member_batch_host, const float* lp_dev, const double* base_dev,
                           double* scores_out_dev, double* fitness_out_dev, void* stream);

/* The beam decode's workgroup shape: 4 or 8 waves, or 0 (the default) for the launch's own rule, which takes the shape
 * that needs fewer rounds over the CUs. The tokens and scores do not depend on it; it exists for tests and timing. */
int nicnes_set_beam_waves(nicnes_handle* h, int32_t waves);
/* Test entry: the beam decode's own per-lane top-K and selection code on GIVEN rows. lp_dev [n_img, beam, V1] fp32
 * log-probs, score_dev [n_img, beam] fp64, live_dev [n_img, beam] int32 (0: the hypothesis is dead and gives no
 * candidate). out_dev [n_img, beam, 2] int32: the selected (b, v) pairs of every image in selection order, (-1, -1)
 * where fewer than beam candidates exist. Any V1 >= 1; needs no theta. Asynchronous on stream. */
int nicnes_test_beam_select(nicnes_handle* h, const float* lp_dev, const double* score_dev, const int32_t* live_dev,
                            int32_t n_img, int32_t beam, int32_t V1, int32_t* out_dev, void* stream);

/* ---- nic_es: the truncation-selection GA (src/algorithm/nic_es/) ----------------------------------------------------
 * The reference keeps every parent, offspring and elite as a .pth file on a shared disk (11.46 MB each). Here a parent
 * is a row of a device table and an offspring is (parent slot, noise index, sign): pair k of a generation perturbs
 * parent parent_of[k] by delta'_k, taken from the shared noise table at the existing index rule on (generation, k),
 * and its two offspring, ids 2k (parent + delta') and 2k + 1 (parent - delta'), share one staging of that row. Only
 * the selected offspring are ever written out, by nicnes_es_advance, on the device.
 * nicnes_es_create allocates the state on the handle (synchronising): two parent tables [max_parents, Dp] fp32
 * (double-buffered: the selected offspring reference the old parents), an elite table [max_elites, Dp], Dp = D rounded
 * up to 64 floats. Replaces the directories of ESIteration (src/algorithm/nic_es/iterations.py). */
int nicnes_es_create(nicnes_handle* h, int32_t max_parents, int32_t max_elites);
int nicnes_es_free(nicnes_handle* h);
/* ES mutation (PolicyNet.evolve with the parent as param_vector, src/algorithm/nets.py:96-113): NICNES_MUTATION_PLAIN,
 * or NICNES_MUTATION_SCALE = SM-PROPORTIONAL, delta'[j] = fp32(fp32(sigma z[j]) * a[j]) with a[j] = |theta_p[j]|, or
 * mean|theta_p| where theta_p[j] is exactly 0; the mean is the engine's (fp32 of an fp64 sum in a fixed order, formed
 * when the row is written). Any other mode, NICNES_MUTATION_DIVIDE included (it is set by
 * nicnes_set_mutation_divide_es): NICNES_ERR_UNSUPPORTED. Independent of nicnes_set_mutation. */
int nicnes_es_set_mutation(nicnes_handle* h, int32_t mode);
/* The ES mutation becomes NICNES_MUTATION_DIVIDE = SM-G-SUM / SM-VECTOR, delta'[j] = fp32(fp32(sigma z[j]) / s_p[j])
 * (IEEE division, the arithmetic of nicnes_set_mutation's divide) with s_p the sensitivity of the pair's own parent
 * (nicnes_sensitivity_es, nicnes_set_sensitivity_es). nicnes_es_evaluate, nicnes_es_offspring and nicnes_es_advance
 * then fail with NICNES_ERR_INVALID, before anything is enqueued, when a parent they name has no valid sensitivity
 * (nicnes_es_advance checks every entry of parent_of_host: the survivors are known only on the device).
 * nicnes_es_set_mutation leaves the mode again. */
int nicnes_set_mutation_divide_es(nicnes_handle* h);
/* The SM-G-SUM sensitivity of each named slot of the CURRENT parent table (Sensitivity.calc_sensitivity, cached by the
 * reference per (task_id, parent_id), safe_mutations.py:34-84): what nicnes_sum_sensitivity computes for the handle's
 * theta (the same kernels, on the first `rows` images of the batch held, with the underflow clamp), for
 * theta = parent row slot, into row slot of a sensitivity table [max_parents, Dp] fp32, which becomes valid. The slots
 * run one after the other on `stream`. slots_host [n_slots] (HOST). The table is allocated at the first call
 * (synchronising then; its pad columns [D, Dp) are written 1.0 once); afterwards the call only enqueues.
 * NICNES_ERR_INVALID: a slot outside [0, parent count), rows outside [1, B], underflow <= 0, no batch held.
 * NICNES_ERR_UNSUPPORTED: rows > 819 (nicnes_sum_sensitivity's limit), before anything is allocated or enqueued.
 * A row stops being valid when nicnes_es_set_parent rewrites its slot, and every row does at nicnes_es_advance (the
 * tables swap). Leaves shared mode (below). */
int nicnes_sensitivity_es(nicnes_handle* h, const int32_t* slots_host, int32_t n_slots, int32_t rows, float underflow,
                          void* stream);
/* slot >= 0: row `slot` of the sensitivity table <- vec_dev [D] fp32 (device), valid from then (tests, resuming).
 * slot = -1: vec_dev is ONE vector every parent shares (SM-VECTOR, Sensitivity.set_sensitivity): the handle keeps one
 * copy, which the kernels read with row stride 0, and which stays valid over nicnes_es_set_parent and
 * nicnes_es_advance, until a per-parent call (this one with slot >= 0, or nicnes_sensitivity_es) leaves shared mode. */
int nicnes_set_sensitivity_es(nicnes_handle* h, int32_t slot, const float* vec_dev, void* stream);
/* out_dev [D] fp32 (device) <- the slot's sensitivity row, or the shared vector for any slot in shared mode.
 * NICNES_ERR_INVALID when the slot has none. */
int nicnes_get_sensitivity_es(nicnes_handle* h, int32_t slot, float* out_dev, void* stream);
/* Parent row `slot` of the current table <- theta32 [D] fp32 (device), and its statistics; the parent count is set
 * apart (slots [0, count) are the parents an evaluate may name). Replaces ESIteration.init_parents / the parent paths
 * of ESTask (nic_es_master.py:27-34). */
int nicnes_es_set_parent(nicnes_handle* h, int32_t slot, const float* theta32, void* stream);
int nicnes_es_set_parent_count(nicnes_handle* h, int32_t count);
/* A row back: table 0 = the current parents, 1 = the elites; theta32_out [D] fp32 (device). */
int nicnes_es_get_row(nicnes_handle* h, int32_t table, int32_t slot, float* theta32_out, void* stream);
/* The row's statistics as the mutation uses them (synchronising): fp32 mean|theta| and the count of exact zeros. */
int nicnes_es_row_stats(nicnes_handle* h, int32_t table, int32_t slot, float* mean_abs_out_host,
                        int64_t* zeros_out_host, void* stream);
/* Evaluate pairs [pair_begin, pair_begin + count) of `generation`: replaces ESWorker.fitness
 * (src/algorithm/nic_es/nic_es_worker.py) for a slice of the offspring. parent_of_host [count] (HOST, copied): the
 * parent slot of each pair of the slice; member_batch_host as in nicnes_evaluate_batches (nullable); fitness_out
 * [count, 2] fp64 = the fitness of offspring (2k, 2k + 1); seq_out [count, 2, B, seq_length] int32 and logprob_out
 * likewise fp32, both nullable. The fused decode (128-row slabs, one workgroup per pair and slab) unless
 * nicnes_set_decode_es says otherwise: a shape forced by nicnes_set_decode_split other than (1, 4), and the sampled
 * fitness modes, are NICNES_ERR_UNSUPPORTED. Screening follows nicnes_set_decode_screen as in nicnes_evaluate, on the
 * fused path only. Only enqueues. */
int nicnes_es_evaluate(nicnes_handle* h, uint64_t generation, int32_t pair_begin, int32_t count, float sigma,
                       const int32_t* parent_of_host, const int32_t* member_batch_host, double* fitness_out,
                       int32_t* seq_out, float* logprob_out, void* stream);
/* The decode path of nicnes_es_evaluate (not a reference interface: ESWorker.fitness decodes one offspring per CPU
 * process, nic_es_worker.py). mode 0 (the default): always the fused decode. mode 1: automatic, the coop path (the split
 * shape of 128-row slabs in one persistent launch, nicnes_set_decode_coop) where the handle's own shape rule
 * (nicnes_decode_shape) picks G = 4 with S = 2 or 4 for (B, count) and the grid fits the GPU at once, as for a rank's
 * share of a generation (62-63 pairs of mscoco_es.json's 500 at 8 ranks); otherwise fused, never the split path or
 * 64-row slabs. mode 2: the coop path with the given S (2 or 4; S is 0 in the other modes): an evaluate whose count x
 * slabs x S workgroups exceed occupancy x CUs, or issued while nicnes_set_decode_coop(h, 0) holds, fails with
 * NICNES_ERR_INVALID before anything is enqueued. Grows the partial-state scratch as nicnes_set_decode_split does
 * (synchronising then). Tokens and greedy fitness do not depend on the path; the coop path never screens. */
int nicnes_set_decode_es(nicnes_handle* h, int32_t mode, int32_t S);
/* The path an ES evaluate of `count` pairs of a B-image batch would take under the current mode: 0 fused, 2 coop (the
 * counterpart of nicnes_decode_path; needs no batch, decodes nothing). Fails as that evaluate would under mode 2. */
int nicnes_decode_path_es(nicnes_handle* h, int32_t B, int32_t count, int32_t* out_host);
/* The gather of a generation's fitness over the ranks of the bound communicator: replaces ESMaster.run_master collecting
 * the workers' ESResults (nic_es_master.py:92-113). The ranks evaluate the balanced shards of nicnes_math.h nn_es_shard
 * (the first n_pairs % ranks ranks hold n_pairs / ranks + 1 pairs, the rest n_pairs / ranks; contiguous, in rank order).
 * fit_local [count_local, 2] fp64 (device), this rank's shard; fit_all [n_pairs, 2] fp64 (device) in pair order on every
 * rank: the shards are padded to the largest share in the handle's scratch, gathered with one ncclAllGather and
 * compacted on the device. NICNES_ERR_INVALID when count_local is not this rank's share of n_pairs or n_pairs is
 * below the rank count. Only enqueues (the scratch is allocated at the first call). Needs nicnes_es_create. */
int nicnes_allgather_fitness_es(nicnes_handle* h, const double* fit_local, int32_t count_local, int32_t n_pairs,
                                double* fit_all, void* stream);
/* One offspring's parameters, fp32(theta_parent +- delta') exactly as the decode forms them: theta32_out [D] fp32
 * (device). sign 0: +, 1: -. What ESWorker writes to its offspring .pth (for tests, the wire and snapshots). */
int nicnes_es_offspring(nicnes_handle* h, uint64_t generation, int32_t pair, int32_t sign, float sigma, int32_t parent,
                        float* theta32_out, void* stream);
/* Truncation selection (the sort of ESMaster.run_master, nic_es_master.py): fitness [n] fp64 (device; a generation's
 * [pairs, 2] ravelled, n <= 2 max_members) -> order_out [n_keep] int32 (device) = the offspring ids in descending
 * fitness, ties to the lower id, NaN last, -0 equal to +0. n_keep outside [1, n]: NICNES_ERR_INVALID. Only enqueues. */
int nicnes_es_select(nicnes_handle* h, const double* fitness, int32_t n, int32_t n_keep, int32_t* order_out,
                     void* stream);
/* The next generation's parents (ESIteration.record_parents): the other table's rows [0, n_front) <- elite rows
 * [0, n_front), rows n_front + i <- offspring order[i] of `generation` (order [n_keep] int32, device, as
 * nicnes_es_select wrote it; parent_of_host [n_pairs] the parent slots of ALL pairs of the generation, so every rank
 * holding the gathered fitness advances identically whatever shard it evaluated). The rows' statistics are refreshed,
 * the tables swap and the parent count becomes n_front + n_keep. Only enqueues. */
int nicnes_es_advance(nicnes_handle* h, uint64_t generation, float sigma, const int32_t* parent_of_host, int32_t n_pairs,
                      const int32_t* order, int32_t n_keep, int32_t n_front, void* stream);
/* Elite row elite_slot <- row `slot` of `table` (0: the current parents, a new elite, Podium.record_elites' copy of the
 * .pth; 1: the elites, an elite moving down the podium) with its statistics. */
int nicnes_es_set_elite(nicnes_handle* h, int32_t elite_slot, int32_t table, int32_t slot, void* stream);
/* The handle's theta <- a row (table 0 parents, 1 elites), a device copy, so that nicnes_split_evaluate /
 * nicnes_evaluate_theta validate an elite candidate (ESMaster's accuracy_on of the elite .pth). */
int nicnes_es_load_theta(nicnes_handle* h, int32_t table, int32_t slot, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NICNES_H */
