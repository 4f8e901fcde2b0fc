// Internal (non-ABI) launch interfaces of the engine's kernels.
#pragma once
#define SCR_SLOTS (64 + 64 + 64 + 1 + 64)   // per lane: c | h' | x of t = 0 | unfinished | h' (odd parity, split path)
#define PART_FLOATS (8 * 7 * 64)             // split path: partial greedy state of one logit workgroup (8 waves x 7 x 64 lanes)
#define COOP_CTR_STRIDE 32                   // coop path: uint32 per member-slab hand-off counter (its own 128-byte line)
#define SCREEN_CAP_WORDS(V1) ((size_t)(((V1) + 63) / 64) * 512)   // screened decode: one word per 64-row stage and thread
#include <hip/hip_runtime.h>
#include <stdint.h>

struct DecodeParams {
    const float* theta;          // base theta, fp32 [D] (flat order: SURVEY.md Appendix A.1)
    const float* noise;          // the sigma-scaled table fp32(sigma * z) [noise_len], or a mutation's delta' rows
    const uint64_t* noise_idx;   // per member slice start (multiple of 64)
    const float* fc;             // unique-image fc features [images, F]
    const int32_t* member_batch; // nullable: member k of the launch decodes images member_batch[k] * B .. + B
    int32_t* seq;                // out: [members, 2, B, T] greedy tokens (masked after the first 0)
    float* lp;                   // out (nullable): [members, 2, B, T] log-prob of the picked token (nets.py:208,225,241)
    const double* sample_u;      // nullable: sampled decode (nets.py:210-231, fused path only): the uniform of
                                 // every (member, sign, row, logit step) [members, 2, B, T]; NULL = greedy
    float* scratch;              // nicnes_decode_scratch_floats(): lane-private c | h' | x0 | unfinished | h' (odd)
    int32_t* stats;              // [0] exact-pass fallbacks (atomic), [1] sampled re-walks, [2] coop (and step queue) timeouts,
                                 // [3] sampled workgroups that found no free logit slot
    float* slog;                 // sampled steps kernel: slog_ns logit slots of nst * 16384 floats (> one per resident
                                 // workgroup): the logit loop stores each step's logits there, the pick reads them
    int32_t* slog_slots;         // slog_ns claim flags (0 free), zero between launches
    int32_t slog_ns;
    int32_t* alive;              // fused path: [members * slabs], 0 once every row of the workgroup finished
    int32_t* alive2;             // split path: [2][alive_stride] by step parity
    float* part;                 // split path: [members * slabs * S] x PART_FLOATS partial greedy states
    uint32_t* coop_ctr;          // coop path: [members * slabs] x 32 hand-off counters (zeroed per launch)
    int32_t coop;                // 1: the split shape (G = 4, S = 2 or 4) in one persistent launch
    int32_t coop_launch;         // coop path: 1 hipLaunchCooperativeKernel (the runtime checks the grid is resident
                                 // at once and fails the launch otherwise), 0 a plain launch of a grid the engine
                                 // bounded by the same occupancy query (the default: same residency, no launch cost)
    uint32_t test_stall_ms;      // test hook (NICNES_TEST_COOP_STALL): coop workgroup 0 starts this late, past the
                                 // partners' spin bound, so they time out (0 = off)
    int32_t no_exit;             // 1: no per-slab early exit (log-probs of a multi-slab batch, see below)
    int32_t no_mask;             // 1: feed every argmax back unmasked (forward_for_sensitivity); fused, split, coop
    int32_t force_exact;         // test hook (NICNES_FORCE_EXACT=1): every step takes the exact tie pass
    float lse_margin;            // widening of the bounded-lse interval: 2e-3 (test hook NICNES_LSE_MARGIN)
    int32_t bounded_lse;         // 1: greedy-only decode with the pair-bounded lse (needs lp == NULL)
    int32_t B, F, V1, T;         // B: rows decoded per sign and slab range
    int32_t B_img;               // images per batch in fc / the member_batch stride (= B, or the whole batch below)
    int32_t sign_off;            // 0; > 0 (the sigma = 0 rollout decoded once): sign s decodes rows s * sign_off + b,
                                 // b < B, valid while < B_img * rpi, and its rows land at s * B + b of one [2B, T] rollout
    int32_t rpi;                 // rows per image (sampled modes: the reference's seq_per_img copies): row r reads
                                 // fc row r / rpi
    int32_t G;                   // row groups per slab: 4 (128-row slabs) or 2 (64-row slabs)
    int32_t S;                   // logit workgroups per member slab (1 + G = 4: the fused step kernel)
    int32_t alive_stride;
    int64_t D;
    int64_t off_img_w, off_img_b, off_emb_w, off_log_w, off_log_b, off_i2h_w, off_i2h_b, off_h2h_w, off_h2h_b;
};

// The screened decode's own arguments (the screened kernels' second argument: DecodeParams, and with it every other
// kernel's argument layout and machine code, stays as it is). cap == NULL: no screening.
struct ScreenArgs {
    uint32_t* cap;               // [members * slabs] capture slots of SCREEN_CAP_WORDS(V1) words: [stage][thread]
    float* norm;                 // [members][4]: max_v |w+_v|^2, max_v |w-_v|^2, max_v |b+_v|, max_v |b-_v| of the
                                 // member's logit rows (nicnes_screen_norm_kernel, before the decode)
    float scale;                 // >= 1, multiplies eps (test hook NICNES_SCREEN_EPS_SCALE)
    unsigned long long* ctr;     // SCREEN_CTR_WORDS counters (atomic): [0] candidate ids captured, [1] rows the first
                                 // certify round left bad; of those [2] with a lane over the cap, [3] with a record
                                 // between the tie windows, [4] with an evicted record in the window, [5] with a
                                 // non-finite bound (or force_exact); [6] rows of [1] that later rounds settled, [7] rows
                                 // that went to the fp32 loop, [8] workgroup steps that ran it; [9 + k] over-cap rows
                                 // whose fuller lane holds 8 (k + 1) + 1 .. 8 (k + 2) hit weights (k = 7: or more);
                                 // [17] waves that ran the fp32 loop (of the 8 of each workgroup step of [8])
    int32_t rounds;              // round budget R: a lane may hold up to 8 R hit weights and still be certified in
                                 // rounds (NICNES_SCREEN_ROUNDS; 1: none after the first). It bounds the weight, not
                                 // the count: packing crowded hits (weight 4) can take a lane one round more than R
};
#define SCREEN_CTR_WORDS 18
#define SCREEN_ROUNDS_DEFAULT 2
#define SCREEN_ROUNDS_MAX 64

// The step queue of the screened fused decode (nicnes_decode_steps_screen_queue_kernel's third argument; ring == NULL:
// the one-launch kernel, one workgroup per member slab). `workers` persistent workgroups take (member slab, step) tasks
// from a bounded FIFO ring; ScreenArgs::cap then holds one capture slot per worker, not per member slab.
struct QueueArgs {
    unsigned long long* ring;    // [slots] (slots a power of two >= the launch's member slabs): sequence << 32 | task,
                                 // task = member slab | (t + 1) << QUEUE_STEP_SHIFT
    uint32_t* ctl;               // QUEUE_CTL_WORDS control words (below)
    int32_t slots;
    int32_t workers;             // workgroups of the launch (the grid is min(member slabs, workers))
};
#define QUEUE_STEP_SHIFT 20      // member slabs < 2^20, steps t + 1 < 2^12
#define QUEUE_HEAD 0             // ctl: the ring's push position, the pop position and the finished member slabs, each on
#define QUEUE_TAIL 32            // a 128-byte line of its own (set before every launch); then the counters that keep
#define QUEUE_DONE 64            // counting over launches: tasks run, waits that ran past QUEUE_SPIN_TICKS
#define QUEUE_GRID 65            // the launch's workers (each ends on one unfilled ticket: tail = head + workers)
#define QUEUE_STEPS 96
#define QUEUE_TIMEOUTS 97
#define QUEUE_CTL_WORDS 128
// the host's rules (pure: tests/test_step_queue_host.py through nicnes_decode_queue_plan)
static inline int32_t nicnes_queue_ring_slots(int64_t items) {
    int32_t n = 1;
    while (n < items && n < (1 << QUEUE_STEP_SHIFT)) n <<= 1;
    return n;
}
// mode 0 off, 1 on, 2 auto: more member slabs than workers (at or below, the one-launch kernel has every member slab
// resident at once and nothing to level)
static inline bool nicnes_queue_use(int mode, int64_t items, int workers) {
    if (items < 1 || items > (1 << QUEUE_STEP_SHIFT) || workers < 1) return false;
    return mode == 1 || (mode == 2 && items > workers);
}

// A mutated decode on the fused greedy path (mode != 0; the kernels' second argument, so the other kernels' argument
// layout is untouched): the delta' rows in DecodeParams::noise hold only the parameters from off_log_w on (logit, i2h,
// h2h: re-read at every step); the image projection and the embedding rows (read once, and only for the tokens taken)
// form delta' = fp32(sigma z) / s (mode 1: SM-G-SUM / SM-VECTOR) or fp32(sigma z) * s (mode 2: SM-PROPORTIONAL)
// themselves, from the sigma-scaled table slice at head_idx[member] and the mutation vector
struct MutHead {
    const float* head_noise;
    const uint64_t* head_idx;
    const float* mut_vec;
    int32_t mode;
};

// nic_es (the *_es kernels' second argument; DecodeParams and every other kernel stay as they are): member k of the
// launch perturbs its own base theta, row parent_of[k] of the parent table, instead of DecodeParams::theta
struct ParentArgs {
    const float* parents;        // fp32 [max_parents, stride]
    const int32_t* parent_of;    // [members] parent slot of each member of the launch
    int64_t stride;              // Dp: D rounded up to 64 floats
};

// launch kinds recorded next to the timing events
#define DK_IMG 0
#define DK_STEP 1        // fused step kernel (logits of t + cell of t + 1)
#define DK_STEPS 4       // fused path, every step in one launch (nicnes_decode_steps_kernel)
#define DK_CELL 2        // split path: token merge of t + cell of t + 1
#define DK_LOGIT 3       // split path: logits of t over one vocabulary range
#define DK_COOP 5        // coop path: every step of the split shape in one launch
#define DK_STEPS2 6      // fused path of 64-row slabs (G = 2, S = 1), every step in one launch

// evs (nullable): up to DECODE_MAX_EVENTS events, recorded before the first launch and after every
// launch; kinds[k] (k >= 1) is the kind of the launch that event k follows. Returns the launch count
// in *n_launch.
#define DECODE_MAX_EVENTS 64
extern "C" hipError_t nicnes_decode_init();
// workgroups of the coop kernels (min over their instantiations) and of the sampled steps kernel one CU holds at
// once (hipOccupancyMaxActiveBlocksPerMultiprocessor at their LDS): the coop grid must fit occ x CUs, the sampled
// logit slots must outnumber occ x CUs
extern "C" hipError_t nicnes_decode_occupancy(int* coop_per_cu, int* sample_per_cu);
// shifts the per-member and per-workgroup pointers of *p to member m0 (a decode of members m0.. on
// its own stream; nslabs = the launch's row slabs)
extern "C" void nicnes_decode_shift(DecodeParams* p, int m0, int nslabs, MutHead* mh, ScreenArgs* sa = nullptr,
                                    ParentArgs* pa = nullptr);
// nic_es: the fused greedy decode (G = 4, S = 1, no sampling, no decode-formed delta') of members with their own base
// theta (ParentArgs); screened when sa has its buffers and the decode is greedy-only with the bounded lse
// With p->coop (G = 4, S = 2 or 4, coop_ctr set): the coop path's one persistent launch on the *_es entries (counters
// zeroed first, p->coop_launch and p->test_stall_ms as in nicnes_launch_decode; never screened)
extern "C" hipError_t nicnes_launch_decode_es(const DecodeParams* p, const ParentArgs* pa, int member_count, int nslabs,
                                              hipStream_t stream, const ScreenArgs* sa = nullptr);
// mh: nullable (or mode 0): no decode-formed delta'
extern "C" hipError_t nicnes_launch_decode(const DecodeParams* p, const MutHead* mh, int member_count, int nslabs,
                                           hipStream_t stream, hipEvent_t* evs, int* kinds, int* n_launch,
                                           const ScreenArgs* sa = nullptr,    // sa: nullable (or cap NULL): the fp32 loop
                                           const QueueArgs* qa = nullptr);    // qa: nullable (or ring NULL): no step queue;
                                                                              // else the screened decode runs from it
// zero seq_logprobs past the batch's last finishing step (rollouts = members x 2 of B rows; after a
// no_exit decode of a batch spanning several slabs)
extern "C" hipError_t nicnes_launch_lp_batch_exit(const int32_t* seq, float* lp, int rollouts, int B, int T,
                                                  hipStream_t stream);
// test entry (nicnes_test_logit_chain): the logits of the member slice at nidx, sign sgn, over hin [32, 128], by the
// 32-row MFMA tile path and by the fmaf chain; reads theta, noise, scratch (one wave's lane scratch), V1, D, off_log_w, off_log_b of *p
extern "C" hipError_t nicnes_launch_test_logit_chain(const DecodeParams* p, uint64_t nidx, int sgn, const float* hin,
                                                     float* out_mfma, float* out_chain, hipStream_t stream);
// test entry (nicnes_test_certify_items): the items (grouped by owner lane: lane_start [257], group 2 row + lane half;
// ids, pos_of their positions in out) of sign sgn over hin [128, 128] through the screened decode's tile certify, one
// workgroup; scratch holds eight waves' lane scratch
extern "C" hipError_t nicnes_launch_test_certify_items(const DecodeParams* p, uint64_t nidx, int sgn, const float* hin,
                                                       const int32_t* lane_start, const int32_t* ids,
                                                       const int32_t* pos_of, float* out, hipStream_t stream);
// beam-search decode (beam_kernels.hip) of theta over `count` images from p->fc, beam width K in 1..8, one launch: seq
// [count, T] and score [count] (the fp64 sum of the winner's log-probs); reads theta, fc, F, V1, T, D and the offsets
// of *p. xscr: nicnes_beam_scratch_floats(count, K) floats of lane-private scratch.
extern "C" size_t nicnes_beam_scratch_floats(int count, int K);
// n_cu: the device's CUs (the launch takes 4-wave workgroups instead of 8-wave ones while that costs fewer rounds);
// force_nw: 4 or 8 waves per workgroup whatever the range (nicnes_set_beam_waves), 0 the rule
extern "C" int nicnes_beam_waves_per_wg(int count, int K, int n_cu);
extern "C" hipError_t nicnes_launch_beam_decode(const DecodeParams* p, int32_t* seq, double* score, float* xscr, int count,
                                                int K, int n_cu, int force_nw, hipStream_t stream);
// test entry (nicnes_test_beam_select): the decode's per-lane top-K and selection over given log-prob rows
// [n_img, K, V1], scores and live flags [n_img, K]; out [n_img, K, 2] (row of the image, id), pre-filled with -1
extern "C" hipError_t nicnes_launch_test_beam_select(const float* lp, const double* score, const int32_t* live, int n_img,
                                                     int K, int V1, int32_t* out, hipStream_t stream);
// the wide greedy decode (decode_wide_kernels.hip): E = input_encoding_size, R = rnn_size, each in {128, 256, 384, 512};
// one launch of member_count x nslabs workgroups (p->G == 4, p->S == 1, greedy, no MutHead), exact exp-sum. One step-loop
// frame, two cells: the plain LSTM cell, or with ln != 0 the layer-norm cell of layer_n models (decode_ln_kernels.hip),
// whose lane scratch is larger. tail6: the theta offsets of the six affine tensors (i2h_ln weight, bias, h2h_ln weight,
// bias, c_ln weight, bias), NULL without layer_n_affine. p->scratch holds nicnes_wide_scratch_floats(member_count * nslabs,
// E, R, ln) floats. evs / kinds / n_launch as nicnes_launch_decode (one launch, kind DK_STEPS). nicnes_decode_wide_init:
// per device, once per handle (the dynamic LDS of both kernels and of the test entry below is above 64 KB).
extern "C" hipError_t nicnes_decode_wide_init();
extern "C" size_t nicnes_wide_scratch_floats(int64_t workgroups, int E, int R, int ln);
extern "C" hipError_t nicnes_launch_decode_wide(const DecodeParams* p, int E, int R, int ln, const int64_t* tail6,
                                                int member_count, int nslabs, hipStream_t stream, hipEvent_t* evs,
                                                int* kinds, int* n_launch);
// test entry (nicnes_test_ln_cell): one layer-norm cell of theta itself (p->noise: D zeros) on rows <= 128 given rows
// xin [rows, E], hin [rows, R], cin [rows, R] by the decode's device function; p->scratch holds one workgroup's lane scratch
extern "C" hipError_t nicnes_launch_test_ln_cell(const DecodeParams* p, int E, int R, const int64_t* tail6,
                                                 const float* xin, const float* hin, const float* cin, int rows,
                                                 float* hout, float* cout, hipStream_t stream);
// the teacher-forced forward (xent_kernels.hip): log-probs of label rows under theta +- delta, E = R = 128 only
struct XentArgs {
    const int32_t* labels;         // [rows held, T] label rows: word ids, 0-padded
    const int32_t* row_img;        // [rows held] the image (row of p.fc) of each label row, ascending
    const int32_t* img_ref_start;  // batches: [images + 1] (the batch's rows: start[k B_img] .. start[(k + 1) B_img]); or NULL
    double* lp_sum;                // out: batches [members, 2, max_rows]; flat [row1 - row0]
    int32_t* n_tok;                // out, likewise
    float* lp_steps;               // out (nullable), likewise x (T + 1): lp_s of the counted targets (the host zeroes it)
    int32_t n_img;                 // rows of p.fc
    int32_t row0, row1;            // the flat range
    int32_t max_rows;              // batches: the outputs' row stride
};
// nicnes_xent_init: per device, once per handle (the kernel's dynamic LDS is above 64 KB)
extern "C" hipError_t nicnes_xent_init();
extern "C" size_t nicnes_xent_scratch_floats(int64_t workgroups);
// row_img[r] = the image whose reference range [img_ref_start[i], img_ref_start[i + 1]) holds row r
extern "C" hipError_t nicnes_launch_xent_row_map(const int32_t* img_ref_start, int n_img, int32_t* row_img,
                                                 hipStream_t stream);
// one launch of members x nslabs workgroups (a flat range: members pseudo-members, nslabs 1), then the n_cand
// candidates' fitness = sum lp_sum / sum n_tok in a fixed fp64 order (each nullable: fitness, tokens = their sum n_tok,
// loss2 = {loss, exp(loss)} of candidate 0). Reads theta,
// noise, noise_idx, fc, member_batch, B_img, scratch (nicnes_xent_scratch_floats(members * nslabs)), F, V1, T, D and
// the offsets of *p
extern "C" hipError_t nicnes_launch_xent(const DecodeParams* p, const XentArgs* xa, int members, int nslabs, int n_cand,
                                         double* fitness, long long* tokens, double* loss2, hipStream_t stream);
// lane scratch for up to member_count members x row_waves 32-row waves of one sign
extern "C" size_t nicnes_decode_scratch_floats(int member_count, int row_waves_per_member);
