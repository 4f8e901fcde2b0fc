// engine.cpp -- the C ABI of libnicnes (include/nicnes.h): handle state, validation, launches.
//
// Host-side orchestration only; the arithmetic lives in decode_kernel.hip, cider_kernel.hip and
// update_kernels.hip. Nothing here allocates or synchronises inside nicnes_evaluate /
// nicnes_grad_partial / nicnes_rank_weights, so a caller may capture them in a hipGraph.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>

#include <rccl/rccl.h>

#include "../../include/nicnes.h"
#include "../../include/nicnes_math.h"
#include "cider_kernel.h"
#include "decode_kernel.h"
#include "update_kernels.h"
#include "sensitivity.h"
#include "trainset_kernels.h"
// the resident training set's two gather kernels and their launchers live in this translation unit (so the library
// keeps its five code objects), ahead of this file's own kernels, whose machine code and order stay as they were
#include "trainset_kernels.hip"

#define SCREEN_DEFAULT 2   // the bf16-screened logit loop of the fused greedy-only decode: 0 off, 1 on,
                           // 2 automatic: on when the decode has more workgroups than the GPU has CUs
#define MB_RING 4   // pinned staging slots of the member -> batch map (nicnes_evaluate_batches)
#define DR_RING 4   // pinned staging slots of a draw's image indices and reference starts (nicnes_draw_batches)

// Work of the teacher-forced forward (xent_kernels.hip), grown to the largest launch: lane scratch of `wgs` workgroups,
// the per-row outputs of `rows` candidate rows, zero slice indices of `pms` pseudo-members (theta itself over a flat
// range). The handle holds one set (its last XENT evaluate's rows stay readable) and every split its own.
struct XentWork {
    float* scratch = nullptr;
    int64_t wgs = 0;
    double* lp_sum = nullptr;
    int32_t* n_tok = nullptr;
    int64_t rows = 0;
    uint64_t* zero_idx = nullptr;
    int32_t pms = 0;
    double* out = nullptr;            // [4]: fitness | loss, perplexity | sum n_tok (as int64)
};

struct nicnes_handle {
    nicnes_config cfg;
    int device = 0;
    std::string err;
    int64_t off[10];
    int64_t D = 0;
    int32_t V1 = 0;

    const float* noise = nullptr;
    uint64_t noise_len = 0;

    double* theta64 = nullptr;
    float* theta32 = nullptr;
    double* m = nullptr;
    double* v = nullptr;
    int64_t t = 0;
    int theta_is_fp32 = 0;
    bool theta_set = false;

    const float* fc = nullptr;
    int32_t B = 0;                    // rows (images) decoded per member
    int32_t n_batches = 1;            // batches held (single_batch: false holds several)
    int32_t n_img = 0;                // images held = n_batches * B
    int32_t img_cap = 0;              // per-image CIDEr-D table capacity
    int32_t* mbatch = nullptr;        // [max_members] member -> batch map of the current evaluate
    // the caller's host map is staged in a ring of pinned buffers (each reused only after its copy has
    // run, told by its event), so an evaluate with a map never waits for the queued GPU work
    int32_t* mb_pin[MB_RING] = {};
    hipEvent_t mb_ev[MB_RING] = {};
    bool mb_used[MB_RING] = {};
    int mb_next = 0;
    int32_t n_refs = 0;
    const int32_t* img_ref_start = nullptr;
    const int32_t* ref_tokens = nullptr;   // the batch's reference rows [n_refs, T] (nicnes_test_batch_state)
    bool batch_set = false;
    // the xent fitness: label rows = the reference rows held, each under its own image
    int32_t* x_row_img = nullptr;     // [max_refs] label row -> image (alloc_refs; built whenever a batch is set)
    std::vector<int32_t> x_row0;      // [n_batches + 1] first label row of every batch held (host)
    int32_t x_max_rows = 0;           // label rows of the largest batch held
    XentWork xw;
    std::vector<int32_t> x_last_rows; // the last XENT evaluate: label rows of every candidate (empty: none yet)
    int64_t x_last_stride = 0;        // ... and their row stride in xw.lp_sum / n_tok
    // nicnes_draw_batches: the batch buffers a draw gathers into (owned; h->fc, ref_tokens and img_ref_start point at
    // them after a draw), the device copy of the staged words and the pinned ring they travel through. A slot holds
    // [n_img] image indices then [n_img + 1] destination starts, and is reused only after its copy has run (its event)
    float* dr_fc = nullptr;           // [dr_img_cap, F]
    int32_t* dr_refs = nullptr;       // [dr_ref_cap, T]
    int32_t* dr_start = nullptr;      // [dr_img_cap + 1]
    int32_t* dr_stage = nullptr;      // [2 * dr_img_cap + 1]
    int32_t dr_img_cap = 0, dr_ref_cap = 0;
    int32_t* dr_pin[DR_RING] = {};
    size_t dr_pin_cap[DR_RING] = {};  // in int32 words
    hipEvent_t dr_ev[DR_RING] = {};
    bool dr_used[DR_RING] = {};
    int dr_next = 0;

    const uint64_t* df_keys = nullptr;
    const double* df_vals = nullptr;
    int64_t df_n = 0;
    uint64_t* hash_keys = nullptr;   // engine-owned open-addressing copy of the df table
    double* hash_vals = nullptr;
    uint64_t hash_mask = 0;
    double ref_len = 0.0;
    bool df_set = false;

    uint64_t* img_hkey = nullptr;     // per-image reference n-gram tables (CIDEr-D)
    int32_t* img_hrow = nullptr;
    double* img_vr = nullptr;
    bool img_tables = false;          // every image has <= IMG_MAXR references
    uint64_t* ref_keys = nullptr;
    double* ref_vec = nullptr;
    int32_t* ref_count = nullptr;
    int32_t* ref_len2 = nullptr;
    double* ref_norm = nullptr;

    uint64_t* nidx = nullptr;
    int32_t* seq = nullptr;
    float* lp = nullptr;              // per-step log-probs for the greedy_* criteria
    double* row_scores = nullptr;     // per-row CIDEr-D of the image-table scorer [2 * max_members, max_batch]
    int fitness_mode = 0;             // nicnes_set_fitness_mode (0 = 'greedy')
    double* su = nullptr;             // sampled modes: the draws of a decode [count, 2, B, T]
    double* base_scores = nullptr;    // self-critical modes: the greedy rows' CIDEr-D [2 count, B]
    int64_t su_cap = 0, base_cap = 0; // ... their capacities (doubles)
    float* slog = nullptr;            // sampled modes: logit slots of the steps kernel (one per resident workgroup + spare)
    int32_t* slog_slots = nullptr;    // ... their claim flags (zero between launches)
    int slog_ns = 0;
    std::vector<double> su_host;      // nicnes_set_sample_draws (test hook): draws to use instead of the engine's
    int rpi = 1;                      // nicnes_set_rows_per_image: rows the sampled modes decode per image
    float* dscratch = nullptr;
    unsigned long long* zcount = nullptr; // nicnes_theta_zeros: the count of exact zeros of theta32
    int32_t* stats = nullptr;
    int32_t* alive = nullptr;         // per decode workgroup: rows left unfinished (fused [stride], split [2][stride])
    int32_t alive_stride = 0;         // max decode workgroups (members x 64-row slabs)
    float* part = nullptr;            // split decode: partial greedy states
    float* noise_sc = nullptr;        // fp32(sc_sigma * table): what the decode kernels read (no multiply per use)
    float sc_sigma = 0.f;
    bool sc_valid = false;
    bool wide = false;                // E or R above 128 (or the test hook NICNES_DECODE_WIDE=1): every decode request goes
                                      // to the wide launcher (decode_wide_kernels.hip): 128-row slabs, one stream
    bool ln = false;                  // cfg.layer_n: a wide handle whose launch runs the layer-norm cell
                                      // (decode_ln_kernels.hip), at every width; ln_off: the six affine tensors' offsets
    bool ln_affine = false;           // cfg.layer_n_affine (with layer_n): theta carries the six tensors at its tail
    int64_t ln_off[6] = {0, 0, 0, 0, 0, 0};
    int mut_mode = 0;                 // nicnes_set_mutation: 0 plain, 1 divide, 2 multiply
    bool mut_full = false;            // NICNES_MUT_FULL=1: materialise every parameter's delta' (no decode-formed head)
    float* mut_vec = nullptr;         // [D] sensitivity (mode 1) or |theta| scale (mode 2)
    float* dbuf = nullptr;            // [max_members, Dp] the members' mutated deltas (mode != 0)
    uint64_t* didx = nullptr;         // [max_members] k * Dp: row offsets of dbuf
    int64_t Dp = 0;
    uint64_t* rank_key = nullptr;     // rank sort scratch (grown to the largest population ranked)
    uint32_t* rank_idx = nullptr;
    size_t rank_cap = 0;
    int64_t part_cap = 0;             // in logit workgroups (members x slabs x S)
    int n_cu = 256;
    int beam_waves = 0;               // nicnes_set_beam_waves: 4 or 8 waves per beam-decode workgroup, 0 the launch's rule
    int dec_S = 0, dec_G = 0;         // nicnes_set_decode_split (0 = automatic)
    // the decode's members in n parts on n streams (nicnes_set_decode_streams, NICNES_DECODE_STREAMS;
    // 0 = automatic: 2 on the split path, 1 on the fused path): one part's launches fill the CUs the
    // others' launch gaps and tails leave idle
    int dec_streams = 0;
    int coop_mode = 1;                // nicnes_set_decode_coop: 0 never, 1 the split shape in one launch when it fits
    int coop_occ = 1;                 // coop kernel workgroups resident per CU (occupancy API): the grid bound
    int sample_occ = 1;               // sampled steps kernel workgroups resident per CU: the logit slots needed
    // NICNES_COOP_LAUNCH=1: hipLaunchCooperativeKernel for the coop kernel. The default plain launch gets the same
    // residency from the same occupancy-bounded grid (coop_fits; MI355X_MICROARCH.md: the cooperative launch adds
    // only the runtime's check of that bound) and costs 0.4 % less per iteration at P = 64 (r04 A/B)
    int coop_launch = 0;
    int es_dec_mode = 0, es_dec_S = 0; // nicnes_set_decode_es: 0 fused, 1 automatic, 2 coop with es_dec_S
    uint32_t test_stall_ms = 0;       // test hook NICNES_TEST_COOP_STALL (ms): coop workgroup 0 starts late
    int test_stall_left = -1;         // ... on the first NICNES_TEST_COOP_STALL_LAUNCHES coop launches only (-1: all)
    int test_slots = 0;               // test hook NICNES_TEST_SLOTS: this many sampled logit slots (0 = enough)
    uint32_t* coop_ctr = nullptr;     // [max_members * slabs * COOP_CTR_STRIDE] coop hand-off counters
    SensWork* sens = nullptr;         // SM-G-SUM sensitivity work buffers (nicnes_sum_sensitivity)
    float* zero_noise = nullptr;      // [D] zeros + one zero index: the sigma = 0 decode of the sensitivity
    uint64_t* zero_idx = nullptr;
    int32_t* sens_tok = nullptr;      // [2 * max_batch * 4] its greedy tokens
    hipStream_t sx[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr;
    hipEvent_t ev_join[3] = {nullptr, nullptr, nullptr};
    double* partials = nullptr;
    double* norms = nullptr;

    ncclComm_t comm = nullptr;        // population shards over ranks (nicnes_comm_init / _attach)
    bool comm_owned = false;
    int comm_nranks = 1;

    bool timing = false;
    int force_exact = 0;      // test hook: exact tie pass on every step (NICNES_FORCE_EXACT=1)
    float lse_margin = 2e-3f; // bounded-lse margin; test hook NICNES_LSE_MARGIN widens it (more undecided rows)
    // bounded-lse policy: greedy-only decodes use the pair-bounded lse unless the previous bounded decode
    // sent rows to the exact pass (peaked, trained-model logits put lse near binade edges); then the
    // next exact_span decodes sum the exp exactly. The fallback counter is read back asynchronously.
    int bounded_mode = 2;     // NICNES_BOUNDED_LSE: 0 never, 1 always, 2 adaptive
    int screen_mode = SCREEN_DEFAULT;  // NICNES_SCREEN / nicnes_set_decode_screen: the fused greedy-only decode screens in bf16
    float screen_scale = 1.0f;         // test hook NICNES_SCREEN_EPS_SCALE (>= 1)
    uint32_t* screen_cap = nullptr;    // capture slots of screen_wgs workgroups (allocated at the first screened decode)
    int64_t screen_wgs = 0;
    float* screen_norm = nullptr;      // [max_members][4]
    unsigned long long* screen_ctr = nullptr;   // [SCREEN_CTR_WORDS] (ScreenArgs::ctr)
    int screen_rounds = SCREEN_ROUNDS_DEFAULT;  // NICNES_SCREEN_ROUNDS: certify rounds of an over-cap lane (ScreenArgs::rounds)
    int queue_mode = 2;                // NICNES_DECODE_QUEUE / nicnes_set_decode_queue: the screened decode's step queue
    int queue_workers = 0;             // NICNES_DECODE_QUEUE_WORKERS: its workers (0: one per CU)
    unsigned long long* queue_ring = nullptr;   // [queue_slots] (QueueArgs::ring; allocated with the screening buffers)
    uint32_t* queue_ctl = nullptr;     // [QUEUE_CTL_WORDS]
    int32_t queue_slots = 0;
    int exact_left = 0;
    int last_bounded = 0;
    int last_decode_bounded = 0;      // nicnes_last_decode_lse: the lse mode of the last decode enqueued
    int32_t fb_seen = 0;
    int32_t* stats_host = nullptr;
    hipEvent_t stats_ev = nullptr;
    bool stats_pending = false;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    hipEvent_t dev[DECODE_MAX_EVENTS] = {};   // between the decode's launches (phase split)
    int dev_kind[DECODE_MAX_EVENTS] = {};     // kind of the launch each event follows (DK_*)
    int n_dev = 0;                            // events recorded by the last timed decode
    bool multi_stream = false;                // the last decode ran on several streams
    bool last_nes_form = true;                // the newest optimizer step took the noise sum (not a globalg)
    // a skipped step (the Adam kernel's skip flag) leaves theta, m, v untouched; the host state it advanced
    // (t, theta_is_fp32) is rolled back once the flag is seen, so a re-run of the iteration steps as the first try would
    bool step_pending_check = false;
    int64_t t_prev = 0;
    int theta_fp32_prev = 0;
    std::vector<nicnes_split*> splits;        // resident evaluation splits (nicnes_split_create), freed with the handle
    std::vector<struct nicnes_trainset*> trainsets;   // resident training sets (nicnes_trainset_create), likewise
    struct nicnes_es* es = nullptr;           // nic_es state (nicnes_es_create), freed with the handle
};

// nic_es state: the parents of the generation being evaluated (ptab[cur]), the table the next generation is written
// to, the podium's elites, and each row's SM-PROPORTIONAL statistics.
struct nicnes_es {
    int32_t max_parents = 0, max_elites = 0, n_parents = 0;
    int64_t Dp = 0;
    int cur = 0;
    int mode = 0;                     // NICNES_MUTATION_PLAIN, _SCALE or _DIVIDE
    float* stab = nullptr;            // [max_parents, Dp] the current parents' sensitivity rows (nicnes_sensitivity_es;
                                      // allocated at the first use, pad columns 1.0)
    float* svec = nullptr;            // [Dp] the vector every parent shares (nicnes_set_sensitivity_es, slot -1)
    bool sens_shared = false;         // DIVIDE reads svec with row stride 0, not stab
    std::vector<uint8_t> sens_valid;  // [max_parents] row p of stab belongs to row p of ptab[cur]
    float* ptab[2] = {nullptr, nullptr};
    float* etab = nullptr;
    float* pmean[2] = {nullptr, nullptr};   // [max_parents] mean|theta_p| of the tables' rows
    int64_t* pzero[2] = {nullptr, nullptr}; // ... their exact zeros
    float* emean = nullptr;
    int64_t* ezero = nullptr;
    double* part_sum = nullptr;       // nicnes_es_stats_scratch(max rows)
    unsigned long long* part_zero = nullptr;
    int32_t* parent_of = nullptr;     // [max_members] device copy of an evaluate's / an advance's parent slots
    double* neg = nullptr;            // [2 max_members] select scratch
    float* dbuf = nullptr;            // [max_members, Dp] delta' rows (allocated at the first proportional evaluate)
    uint64_t* didx = nullptr;
    double* gat = nullptr;            // nicnes_allgather_fitness_es: this rank's padded share | every rank's
    size_t gat_cap = 0;               // ... in doubles
};

// A resident evaluation split (nicnes_split_create): N images' fc rows, their references cooked WITHOUT the end token
// against the split's own df table, and the work buffers of its one-call decode. Nothing here is shared with the
// handle's training batches, df table or evaluate buffers.
#define SPLIT_ROWS 128          // rows per sign of a pseudo-member: it decodes 2 * SPLIT_ROWS images
#define SPLIT_MAX_PM 4096       // pseudo-members of one decode (2^20 images, the bound of nicnes_set_batches)
struct nicnes_split {
    nicnes_handle* h = nullptr;
    int32_t N = 0, n_refs = 0;
    float* fc = nullptr;              // [N + 2 * SPLIT_ROWS, F]: the tail rows (zeros) are decoded and dropped
    int32_t* ref_tokens = nullptr;    // [n_refs, T]
    int32_t* img_ref_start = nullptr; // [N + 1]
    std::vector<int32_t> start_host;  // ... its host copy (nicnes_split_xent sizes its launch from it)
    int32_t* row_img = nullptr;       // [n_refs] label row -> image (nicnes_split_xent)
    XentWork xw;
    uint64_t* hash_keys = nullptr;    // the split's df table
    double* hash_vals = nullptr;
    uint64_t hash_mask = 0;
    double ref_len = 0.0;
    uint64_t* ref_keys = nullptr;     // cooked references (CiderTables)
    double* ref_vec = nullptr;
    int32_t* ref_count = nullptr;
    int32_t* ref_len2 = nullptr;
    double* ref_norm = nullptr;
    int32_t* img_stats = nullptr;     // per-image BLEU statistics [N, 10], ROUGE_L and CIDEr-D [N]
    double* img_rouge = nullptr;
    double* img_cider = nullptr;
    // decode work, grown to the largest range decoded: pm_cap pseudo-members (tokens, log-probs, lane scratch, alive
    // flags, coop counters, the zero slice index and the member -> image block map) and wg_cap logit workgroups
    int32_t pm_cap = 0;
    int64_t wg_cap = 0;
    int32_t* seq = nullptr;
    float* lp = nullptr;
    float* scratch = nullptr;
    int32_t* alive = nullptr;
    uint32_t* coop_ctr = nullptr;
    uint64_t* zero_idx = nullptr;
    int32_t* block = nullptr;
    float* part = nullptr;
    // beam decode work (nicnes_split_decode_beam), grown to the largest (count, beam) seen: tokens and scores of
    // beam_rows images, beam_scr floats of lane-private scratch
    int32_t beam_rows = 0;
    size_t beam_scr = 0;
    int32_t* beam_seq = nullptr;
    double* beam_score = nullptr;
    float* beam_xscr = nullptr;
};

// A resident training set (nicnes_trainset_create): every training image's fc row and raw reference rows on the
// device, and the host's copy of what a draw needs without asking the device: each image's reference count.
struct nicnes_trainset {
    nicnes_handle* h = nullptr;
    int32_t N = 0, n_refs = 0;
    float* fc = nullptr;              // [N, F]
    int32_t* ref_tokens = nullptr;    // [n_refs, T]
    int32_t* img_ref_start = nullptr; // [N + 1]
    std::vector<int32_t> count;       // [N] references per image (host)
};

namespace {

// how a refusal on the wide path names the handle's model
std::string wide_what(const nicnes_handle* h) {
    return h->ln ? "layer_n models: " : "wide models (rnn_size or input_encoding_size above 128): ";
}

int fail(nicnes_handle* h, int code, const std::string& msg) {
    if (h) h->err = msg;
    return code;
}

#define HIPC(h, expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail((h), NICNES_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

void layout(const nicnes_config* c, int64_t* off) {
    const int64_t V1 = (int64_t)c->vocab_size + 1, E = c->input_encoding_size, R = c->rnn_size,
                  F = c->fc_feat_size;
    int64_t o = 0;
    off[0] = o; o += E * F;        // img_embed.weight
    off[1] = o; o += E;            // img_embed.bias
    off[2] = o; o += V1 * E;       // embed.weight
    off[3] = o; o += V1 * R;       // logit.weight
    off[4] = o; o += V1;           // logit.bias
    off[5] = o; o += 5 * R * E;    // core.i2h.weight
    off[6] = o; o += 5 * R;        // core.i2h.bias
    off[7] = o; o += 5 * R * R;    // core.h2h.weight
    off[8] = o; o += 5 * R;        // core.h2h.bias
    off[9] = o;
}

// layer_n_affine (with layer_n; ignored without it, as the reference ignores it): six tensors appended behind the nine
bool ln_affine_of(const nicnes_config* c) { return c->layer_n != 0 && c->layer_n_affine != 0; }

// the six tail offsets + D; without affine off7[0..5] = off7[6] = the nine tensors' end
void layout_ln(const nicnes_config* c, int64_t* off7) {
    int64_t off[10];
    layout(c, off);
    const int64_t R = c->rnn_size;
    const bool a = ln_affine_of(c);
    int64_t o = off[9];
    off7[0] = o; o += a ? 5 * R : 0;   // core.i2h_ln.weight
    off7[1] = o; o += a ? 5 * R : 0;   // core.i2h_ln.bias
    off7[2] = o; o += a ? 5 * R : 0;   // core.h2h_ln.weight
    off7[3] = o; o += a ? 5 * R : 0;   // core.h2h_ln.bias
    off7[4] = o; o += a ? R : 0;       // core.c_ln.weight
    off7[5] = o; o += a ? R : 0;       // core.c_ln.bias
    off7[6] = o;
}

// nicnes_allgather_fitness_es: the ranks' padded shares [world, pad, 2] compacted into pair order [n_pairs, 2]
__global__ void es_compact_fitness_kernel(const double* padded, double* out, int n_pairs, int world, int pad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;      // entry i of [n_pairs, 2]
    if (i >= 2 * n_pairs) return;
    const int k = i >> 1, q = n_pairs / world, r = n_pairs % world;
    // pair k belongs to the rank whose nn_es_shard holds it
    const int rank = k < r * (q + 1) ? k / (q + 1) : r + (k - r * (q + 1)) / q;
    const int begin = rank * q + (rank < r ? rank : r);
    out[i] = padded[((size_t)rank * pad + (k - begin)) * 2 + (i & 1)];
}

// nicnes_es_load_theta: a table row widened into the fp64 master (defined first: the kernel below stays the last of
// this file's code object)
__global__ void f32_to_f64_kernel(const float* in, double* out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (double)in[i];
}

__global__ void f64_to_f32_kernel(const double* in, float* out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (float)in[i];
}

// decode shape: G row groups per slab (4: 128-row slabs; 2: 64-row slabs when that pads fewer rows,
// e.g. mscoco_nes.json's batch_size 64), and S logit workgroups per member slab
int auto_G(int B) { return (B + 63) / 64 * 64 < (B + 127) / 128 * 128 ? 2 : 4; }
int nslabs_of(int B, int G) { return (B + 32 * G - 1) / (32 * G); }

// S minimising the makespan ceil(n_wg * S / n_cu) * (1/S + per-workgroup overhead); the split path
// (two launches per step) is charged 2 % over the fused step kernel
int auto_split(int64_t n_wg, int n_cu, int G) {
    int best = 1;
    double bc = 1e300;
    for (int S = 1; S <= 16; S *= 2) {
        const double rounds = std::ceil((double)n_wg * S / n_cu);
        const double cost = rounds * (1.0 / S + 0.03) * ((G == 4 && S > 1) ? 1.02 : 1.0);
        if (cost < bc - 1e-12) {
            bc = cost;
            best = S;
        }
    }
    return best;
}

// logit workgroups the automatic rule can ask for, up to max_members x the widest slab count
int64_t auto_part_cap(int max_members, int max_batch, int n_cu) {
    int64_t cap = 1;
    for (int G = 2; G <= 4; G += 2) {
        const int ns = nslabs_of(max_batch, G);
        for (int64_t n = 1; n <= (int64_t)max_members * ns; ++n)
            cap = std::max(cap, n * auto_split(n, n_cu, G));
    }
    return cap;
}

template <class T>
int dalloc(nicnes_handle* h, T** p, size_t n) {
    if (n == 0) n = 1;
    hipError_t e = hipMalloc((void**)p, n * sizeof(T));
    if (e != hipSuccess) return fail(h, NICNES_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    return NICNES_OK;
}

void decode_shape(const nicnes_handle* h, int B, int count, int* G, int* nslabs, int* S) {
    if (h->wide) {            // the wide path: one workgroup per (member, 128-row slab)
        *G = 4;
        *nslabs = nslabs_of(B, 4);
        *S = 1;
        return;
    }
    *G = h->dec_G ? h->dec_G : auto_G(B);
    *nslabs = nslabs_of(B, *G);
    *S = h->dec_S ? h->dec_S : auto_split((int64_t)count * *nslabs, h->n_cu, *G);
}

// The coop path (the split shape in one persistent launch, nicnes_decode_coop_kernel): 128-row slabs, 2 or
// 4 logit ranges per member slab, and every workgroup of the launch resident at once (one per CU).
// the step queue's switch from the environment: NICNES_DECODE_QUEUE=0/1/2 and NICNES_DECODE_QUEUE_WORKERS=n (n >= 1; anything
// else leaves the value as it is)
void queue_env(int* mode, int* workers) {
    const char* dq = getenv("NICNES_DECODE_QUEUE");
    if (dq && dq[0] >= '0' && dq[0] <= '2' && dq[1] == 0) *mode = dq[0] - '0';
    const char* dw = getenv("NICNES_DECODE_QUEUE_WORKERS");
    if (dw && dw[0] && atoi(dw) >= 1) *workers = atoi(dw);
}

bool coop_fits(const nicnes_handle* h, int G, int nslabs, int S, int count) {
    // (nst >= S: coop_step assumes every logit range non-empty; the split path handles empty ranges)
    return h->coop_mode && G == 4 && (S == 2 || S == 4) && (h->V1 + 63) / 64 >= S &&
           (int64_t)count * nslabs * S <= (int64_t)h->coop_occ * h->n_cu;
}

// Buffers sized by the reference count: the cooked reference n-gram vectors (CIDEr-D).
// the screened decode's buffers: a capture slot per workgroup of the largest fused decode and the members' norms. If
// they cannot be had, screening is off for this engine (the fp32 loop decodes the same tokens).
void ensure_screen(nicnes_handle* h) {
    if (h->wide) h->screen_mode = 0;             // the wide path sums the exp exactly: no screening, no step queue
    if (!h->screen_mode || (h->screen_cap && h->screen_norm)) return;
    const int64_t wgs = (int64_t)h->cfg.max_members * nslabs_of(h->cfg.max_batch, 4);
    bool ok = hipMalloc((void**)&h->screen_cap, (size_t)wgs * SCREEN_CAP_WORDS(h->V1) * sizeof(uint32_t)) == hipSuccess;
    if (ok) ok = hipMalloc((void**)&h->screen_norm, (size_t)h->cfg.max_members * 4 * sizeof(float)) == hipSuccess;
    if (ok && !h->screen_ctr)
        ok = hipMalloc((void**)&h->screen_ctr, SCREEN_CTR_WORDS * sizeof(unsigned long long)) == hipSuccess &&
             hipMemset(h->screen_ctr, 0, SCREEN_CTR_WORDS * sizeof(unsigned long long)) == hipSuccess;
    // the step queue's ring (a slot per member slab of the largest fused decode, rounded up to a power of two) and its
    // control words
    const int32_t slots = nicnes_queue_ring_slots(wgs);
    if (ok && !h->queue_ring && slots >= wgs)
        ok = hipMalloc((void**)&h->queue_ring, (size_t)slots * sizeof(unsigned long long)) == hipSuccess &&
             hipMalloc((void**)&h->queue_ctl, QUEUE_CTL_WORDS * sizeof(uint32_t)) == hipSuccess &&
             hipMemset(h->queue_ctl, 0, QUEUE_CTL_WORDS * sizeof(uint32_t)) == hipSuccess;
    if (ok) {
        h->screen_wgs = wgs;
        if (h->queue_ring) h->queue_slots = slots;
        return;
    }
    (void)hipGetLastError();
    if (h->screen_cap) (void)hipFree(h->screen_cap);
    if (h->screen_norm) (void)hipFree(h->screen_norm);
    if (h->queue_ring) (void)hipFree(h->queue_ring);
    if (h->queue_ctl) (void)hipFree(h->queue_ctl);
    h->screen_cap = nullptr;
    h->screen_norm = nullptr;
    h->queue_ring = nullptr;
    h->queue_ctl = nullptr;
    h->queue_slots = 0;
    h->screen_mode = 0;
}

int alloc_refs(nicnes_handle* h, int max_refs) {
    void* old[] = {h->ref_keys, h->ref_vec, h->ref_count, h->ref_len2, h->ref_norm, h->x_row_img};
    for (void* q : old)
        if (q) (void)hipFree(q);
    h->ref_keys = nullptr; h->ref_vec = nullptr; h->ref_count = nullptr; h->ref_len2 = nullptr; h->ref_norm = nullptr;
    h->x_row_img = nullptr;
    const size_t MR = (size_t)max_refs;
    int rc = dalloc(h, &h->ref_keys, MR * 64);
    if (!rc) rc = dalloc(h, &h->ref_vec, MR * 64);
    if (!rc) rc = dalloc(h, &h->ref_count, MR);
    if (!rc) rc = dalloc(h, &h->ref_len2, MR);
    if (!rc) rc = dalloc(h, &h->ref_norm, MR * 4);
    if (!rc) rc = dalloc(h, &h->x_row_img, MR);
    if (!rc) h->cfg.max_refs = max_refs;
    return rc;
}

// Buffers sized by the batch: per-image n-gram tables, tokens / log-probs / row scores of a launch,
// decode lane scratch, alive flags and partial states.
int alloc_batch(nicnes_handle* h, int max_batch) {
    void* old[] = {h->seq, h->lp, h->row_scores, h->dscratch, h->alive, h->part};
    for (void* q : old)
        if (q) (void)hipFree(q);
    h->seq = nullptr; h->lp = nullptr; h->row_scores = nullptr; h->dscratch = nullptr; h->alive = nullptr;
    h->part = nullptr;
    if (h->coop_ctr) (void)hipFree(h->coop_ctr);
    h->coop_ctr = nullptr;
    const size_t MM = (size_t)h->cfg.max_members, MB = (size_t)max_batch, T = (size_t)h->cfg.seq_length;
    // lane scratch: 2G row waves per slab, the larger of the two slab layouts
    const int rw = std::max(8 * nslabs_of((int)MB, 4), 4 * nslabs_of((int)MB, 2));
    h->alive_stride = (int32_t)(MM * (size_t)nslabs_of((int)MB, 2));
    const int ns = std::max(nslabs_of((int)MB, 2), nslabs_of((int)MB, 4));
    const int es_S = h->es_dec_mode == 2 ? h->es_dec_S : (h->es_dec_mode == 1 ? 4 : 1);   // nicnes_set_decode_es's shapes
    h->part_cap = std::max(auto_part_cap((int)MM, (int)MB, h->n_cu), (int64_t)MM * ns * std::max({h->dec_S, es_S, 1}));
    int rc = dalloc(h, &h->seq, MM * 2 * MB * T);
    if (!rc) rc = dalloc(h, &h->lp, MM * 2 * MB * T);
    if (!rc) rc = dalloc(h, &h->row_scores, MM * 2 * MB);
    // (the wide path: its lane scratch is sized from (E, R), one workgroup per member and 128-row slab)
    const size_t wide_fl = !h->wide ? 0 : nicnes_wide_scratch_floats((int64_t)MM * nslabs_of((int)MB, 4),
                                                                     h->cfg.input_encoding_size, h->cfg.rnn_size, h->ln);
    if (!rc) rc = dalloc(h, &h->dscratch, std::max(nicnes_decode_scratch_floats((int)MM, rw), wide_fl));
    if (!rc) rc = dalloc(h, &h->coop_ctr, MM * (size_t)ns * COOP_CTR_STRIDE);
    if (!rc) rc = dalloc(h, &h->alive, 3 * (size_t)h->alive_stride);
    if (!rc) rc = dalloc(h, &h->part, (size_t)h->part_cap * PART_FLOATS);
    if (!rc) h->cfg.max_batch = max_batch;
    return rc;
}

// Per-image CIDEr-D n-gram tables for every image held (all batches of a per-member-batch evaluate).
int alloc_images(nicnes_handle* h, int n_img) {
    void* old[] = {h->img_hkey, h->img_hrow, h->img_vr};
    for (void* q : old)
        if (q) (void)hipFree(q);
    h->img_hkey = nullptr; h->img_hrow = nullptr; h->img_vr = nullptr;
    const size_t N = (size_t)n_img;
    int rc = dalloc(h, &h->img_hkey, N * IMG_CAP);
    if (!rc) rc = dalloc(h, &h->img_hrow, N * IMG_CAP);
    if (!rc) rc = dalloc(h, &h->img_vr, N * IMG_ROWS * IMG_MAXR);
    if (!rc) h->img_cap = n_img;
    return rc;
}

void xent_work_free(XentWork* w) {
    void* bufs[] = {w->scratch, w->lp_sum, w->n_tok, w->zero_idx, w->out};
    for (void* q : bufs)
        if (q) (void)hipFree(q);
    *w = XentWork();
}

// grown outside every launch (synchronising then)
int xent_work_grow(nicnes_handle* h, XentWork* w, int64_t wgs, int64_t rows, int32_t pms) {
    if (!w->out) {
        int rc = dalloc(h, &w->out, 4);
        if (rc) return rc;
    }
    if (wgs > w->wgs) {
        HIPC(h, hipDeviceSynchronize());
        if (w->scratch) (void)hipFree(w->scratch);
        w->scratch = nullptr;
        w->wgs = 0;
        int rc = dalloc(h, &w->scratch, nicnes_xent_scratch_floats(wgs));
        if (rc) return rc;
        w->wgs = wgs;
    }
    if (rows > w->rows) {
        HIPC(h, hipDeviceSynchronize());
        if (w->lp_sum) (void)hipFree(w->lp_sum);
        if (w->n_tok) (void)hipFree(w->n_tok);
        w->lp_sum = nullptr; w->n_tok = nullptr;
        w->rows = 0;
        int rc = dalloc(h, &w->lp_sum, (size_t)rows);
        if (!rc) rc = dalloc(h, &w->n_tok, (size_t)rows);
        if (rc) return rc;
        w->rows = rows;
    }
    if (pms > w->pms) {
        HIPC(h, hipDeviceSynchronize());
        if (w->zero_idx) (void)hipFree(w->zero_idx);
        w->zero_idx = nullptr;
        w->pms = 0;
        int rc = dalloc(h, &w->zero_idx, (size_t)pms);
        if (rc) return rc;
        HIPC(h, hipMemset(w->zero_idx, 0, (size_t)pms * sizeof(uint64_t)));
        w->pms = pms;
    }
    return NICNES_OK;
}

// the batches' label rows for the xent fitness, from the host's copy st [n_img + 1] of img_ref_start: every batch's first
// row, the largest batch, and (enqueued) the row -> image map
int xent_batch_rows(nicnes_handle* h, const int32_t* st, int n_batches, int B, hipStream_t s) {
    h->x_row0.resize((size_t)n_batches + 1);
    h->x_max_rows = 0;
    for (int k = 0; k <= n_batches; ++k) h->x_row0[(size_t)k] = st[(size_t)k * B];
    for (int k = 0; k < n_batches; ++k) h->x_max_rows = std::max(h->x_max_rows, h->x_row0[k + 1] - h->x_row0[k]);
    h->x_last_rows.clear();
    HIPC(h, nicnes_launch_xent_row_map(h->img_ref_start, n_batches * B, h->x_row_img, s));
    return NICNES_OK;
}

}  // namespace

extern "C" {

int64_t nicnes_param_count(const nicnes_config* cfg) {
    if (!cfg) return -1;
    int64_t off7[7];
    layout_ln(cfg, off7);
    return off7[6];
}

int nicnes_param_offsets(const nicnes_config* cfg, int64_t* out10_host) {
    if (!cfg || !out10_host) return NICNES_ERR_INVALID;
    layout(cfg, out10_host);
    out10_host[9] = nicnes_param_count(cfg);     // D, the layer-norm tail included
    return NICNES_OK;
}

int nicnes_param_offsets_ln(const nicnes_config* cfg, int64_t* out7_host) {
    if (!cfg || !out7_host || !ln_affine_of(cfg)) return NICNES_ERR_INVALID;
    layout_ln(cfg, out7_host);
    return NICNES_OK;
}

int nicnes_create(const nicnes_config* cfg, int device, nicnes_handle** out) {
    if (!cfg || !out) return NICNES_ERR_INVALID;
    *out = nullptr;
    const int V1 = cfg->vocab_size + 1;
    const auto width_ok = [](int w) { return w == 128 || w == 256 || w == 384 || w == 512; };
    if (!width_ok(cfg->input_encoding_size) || !width_ok(cfg->rnn_size)) return NICNES_ERR_UNSUPPORTED;
    if (cfg->fc_feat_size <= 0 || cfg->fc_feat_size % 128 != 0) return NICNES_ERR_UNSUPPORTED;
    if (V1 % 4 != 0 || V1 < 8 || V1 > 16384) return NICNES_ERR_UNSUPPORTED;
    if (cfg->seq_length < 1 || cfg->seq_length > 16) return NICNES_ERR_UNSUPPORTED;
    if (cfg->max_batch < 1 || cfg->max_batch > 1024 || cfg->max_members < 1 || cfg->max_refs < 1)
        return NICNES_ERR_INVALID;
    nicnes_handle* h = new nicnes_handle();
    h->cfg = *cfg;
    h->device = device;
    h->V1 = V1;
    h->wide = cfg->input_encoding_size > 128 || cfg->rnn_size > 128;
    {   // test hook: the default widths down the wide path too (bit-comparable with the fused kernel)
        const char* dw = getenv("NICNES_DECODE_WIDE");
        if (dw && dw[0] == '1' && dw[1] == 0) h->wide = true;
    }
    h->ln = cfg->layer_n != 0;
    h->ln_affine = ln_affine_of(cfg);
    if (h->ln) h->wide = true;
    layout(cfg, h->off);
    {
        int64_t off7[7];
        layout_ln(cfg, off7);
        for (int i = 0; i < 6; ++i) h->ln_off[i] = off7[i];
        h->off[9] = off7[6];
    }
    h->D = h->off[9];
    if (h->D * 4 >= (int64_t)1 << 32) {
        delete h;
        return NICNES_ERR_UNSUPPORTED;
    }
    if (cfg->noise_len < (uint64_t)h->D) {
        delete h;
        return NICNES_ERR_INVALID;
    }
    if (hipSetDevice(device) != hipSuccess) {
        delete h;
        return NICNES_ERR_HIP;
    }
    const size_t D = (size_t)h->D, MM = (size_t)cfg->max_members;
    int rc = NICNES_OK;
    if (!rc) rc = dalloc(h, &h->theta64, D);
    if (!rc) rc = dalloc(h, &h->theta32, D);
    if (!rc) rc = dalloc(h, &h->m, D);
    if (!rc) rc = dalloc(h, &h->v, D);
    if (!rc) rc = dalloc(h, &h->nidx, MM);
    {
        const char* fe = getenv("NICNES_FORCE_EXACT");
        h->force_exact = (fe && fe[0] == '1') ? 1 : 0;
        const char* lm = getenv("NICNES_LSE_MARGIN");
        if (lm && lm[0]) h->lse_margin = (float)atof(lm);
        const char* mf = getenv("NICNES_MUT_FULL");
        h->mut_full = mf && mf[0] == '1';
        const char* bl = getenv("NICNES_BOUNDED_LSE");
        if (bl && (bl[0] == '0' || bl[0] == '1')) h->bounded_mode = bl[0] - '0';
        const char* ds = getenv("NICNES_DECODE_STREAMS");
        if (ds && ds[0] >= '1' && ds[0] <= '4' && ds[1] == 0) h->dec_streams = ds[0] - '0';
        const char* dc = getenv("NICNES_DECODE_COOP");
        if (dc && (dc[0] == '0' || dc[0] == '1') && dc[1] == 0) h->coop_mode = dc[0] - '0';
        const char* cl = getenv("NICNES_COOP_LAUNCH");
        if (cl && (cl[0] == '0' || cl[0] == '1') && cl[1] == 0) h->coop_launch = cl[0] - '0';
        const char* st = getenv("NICNES_TEST_COOP_STALL");
        if (st && st[0]) h->test_stall_ms = (uint32_t)atoi(st);
        const char* sl = getenv("NICNES_TEST_COOP_STALL_LAUNCHES");
        if (sl && sl[0]) h->test_stall_left = atoi(sl);
        const char* ts = getenv("NICNES_TEST_SLOTS");
        if (ts && ts[0]) h->test_slots = atoi(ts);
        const char* sc = getenv("NICNES_SCREEN");
        if (sc && sc[0] >= '0' && sc[0] <= '2' && sc[1] == 0) h->screen_mode = sc[0] - '0';
        const char* se = getenv("NICNES_SCREEN_EPS_SCALE");
        if (se && se[0]) h->screen_scale = std::max(1.0f, (float)atof(se));
        const char* sr = getenv("NICNES_SCREEN_ROUNDS");
        if (sr && sr[0]) h->screen_rounds = std::min(SCREEN_ROUNDS_MAX, std::max(1, atoi(sr)));
        queue_env(&h->queue_mode, &h->queue_workers);
    }
    {
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0)
            h->n_cu = ncu;
    }
    if (!rc && nicnes_decode_init() != hipSuccess) rc = fail(h, NICNES_ERR_HIP, "nicnes_decode_init");
    if (!rc && nicnes_decode_wide_init() != hipSuccess) rc = fail(h, NICNES_ERR_HIP, "nicnes_decode_wide_init");
    if (!rc && nicnes_xent_init() != hipSuccess) rc = fail(h, NICNES_ERR_HIP, "nicnes_xent_init");
    if (!rc && (nicnes_decode_occupancy(&h->coop_occ, &h->sample_occ) != hipSuccess || h->coop_occ < 1 ||
                h->sample_occ < 1))
        rc = fail(h, NICNES_ERR_HIP, "nicnes_decode_occupancy");
    if (!rc) rc = dalloc(h, &h->stats, 4);
    if (!rc && hipHostMalloc((void**)&h->stats_host, 4 * sizeof(int32_t), hipHostMallocDefault) != hipSuccess)
        rc = fail(h, NICNES_ERR_HIP, "hipHostMalloc");
    if (!rc && hipEventCreateWithFlags(&h->stats_ev, hipEventDisableTiming) != hipSuccess)
        rc = fail(h, NICNES_ERR_HIP, "hipEventCreate");
    if (!rc) rc = dalloc(h, &h->partials, 2 * (size_t)nicnes_adam_blocks(h->D));
    if (!rc) rc = dalloc(h, &h->norms, 3);       // |step|^2, |theta|^2, the skip flag
    if (!rc) {
        h->rank_cap = nicnes_rank_scratch_pairs(2 * cfg->max_members);
        rc = dalloc(h, &h->rank_key, h->rank_cap);
        if (!rc) rc = dalloc(h, &h->rank_idx, h->rank_cap);
    }
    if (!rc) ensure_screen(h);
    if (!rc) rc = alloc_refs(h, cfg->max_refs);
    if (!rc) rc = alloc_batch(h, cfg->max_batch);
    if (!rc) rc = alloc_images(h, cfg->max_batch);
    if (!rc) rc = dalloc(h, &h->mbatch, (size_t)cfg->max_members);
    for (int i = 0; i < MB_RING && !rc; ++i) {
        if (hipHostMalloc((void**)&h->mb_pin[i], (size_t)cfg->max_members * sizeof(int32_t), hipHostMallocDefault) != hipSuccess)
            rc = fail(h, NICNES_ERR_HIP, "hipHostMalloc");
        else if (hipEventCreateWithFlags(&h->mb_ev[i], hipEventDisableTiming) != hipSuccess)
            rc = fail(h, NICNES_ERR_HIP, "hipEventCreate");
    }
    if (rc) {
        nicnes_destroy(h);
        return rc;
    }
    (void)hipMemset(h->m, 0, D * sizeof(double));
    (void)hipMemset(h->v, 0, D * sizeof(double));
    (void)hipMemset(h->stats, 0, 4 * sizeof(int32_t));
    if (hipDeviceSynchronize() != hipSuccess) {
        nicnes_destroy(h);
        return NICNES_ERR_HIP;
    }
    *out = h;
    return NICNES_OK;
}

static void split_free(nicnes_split* sp);
static void trainset_free(nicnes_trainset* ts);

int nicnes_destroy(nicnes_handle* h) {
    if (!h) return NICNES_OK;
    (void)hipSetDevice(h->device);
    if (h->comm && h->comm_owned) (void)ncclCommDestroy(h->comm);
    if (!h->splits.empty() || !h->trainsets.empty()) (void)hipDeviceSynchronize();
    for (nicnes_split* sp : h->splits) split_free(sp);
    h->splits.clear();
    for (nicnes_trainset* ts : h->trainsets) trainset_free(ts);
    h->trainsets.clear();
    (void)nicnes_es_free(h);
    void* bufs[] = {h->theta64, h->theta32, h->m, h->v, h->ref_keys, h->ref_vec, h->ref_count, h->ref_len2,
                    h->ref_norm, h->nidx, h->seq, h->lp, h->row_scores, h->dscratch, h->stats, h->partials, h->norms,
                    h->hash_keys, h->hash_vals, h->img_hkey, h->img_hrow, h->img_vr, h->alive, h->part,
                    h->rank_key, h->rank_idx, h->mbatch, h->mut_vec, h->dbuf, h->didx, h->noise_sc, h->coop_ctr,
                    h->zero_noise, h->zero_idx, h->sens_tok, h->su, h->base_scores, h->slog, h->slog_slots, h->zcount,
                    h->screen_cap, h->screen_norm, h->screen_ctr, h->queue_ring, h->queue_ctl, h->dr_fc, h->dr_refs, h->dr_start, h->dr_stage,
                    h->x_row_img};
    xent_work_free(&h->xw);
    if (h->sens) nicnes_sens_destroy(h->sens);
    for (void* p : bufs)
        if (p) (void)hipFree(p);
    if (h->stats_pending) (void)hipEventSynchronize(h->stats_ev);
    if (h->stats_host) (void)hipHostFree(h->stats_host);
    if (h->stats_ev) (void)hipEventDestroy(h->stats_ev);
    for (int i = 0; i < MB_RING; ++i) {
        if (h->mb_ev[i]) {
            (void)hipEventSynchronize(h->mb_ev[i]);
            (void)hipEventDestroy(h->mb_ev[i]);
        }
        if (h->mb_pin[i]) (void)hipHostFree(h->mb_pin[i]);
    }
    for (int i = 0; i < DR_RING; ++i) {
        if (h->dr_ev[i]) {
            (void)hipEventSynchronize(h->dr_ev[i]);
            (void)hipEventDestroy(h->dr_ev[i]);
        }
        if (h->dr_pin[i]) (void)hipHostFree(h->dr_pin[i]);
    }
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->dev)
        if (e) (void)hipEventDestroy(e);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    for (int i = 0; i < 3; ++i) {
        if (h->ev_join[i]) (void)hipEventDestroy(h->ev_join[i]);
        if (h->sx[i]) {
            (void)hipStreamSynchronize(h->sx[i]);
            (void)hipStreamDestroy(h->sx[i]);
        }
    }
    delete h;
    return NICNES_OK;
}

const char* nicnes_last_error(const nicnes_handle* h) { return h ? h->err.c_str() : "null handle"; }

int nicnes_set_noise_table(nicnes_handle* h, const float* table, uint64_t len) {
    if (!h || !table) return NICNES_ERR_INVALID;
    if (len != h->cfg.noise_len) return fail(h, NICNES_ERR_INVALID, "noise table length != config.noise_len");
    if (((uintptr_t)table & 15u) != 0) return fail(h, NICNES_ERR_INVALID, "noise table must be 16-byte aligned");
    h->noise = table;
    h->noise_len = len;
    h->sc_valid = false;          // the sigma-scaled copy is rebuilt at the next evaluation
    return NICNES_OK;
}

int nicnes_set_theta(nicnes_handle* h, const double* theta64, int is_fp32_origin, void* stream) {
    if (!h || !theta64) return NICNES_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipMemcpyAsync(h->theta64, theta64, (size_t)h->D * sizeof(double), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(f64_to_f32_kernel, dim3((unsigned)((h->D + 255) / 256)), dim3(256), 0, s, h->theta64,
                       h->theta32, h->D);
    HIPC(h, hipGetLastError());
    h->theta_is_fp32 = is_fp32_origin ? 1 : 0;
    h->step_pending_check = false;
    h->theta_set = true;
    return NICNES_OK;
}

int nicnes_get_theta(nicnes_handle* h, double* theta64_out, float* theta32_out, void* stream) {
    if (!h || !h->theta_set) return NICNES_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    if (theta64_out)
        HIPC(h, hipMemcpyAsync(theta64_out, h->theta64, (size_t)h->D * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (theta32_out)
        HIPC(h, hipMemcpyAsync(theta32_out, h->theta32, (size_t)h->D * sizeof(float), hipMemcpyDeviceToDevice, s));
    return NICNES_OK;
}

int nicnes_set_adam_state(nicnes_handle* h, const double* m, const double* v, int64_t t, void* stream) {
    if (!h || !m || !v || t < 0) return NICNES_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipMemcpyAsync(h->m, m, (size_t)h->D * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIPC(h, hipMemcpyAsync(h->v, v, (size_t)h->D * sizeof(double), hipMemcpyDeviceToDevice, s));
    h->t = t;
    h->step_pending_check = false;
    return NICNES_OK;
}

int nicnes_get_adam_state(nicnes_handle* h, double* m_out, double* v_out, int64_t* t_out_host, void* stream) {
    if (!h) return NICNES_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    if (m_out) HIPC(h, hipMemcpyAsync(m_out, h->m, (size_t)h->D * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (v_out) HIPC(h, hipMemcpyAsync(v_out, h->v, (size_t)h->D * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (t_out_host) *t_out_host = h->t;
    return NICNES_OK;
}

static CiderTables tables_of(nicnes_handle* h) {
    CiderTables tb;
    tb.df_keys = h->df_keys;
    tb.df_vals = h->df_vals;
    tb.df_n = h->df_n;
    tb.hash_keys = h->hash_keys;
    tb.hash_vals = h->hash_vals;
    tb.hash_mask = h->hash_mask;
    tb.ref_len = h->ref_len;
    tb.ref_keys = h->ref_keys;
    tb.ref_vec = h->ref_vec;
    tb.ref_count = h->ref_count;
    tb.ref_len2 = h->ref_len2;
    tb.ref_norm = h->ref_norm;
    tb.img_hkey = h->img_hkey;
    tb.img_hrow = h->img_hrow;
    tb.img_vr = h->img_vr;
    tb.fault = h->stats;
    return tb;
}

int nicnes_set_df_table(nicnes_handle* h, const uint64_t* keys, const double* df, int64_t n, double ref_len_log) {
    if (!h || n < 0 || (n > 0 && (!keys || !df))) return NICNES_ERR_INVALID;
    HIPC(h, hipSetDevice(h->device));
    if (h->hash_keys) (void)hipFree(h->hash_keys);
    if (h->hash_vals) (void)hipFree(h->hash_vals);
    h->hash_keys = nullptr;
    h->hash_vals = nullptr;
    const uint64_t cap = nicnes_df_hash_capacity(n);
    int rc = dalloc(h, &h->hash_keys, cap);
    if (rc) return rc;
    rc = dalloc(h, &h->hash_vals, cap);
    if (rc) return rc;
    HIPC(h, hipMemset(h->hash_keys, 0, cap * sizeof(uint64_t)));
    HIPC(h, nicnes_launch_df_hash_build(keys, df, n, h->hash_keys, h->hash_vals, cap - 1, nullptr));
    HIPC(h, hipDeviceSynchronize());
    h->hash_mask = cap - 1;
    h->df_keys = keys;
    h->df_vals = df;
    h->df_n = n;
    h->ref_len = ref_len_log;
    h->df_set = true;
    h->batch_set = false;   // reference vectors depend on the df table: set the batch again
    return NICNES_OK;
}

int nicnes_set_batches(nicnes_handle* h, const float* fc, int32_t n_batches, int32_t B, const int32_t* ref_tokens,
                       int32_t n_refs, const int32_t* img_ref_start, void* stream) {
    if (!h || !fc || !ref_tokens || !img_ref_start) return NICNES_ERR_INVALID;
    if (B < 1 || B > 1024) return fail(h, NICNES_ERR_INVALID, "B out of [1, 1024]");
    if (n_batches < 1 || (int64_t)n_batches * B > (1 << 20)) return fail(h, NICNES_ERR_INVALID, "n_batches out of range");
    const int n_img = n_batches * B;
    if (n_refs < n_img) return fail(h, NICNES_ERR_INVALID, "n_refs < images");
    if (!h->df_set) return fail(h, NICNES_ERR_INVALID, "nicnes_set_df_table first");
    if (((uintptr_t)fc & 15u) != 0) return fail(h, NICNES_ERR_INVALID, "fc must be 16-byte aligned");
    HIPC(h, hipSetDevice(h->device));
    // a batch-size curriculum (bs_multiplier, tools/iteration.py:149-153) or more batches can outgrow
    // the sizes the handle was created with: re-create those buffers (outside every evaluate, so no
    // launch in flight uses them once the device is idle)
    if (B > h->cfg.max_batch || n_refs > h->cfg.max_refs || n_img > h->img_cap) {
        HIPC(h, hipDeviceSynchronize());
        int rc = NICNES_OK;
        if (n_refs > h->cfg.max_refs) rc = alloc_refs(h, std::max(n_refs, 2 * h->cfg.max_refs));
        if (!rc && B > h->cfg.max_batch) rc = alloc_batch(h, B);
        if (!rc && n_img > h->img_cap) rc = alloc_images(h, n_img);
        if (rc) {
            h->batch_set = false;
            return rc;
        }
    }
    // reference ranges: CiderD asserts every image has references (len(ref) > 0, upstream
    // cider_scorer); ranges must tile [0, n_refs)
    std::vector<int32_t> st((size_t)n_img + 1);
    HIPC(h, hipMemcpyAsync(st.data(), img_ref_start, st.size() * sizeof(int32_t), hipMemcpyDeviceToHost,
                           (hipStream_t)stream));
    HIPC(h, hipStreamSynchronize((hipStream_t)stream));
    int maxr = 0;
    bool ok = st[0] == 0 && st[n_img] == n_refs;
    for (int b = 0; b < n_img && ok; ++b) {
        ok = st[b + 1] > st[b];
        maxr = std::max(maxr, st[b + 1] - st[b]);
    }
    if (!ok) {
        h->batch_set = false;
        return fail(h, NICNES_ERR_INVALID, "img_ref_start must start at 0, end at n_refs and give every image >= 1 reference");
    }
    h->fc = fc;
    h->B = B;
    h->n_batches = n_batches;
    h->n_img = n_img;
    h->n_refs = n_refs;
    h->img_ref_start = img_ref_start;
    h->ref_tokens = ref_tokens;
    if (int rc = xent_batch_rows(h, st.data(), n_batches, B, (hipStream_t)stream)) {
        h->batch_set = false;
        return rc;
    }
    CiderTables tb = tables_of(h);
    HIPC(h, nicnes_launch_cook_refs(ref_tokens, n_refs, h->cfg.seq_length, &tb, (hipStream_t)stream));
    // per-image n-gram tables when every image has at most IMG_MAXR references (else the
    // per-reference scan kernel scores the candidates)
    h->img_tables = maxr <= IMG_MAXR;
    if (h->img_tables) {
        HIPC(h, hipMemsetAsync(h->img_vr, 0, (size_t)n_img * IMG_ROWS * IMG_MAXR * sizeof(double), (hipStream_t)stream));
        HIPC(h, nicnes_launch_img_ngrams(img_ref_start, n_img, &tb, (hipStream_t)stream));
    }
    h->batch_set = true;
    return NICNES_OK;
}

int nicnes_set_batch(nicnes_handle* h, const float* fc, int32_t B, const int32_t* ref_tokens, int32_t n_refs,
                     const int32_t* img_ref_start, void* stream) {
    return nicnes_set_batches(h, fc, 1, B, ref_tokens, n_refs, img_ref_start, stream);
}

// ---- resident training sets ---------------------------------------------------------------------------------------
static void trainset_free(nicnes_trainset* ts) {
    void* bufs[] = {ts->fc, ts->ref_tokens, ts->img_ref_start};
    for (void* q : bufs)
        if (q) (void)hipFree(q);
    delete ts;
}

static bool trainset_of(const nicnes_handle* h, const nicnes_trainset* ts) {
    return h && ts && std::find(h->trainsets.begin(), h->trainsets.end(), ts) != h->trainsets.end();
}

int nicnes_trainset_create(nicnes_handle* h, const float* fc, int32_t N, const int32_t* ref_tokens, int32_t n_refs,
                           const int32_t* img_ref_start, nicnes_trainset** out, void* stream) {
    if (!h || !ref_tokens || !img_ref_start || !out) return NICNES_ERR_INVALID;   // fc NULL: rows written later
    *out = nullptr;
    if (N < 1 || N > (1 << 24)) return fail(h, NICNES_ERR_INVALID, "N out of [1, 2^24]");
    const size_t F = (size_t)h->cfg.fc_feat_size, T = (size_t)h->cfg.seq_length;
    if (n_refs < N || (int64_t)n_refs * (int64_t)T > INT32_MAX) return fail(h, NICNES_ERR_INVALID, "n_refs out of range");
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipStreamSynchronize(s));        // the caller's arrays may have been written on its stream
    // what nicnes_set_batches checks per call, once: the ranges tile [0, n_refs) and every image has a reference
    std::vector<int32_t> st((size_t)N + 1);
    HIPC(h, hipMemcpy(st.data(), img_ref_start, st.size() * sizeof(int32_t), hipMemcpyDefault));
    bool ok = st[0] == 0 && st[N] == n_refs;
    for (int b = 0; b < N && ok; ++b) ok = st[b + 1] > st[b];
    if (!ok)
        return fail(h, NICNES_ERR_INVALID,
                    "img_ref_start must start at 0, end at n_refs and give every image >= 1 reference");
    // what Engine.set_batches checks on the host: a token outside the vocabulary would alias another word in the
    // scorer's 14-bit key fields
    std::vector<int32_t> tok((size_t)n_refs * T);
    HIPC(h, hipMemcpy(tok.data(), ref_tokens, tok.size() * sizeof(int32_t), hipMemcpyDefault));
    for (int32_t t : tok)
        if (t < 0 || t > h->cfg.vocab_size) return fail(h, NICNES_ERR_INVALID, "reference token outside [0, vocab_size]");
    nicnes_trainset* ts = new nicnes_trainset();
    ts->h = h;
    ts->N = N;
    ts->n_refs = n_refs;
    ts->count.resize((size_t)N);
    for (int b = 0; b < N; ++b) ts->count[(size_t)b] = st[b + 1] - st[b];
    auto run = [&]() -> int {
        int rc = dalloc(h, &ts->fc, (size_t)N * F);
        if (!rc) rc = dalloc(h, &ts->ref_tokens, tok.size());
        if (!rc) rc = dalloc(h, &ts->img_ref_start, st.size());
        if (rc) return rc;
        if (fc)
            HIPC(h, hipMemcpy(ts->fc, fc, (size_t)N * F * sizeof(float), hipMemcpyDefault));
        else                                 // zeros until nicnes_trainset_write_fc fills the rows
            HIPC(h, hipMemset(ts->fc, 0, (size_t)N * F * sizeof(float)));
        HIPC(h, hipMemcpy(ts->ref_tokens, tok.data(), tok.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPC(h, hipMemcpy(ts->img_ref_start, st.data(), st.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPC(h, hipDeviceSynchronize());
        return NICNES_OK;
    };
    const int rc = run();
    if (rc) {
        trainset_free(ts);
        return rc;
    }
    h->trainsets.push_back(ts);
    *out = ts;
    return NICNES_OK;
}

int nicnes_trainset_write_fc(nicnes_handle* h, nicnes_trainset* ts, int32_t first, int32_t count, const float* fc,
                             void* stream) {
    if (!h || !fc) return NICNES_ERR_INVALID;
    if (!trainset_of(h, ts)) return fail(h, NICNES_ERR_INVALID, "not a training set of this handle");
    if (first < 0 || count < 1 || (int64_t)first + count > ts->N)
        return fail(h, NICNES_ERR_INVALID, "rows [first, first + count) outside the set");
    const size_t F = (size_t)h->cfg.fc_feat_size;
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipStreamSynchronize((hipStream_t)stream));   // the caller's rows, and a gather still reading the set
    HIPC(h, hipMemcpy(ts->fc + (size_t)first * F, fc, (size_t)count * F * sizeof(float), hipMemcpyDefault));
    return NICNES_OK;
}

int nicnes_trainset_destroy(nicnes_handle* h, nicnes_trainset* ts) {
    if (!h) return NICNES_ERR_INVALID;
    if (!ts) return NICNES_OK;
    if (!trainset_of(h, ts)) return fail(h, NICNES_ERR_INVALID, "not a training set of this handle");
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipDeviceSynchronize());         // a gather of a draw may still read the set
    h->trainsets.erase(std::find(h->trainsets.begin(), h->trainsets.end(), ts));
    trainset_free(ts);
    return NICNES_OK;
}

// the draw's own batch buffers for n_img images and n_refs reference rows (grown outside every launch)
static int draw_grow(nicnes_handle* h, int n_img, int n_refs) {
    const size_t F = (size_t)h->cfg.fc_feat_size, T = (size_t)h->cfg.seq_length;
    if (n_img > h->dr_img_cap) {
        HIPC(h, hipDeviceSynchronize());
        void* old[] = {h->dr_fc, h->dr_start, h->dr_stage};
        for (void* q : old)
            if (q) (void)hipFree(q);
        h->dr_fc = nullptr; h->dr_start = nullptr; h->dr_stage = nullptr;
        h->dr_img_cap = 0;
        const size_t cap = (size_t)std::max(n_img, h->img_cap);
        int rc = dalloc(h, &h->dr_fc, cap * F);
        if (!rc) rc = dalloc(h, &h->dr_start, cap + 1);
        if (!rc) rc = dalloc(h, &h->dr_stage, 2 * cap + 1);
        if (rc) return rc;
        h->dr_img_cap = (int32_t)cap;
    }
    if (n_refs > h->dr_ref_cap) {
        HIPC(h, hipDeviceSynchronize());
        if (h->dr_refs) (void)hipFree(h->dr_refs);
        h->dr_refs = nullptr;
        h->dr_ref_cap = 0;
        const size_t cap = (size_t)std::max(n_refs, h->cfg.max_refs);
        int rc = dalloc(h, &h->dr_refs, cap * T);
        if (rc) return rc;
        h->dr_ref_cap = (int32_t)cap;
    }
    return NICNES_OK;
}

int nicnes_draw_batches(nicnes_handle* h, nicnes_trainset* ts, const int32_t* image_ix_host, int32_t n_batches, int32_t B,
                        void* stream) {
    if (!h || !image_ix_host) return NICNES_ERR_INVALID;
    if (!trainset_of(h, ts)) return fail(h, NICNES_ERR_INVALID, "not a training set of this handle");
    if (B < 1 || B > 1024) return fail(h, NICNES_ERR_INVALID, "B out of [1, 1024]");
    if (n_batches < 1 || (int64_t)n_batches * B > (1 << 20)) return fail(h, NICNES_ERR_INVALID, "n_batches out of range");
    if (!h->df_set) return fail(h, NICNES_ERR_INVALID, "nicnes_set_df_table first");
    const int n_img = n_batches * B;
    // the host's own copy of the counts gives n_refs and the largest reference count: nothing is read back
    int64_t total = 0;
    int maxr = 0;
    for (int i = 0; i < n_img; ++i) {
        const int32_t ix = image_ix_host[i];
        if (ix < 0 || ix >= ts->N) return fail(h, NICNES_ERR_INVALID, "image index outside [0, N)");
        total += ts->count[(size_t)ix];
        maxr = std::max(maxr, ts->count[(size_t)ix]);
    }
    if (total * h->cfg.seq_length > INT32_MAX) return fail(h, NICNES_ERR_INVALID, "too many reference rows in one draw");
    const int n_refs = (int)total;
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    // growth as in nicnes_set_batches (synchronising then), and the draw's own buffers with it
    {
        int rc = NICNES_OK;
        if (B > h->cfg.max_batch || n_refs > h->cfg.max_refs || n_img > h->img_cap) {
            HIPC(h, hipDeviceSynchronize());
            h->batch_set = false;            // the batch held loses its cooked buffers: whatever fails below, it is gone
            if (n_refs > h->cfg.max_refs) rc = alloc_refs(h, std::max(n_refs, 2 * h->cfg.max_refs));
            if (!rc && B > h->cfg.max_batch) rc = alloc_batch(h, B);
            if (!rc && n_img > h->img_cap) rc = alloc_images(h, n_img);
        }
        const bool own = h->fc == h->dr_fc && h->fc;    // the batch held lives in the buffers about to move
        if (!rc && (n_img > h->dr_img_cap || n_refs > h->dr_ref_cap)) {
            if (own) h->batch_set = false;
            rc = draw_grow(h, n_img, n_refs);
        }
        if (rc) {
            h->batch_set = false;
            return rc;
        }
    }
    // staging: [n_img] indices, [n_img + 1] destination starts, through a pinned slot whose last copy has run
    const size_t words = 2 * (size_t)n_img + 1;
    const int slot = h->dr_next;
    h->dr_next = (slot + 1) % DR_RING;
    if (!h->dr_ev[slot]) HIPC(h, hipEventCreateWithFlags(&h->dr_ev[slot], hipEventDisableTiming));
    if (h->dr_used[slot]) HIPC(h, hipEventSynchronize(h->dr_ev[slot]));
    h->dr_used[slot] = false;
    if (words > h->dr_pin_cap[slot]) {
        if (h->dr_pin[slot]) (void)hipHostFree(h->dr_pin[slot]);
        h->dr_pin[slot] = nullptr;
        h->dr_pin_cap[slot] = 0;
        const size_t cap = std::max(words, 2 * (size_t)h->img_cap + 1);
        if (hipHostMalloc((void**)&h->dr_pin[slot], cap * sizeof(int32_t), hipHostMallocDefault) != hipSuccess)
            return fail(h, NICNES_ERR_HIP, "hipHostMalloc");
        h->dr_pin_cap[slot] = cap;
    }
    int32_t* pin = h->dr_pin[slot];
    std::memcpy(pin, image_ix_host, (size_t)n_img * sizeof(int32_t));
    int32_t* dst = pin + n_img;
    dst[0] = 0;
    for (int i = 0; i < n_img; ++i) dst[i + 1] = dst[i] + ts->count[(size_t)image_ix_host[i]];
    h->batch_set = false;                    // until everything below is enqueued
    HIPC(h, hipMemcpyAsync(h->dr_stage, pin, words * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPC(h, hipEventRecord(h->dr_ev[slot], s));
    h->dr_used[slot] = true;
    HIPC(h, nicnes_launch_gather_fc(ts->fc, h->dr_stage, n_img, h->cfg.fc_feat_size, h->dr_fc, s));
    HIPC(h, nicnes_launch_gather_refs(ts->ref_tokens, ts->img_ref_start, h->dr_stage, h->dr_stage + n_img, n_img,
                                      h->cfg.seq_length, h->dr_refs, h->dr_start, s));
    // from here on: nicnes_set_batches on the handle's own buffers
    h->fc = h->dr_fc;
    h->B = B;
    h->n_batches = n_batches;
    h->n_img = n_img;
    h->n_refs = n_refs;
    h->img_ref_start = h->dr_start;
    h->ref_tokens = h->dr_refs;
    if (int rc = xent_batch_rows(h, dst, n_batches, B, s)) return rc;
    CiderTables tb = tables_of(h);
    HIPC(h, nicnes_launch_cook_refs(h->dr_refs, n_refs, h->cfg.seq_length, &tb, s));
    h->img_tables = maxr <= IMG_MAXR;
    if (h->img_tables) {
        HIPC(h, hipMemsetAsync(h->img_vr, 0, (size_t)n_img * IMG_ROWS * IMG_MAXR * sizeof(double), s));
        HIPC(h, nicnes_launch_img_ngrams(h->dr_start, n_img, &tb, s));
    }
    h->batch_set = true;
    return NICNES_OK;
}

int nicnes_test_batch_state(nicnes_handle* h, float* fc_out, int32_t* refs_out, int32_t* starts_out, void* stream) {
    if (!h) return NICNES_ERR_INVALID;
    if (!h->batch_set) return fail(h, NICNES_ERR_INVALID, "nicnes_set_batch first");
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    const size_t F = (size_t)h->cfg.fc_feat_size, T = (size_t)h->cfg.seq_length;
    if (fc_out)
        HIPC(h, hipMemcpyAsync(fc_out, h->fc, (size_t)h->n_img * F * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (refs_out)
        HIPC(h, hipMemcpyAsync(refs_out, h->ref_tokens, (size_t)h->n_refs * T * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (starts_out)
        HIPC(h, hipMemcpyAsync(starts_out, h->img_ref_start, ((size_t)h->n_img + 1) * sizeof(int32_t),
                               hipMemcpyDeviceToDevice, s));
    return NICNES_OK;
}

int nicnes_noise_indices(nicnes_handle* h, uint64_t iteration, int32_t member_begin, int32_t count, uint64_t* out,
                         void* stream) {
    if (!h || !out || member_begin < 0 || count < 0) return NICNES_ERR_INVALID;
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, nicnes_launch_noise_index(h->cfg.noise_seed, iteration, (uint64_t)member_begin, count, h->cfg.noise_len,
                                      (uint64_t)h->D, out, (hipStream_t)stream));
    return NICNES_OK;
}

int nicnes_noise_vectors(nicnes_handle* h, uint64_t iteration, int32_t member_begin, int32_t count, float sigma,
                         float* out, void* stream) {
    if (!h || !out || member_begin < 0 || count < 1) return NICNES_ERR_INVALID;
    if (count > h->cfg.max_members) return fail(h, NICNES_ERR_INVALID, "count > max_members");
    if (!h->noise) return fail(h, NICNES_ERR_INVALID, "nicnes_set_noise_table first");
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, nicnes_launch_noise_index(h->cfg.noise_seed, iteration, (uint64_t)member_begin, count, h->cfg.noise_len,
                                      (uint64_t)h->D, h->nidx, s));
    if (h->mut_mode)
        HIPC(h, nicnes_launch_mutate(h->noise, h->nidx, count, h->D, sigma, h->mut_vec, h->mut_mode, out, h->D, s));
    else
        HIPC(h, nicnes_launch_noise_vectors(h->noise, h->nidx, count, h->D, sigma, out, s));
    return NICNES_OK;
}

int nicnes_set_mutation(nicnes_handle* h, int32_t mode, const float* vec, void* stream) {
    if (!h || mode < 0 || mode > 2 || (mode && !vec)) return NICNES_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    if (mode && !h->mut_vec) {       // first use: the [D] vector
        HIPC(h, hipDeviceSynchronize());
        int rc = dalloc(h, &h->mut_vec, (size_t)h->D);
        if (rc) return rc;
    }
    if (mode) HIPC(h, hipMemcpyAsync(h->mut_vec, vec, (size_t)h->D * sizeof(float), hipMemcpyDeviceToDevice, s));
    h->mut_mode = mode;
    return NICNES_OK;
}

int nicnes_set_mutation_proportional(nicnes_handle* h, float mean_abs, void* stream) {
    if (!h || !(mean_abs >= 0.f)) return NICNES_ERR_INVALID;
    if (!h->theta_set) return fail(h, NICNES_ERR_INVALID, "nicnes_set_theta first");
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    if (!h->mut_vec) {               // first use: the [D] vector
        HIPC(h, hipDeviceSynchronize());
        int rc = dalloc(h, &h->mut_vec, (size_t)h->D);
        if (rc) return rc;
    }
    HIPC(h, nicnes_launch_proportional(h->theta32, h->D, mean_abs, h->mut_vec, s));
    h->mut_mode = 2;
    return NICNES_OK;
}

int nicnes_theta_zeros(nicnes_handle* h, int64_t* count_out_host, void* stream) {
    if (!h || !count_out_host) return NICNES_ERR_INVALID;
    if (!h->theta_set) return fail(h, NICNES_ERR_INVALID, "nicnes_set_theta first");
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    if (!h->zcount) {
        HIPC(h, hipDeviceSynchronize());
        int rc = dalloc(h, &h->zcount, 1);
        if (rc) return rc;
    }
    unsigned long long* d = h->zcount;
    HIPC(h, nicnes_launch_count_zeros(h->theta32, h->D, d, s));
    unsigned long long c = 0;
    HIPC(h, hipMemcpyAsync(&c, d, sizeof c, hipMemcpyDeviceToHost, s));
    HIPC(h, hipStreamSynchronize(s));
    *count_out_host = (int64_t)c;
    return NICNES_OK;
}

int nicnes_set_rows_per_image(nicnes_handle* h, int32_t n) {
    if (!h || n < 1 || n > 64) return NICNES_ERR_INVALID;
    h->rpi = n;
    return NICNES_OK;
}

int nicnes_set_sample_draws(nicnes_handle* h, const double* u_host, int64_t n) {
    if (!h || n < 0 || (n > 0 && !u_host)) return NICNES_ERR_INVALID;
    h->su_host.assign(u_host, u_host + n);
    return NICNES_OK;
}

int nicnes_set_fitness_mode(nicnes_handle* h, int32_t mode) {
    if (!h) return NICNES_ERR_INVALID;
    if (mode < NICNES_FITNESS_GREEDY || mode > NICNES_FITNESS_XENT)
        return fail(h, NICNES_ERR_UNSUPPORTED, "fitness mode: the engine implements greedy, greedy_{log,exp,lin,avg}prob, "
                                               "sample, self_critical, sc_loss and xent");
    if (h->wide && mode == NICNES_FITNESS_XENT)
        return fail(h, NICNES_ERR_UNSUPPORTED, wide_what(h) + "the xent fitness is not supported (E = R = 128 only)");
    if (h->wide && mode >= NICNES_FITNESS_SAMPLE)
        return fail(h, NICNES_ERR_UNSUPPORTED, wide_what(h) + "the sampled fitness "
                                               "modes are not supported (greedy, greedy_*)");
    h->fitness_mode = mode;
    return NICNES_OK;
}

// [D] zeros + one zero slice index: theta itself as a "member" (the sigma = 0 decodes)
static int ensure_zero_noise(nicnes_handle* h) {
    if (h->zero_noise) return NICNES_OK;
    HIPC(h, hipDeviceSynchronize());
    int rc = dalloc(h, &h->zero_noise, (size_t)h->D);
    if (!rc) rc = dalloc(h, &h->zero_idx, 1);
    if (rc) return rc;
    HIPC(h, hipMemset(h->zero_noise, 0, (size_t)h->D * sizeof(float)));
    HIPC(h, hipMemset(h->zero_idx, 0, sizeof(uint64_t)));
    return NICNES_OK;
}

int nicnes_evaluate(nicnes_handle* h, uint64_t iteration, int32_t member_begin, int32_t count, float sigma,
                    double* fitness_out, int32_t* seq_out, void* stream) {
    return nicnes_evaluate_lp(h, iteration, member_begin, count, sigma, fitness_out, seq_out, nullptr, stream);
}

int nicnes_evaluate_lp(nicnes_handle* h, uint64_t iteration, int32_t member_begin, int32_t count, float sigma,
                       double* fitness_out, int32_t* seq_out, float* logprob_out, void* stream) {
    return nicnes_evaluate_batches(h, iteration, member_begin, count, sigma, nullptr, fitness_out, seq_out, logprob_out,
                                   stream);
}

// The row buffers (tokens, log-probs, row scores, decode scratch) grown to `rows` rollout rows, before anything
// takes their addresses.
static int ensure_rows(nicnes_handle* h, int rows) {
    if (rows <= h->cfg.max_batch) return NICNES_OK;
    HIPC(h, hipDeviceSynchronize());
    return alloc_batch(h, rows);
}

// The caller's member -> batch map (host, `count` entries, nullable) checked and copied to the device on s:
// *mb_out = the device map, or NULL when none was given (then only one batch may be held).
static int stage_member_batch(nicnes_handle* h, const int32_t* member_batch_host, int count, hipStream_t s,
                              const int32_t** mb_out) {
    *mb_out = nullptr;
    if (member_batch_host) {
        for (int k = 0; k < count; ++k)
            if (member_batch_host[k] < 0 || member_batch_host[k] >= h->n_batches)
                return fail(h, NICNES_ERR_INVALID, "member_batch entry outside [0, n_batches)");
        // the caller's array may go away on return: copied to a pinned ring slot whose previous copy has run
        const int slot = h->mb_next;
        h->mb_next = (slot + 1) % MB_RING;
        if (h->mb_used[slot]) HIPC(h, hipEventSynchronize(h->mb_ev[slot]));
        std::memcpy(h->mb_pin[slot], member_batch_host, (size_t)count * sizeof(int32_t));
        HIPC(h, hipMemcpyAsync(h->mbatch, h->mb_pin[slot], (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIPC(h, hipEventRecord(h->mb_ev[slot], s));
        h->mb_used[slot] = true;
        *mb_out = h->mbatch;
    } else if (h->n_batches != 1) {
        return fail(h, NICNES_ERR_INVALID, "several batches are held: pass member_batch (nicnes_evaluate_batches)");
    }
    return NICNES_OK;
}

// CIDEr-D of n_cand candidates of `rows` rollout rows each (seq, lp [n_cand, rows, T] on the device; lp, mb, base
// and scores_out nullable) against the batches held, and the fitness of the handle's mode: the image tables when
// every image has <= IMG_MAXR references (per-row scores land in h->row_scores), else the per-reference scan.
// The one scorer dispatch: nicnes_evaluate* and nicnes_test_score_rows both end here.
static int score_rollouts(nicnes_handle* h, const int32_t* seq, const float* lp, int n_cand, int rows, int rpi,
                          const int32_t* mb, const double* base, double* fitness_out, double* scores_out,
                          hipStream_t s) {
    CiderTables tb = tables_of(h);
    if (h->img_tables) {
        HIPC(h, nicnes_launch_cider_img(seq, n_cand, rows, h->cfg.seq_length, &tb, h->img_ref_start, mb, lp,
                                         h->fitness_mode, h->row_scores, fitness_out, s, base, rpi));
        if (scores_out)
            HIPC(h, hipMemcpyAsync(scores_out, h->row_scores, (size_t)n_cand * rows * sizeof(double),
                                   hipMemcpyDeviceToDevice, s));
    } else {
        HIPC(h, nicnes_launch_cider(seq, n_cand, rows, h->cfg.seq_length, &tb, h->img_ref_start, mb, lp,
                                    h->fitness_mode, fitness_out, s, base, scores_out, rpi));
    }
    return NICNES_OK;
}

// ---- a decode request, piece by piece: what every site that builds a DecodeParams shares -------------------------
// What the handle alone fixes; everything else is zero. Each site adds its buffers, its shape (B, B_img, rpi, sign_off,
// G, S, coop) and its switches (no_exit, test_stall_ms) itself.
static DecodeParams decode_base(const nicnes_handle* h) {
    DecodeParams p{};
    p.F = h->cfg.fc_feat_size;
    p.V1 = h->V1;
    p.T = h->cfg.seq_length;
    p.D = h->D;
    p.off_img_w = h->off[0];
    p.off_img_b = h->off[1];
    p.off_emb_w = h->off[2];
    p.off_log_w = h->off[3];
    p.off_log_b = h->off[4];
    p.off_i2h_w = h->off[5];
    p.off_i2h_b = h->off[6];
    p.off_h2h_w = h->off[7];
    p.off_h2h_b = h->off[8];
    p.stats = h->stats;
    p.force_exact = h->force_exact;
    p.lse_margin = h->lse_margin;
    p.coop_launch = h->coop_launch;
    return p;
}

// h->noise_sc = fp32(sigma * z), the table scaled once per sigma (its bit pattern): the plain decode's noise, and the
// sigma z a mutated fused decode forms the head parameters' delta' from. Allocated at the first use.
static int ensure_noise_scaled(nicnes_handle* h, float sigma, hipStream_t s) {
    if (!h->noise_sc) {
        HIPC(h, hipDeviceSynchronize());
        int rc = dalloc(h, &h->noise_sc, (size_t)h->cfg.noise_len);
        if (rc) return rc;
    }
    if (!h->sc_valid || __builtin_bit_cast(uint32_t, h->sc_sigma) != __builtin_bit_cast(uint32_t, sigma)) {
        HIPC(h, nicnes_launch_scale(h->noise, h->noise_sc, h->cfg.noise_len, sigma, s));
        h->sc_sigma = sigma;
        h->sc_valid = true;
    }
    return NICNES_OK;
}

// The members' mutated delta' rows [max_members, Dp] and their row offsets k * Dp, allocated at the first mutated
// decode (the handle's safe / proportional mutations, nic_es's proportional one)
static int ensure_delta_rows(nicnes_handle* h, float** dbuf, uint64_t** didx, int64_t Dp, hipStream_t s) {
    if (*dbuf) return NICNES_OK;
    HIPC(h, hipDeviceSynchronize());
    int rc = dalloc(h, dbuf, (size_t)h->cfg.max_members * (size_t)Dp);
    if (!rc) rc = dalloc(h, didx, (size_t)h->cfg.max_members);
    if (rc) return rc;
    HIPC(h, nicnes_launch_iota_stride(*didx, h->cfg.max_members, (uint64_t)Dp, s));
    return NICNES_OK;
}

// The bounded-lse policy (nicnes_handle::bounded_mode) and the read-back of the decode counters that drives it, in the
// order an evaluate calls them. lse_poll: a finished read-back's faults reported, and two or more new fallbacks of a
// bounded decode send the next 32 decodes to the exact sum.
static int lse_poll(nicnes_handle* h) {
    if (!h->stats_pending || hipEventQuery(h->stats_ev) != hipSuccess) return NICNES_OK;
    const int32_t fb = h->stats_host[0];
    if (h->stats_host[2] != 0)
        return fail(h, NICNES_ERR_FAULT, "coop decode: a workgroup's partners never arrived (hand-off timeout)");
    if (h->stats_host[3] != 0)
        return fail(h, NICNES_ERR_FAULT, "sampled decode: a workgroup found no free logit slot");
    if (h->last_bounded && fb - h->fb_seen >= 2) h->exact_left = 32;
    h->fb_seen = fb;
    h->stats_pending = false;
    return NICNES_OK;
}

// the policy as it stands (nicnes_split_decode reads it without advancing it: tokens do not depend on the lse mode)
static bool lse_bounded_now(const nicnes_handle* h) {
    if (h->wide) return false;                    // the wide path: the exact exp-sum only
    return h->bounded_mode == 1 || (h->bounded_mode == 2 && h->exact_left == 0);
}

// the lse mode of the decode being built; a greedy-only one (no log-probs) spends one of the exact decodes left
static bool lse_decide(nicnes_handle* h, bool greedy_only) {
    const bool bounded = lse_bounded_now(h);
    if (h->bounded_mode == 2 && h->exact_left > 0 && greedy_only) --h->exact_left;
    h->last_decode_bounded = (bounded && greedy_only) ? 1 : 0;
    return bounded;
}

// after the launch: the counters read back without a host wait, unless a read-back is still in flight
static int lse_arm(nicnes_handle* h, bool bounded_greedy, hipStream_t s) {
    if (h->stats_pending) return NICNES_OK;
    HIPC(h, hipMemcpyAsync(h->stats_host, h->stats, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPC(h, hipEventRecord(h->stats_ev, s));
    h->stats_pending = true;
    h->last_bounded = bounded_greedy;
    return NICNES_OK;
}

// The screened logit loop's arguments for a decode of `members` members in `workgroups` fused workgroups: its buffers
// when the caller's path allows it (eligible), the mode asks for it and the decode fits them, else cap == NULL (the
// fp32 loop). Automatic mode: from one workgroup per CU on (P = 256, B = 128: 15.7 ms an iteration screened against
// 23.05 ms unscreened); fewer workgroups than CUs were not measured. The buffers (ensure_screen, at create
// or at the setter: nothing is allocated here) hold screen_wgs capture slots and max_members rows of norms.
static ScreenArgs pick_screen(const nicnes_handle* h, int members, int64_t workgroups, bool eligible) {
    ScreenArgs sa{nullptr, nullptr, h->screen_scale, h->screen_ctr, h->screen_rounds};
    const bool on = h->screen_mode == 1 || (h->screen_mode == 2 && workgroups >= h->n_cu);
    if (eligible && on && h->screen_cap && h->screen_norm && workgroups <= h->screen_wgs &&
        members <= h->cfg.max_members) {
        sa.cap = h->screen_cap;
        sa.norm = h->screen_norm;
    }
    return sa;
}

// The decode of `count` members enqueued on s, or in parts on s and the engine's streams: the one fork/join of
// nicnes_evaluate*, nicnes_split_decode and nicnes_es_evaluate. With pa (nic_es: members with their own base theta)
// the launches are nicnes_launch_decode_es, which takes no MutHead, timing events or queue. Returns the number of
// streams used, or -(error code).
static int launch_decode_parts(nicnes_handle* h, const DecodeParams& p, const MutHead& mh, const ScreenArgs& sa,
                               const QueueArgs* qa, const ParentArgs* pa, int count, int nslabs, hipStream_t s, bool timed,
                               int* n_ev) {
#define HIPN(expr)                                                                                           \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess) return -fail(h, NICNES_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
    // the coop launch needs all its workgroups resident: never split over streams. (nic_es decodes with S == 1 unless
    // coop, so the same rule gives it one stream unless nicnes_set_decode_streams asks for more)
    const int nstr = p.coop || h->wide ? 1 : std::min(count, h->dec_streams ? h->dec_streams : (p.S == 1 ? 1 : 2));
    if (h->wide) {
        // the wide path: one launch on the caller's stream; no MutHead (the delta' rows are whole), no nic_es parents
        if (pa || mh.mode || sa.cap || p.sample_u)
            return -fail(h, NICNES_ERR_UNSUPPORTED, wide_what(h) + "greedy decode "
                                                    "only");
        HIPN(nicnes_launch_decode_wide(&p, h->cfg.input_encoding_size, h->cfg.rnn_size, h->ln,
                                       h->ln_affine ? h->ln_off : nullptr, count, nslabs, s, timed ? h->dev : nullptr,
                                       h->dev_kind, n_ev));
    } else if (nstr > 1) {
        // members split evenly over the caller's stream and nstr - 1 engine streams; the parts share
        // nothing but the fallback counter (an atomic). No per-launch events: the launches overlap
        if (!h->ev_fork) HIPN(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
        for (int i = 0; i < nstr - 1; ++i)
            if (!h->sx[i]) {
                HIPN(hipStreamCreateWithFlags(&h->sx[i], hipStreamNonBlocking));
                HIPN(hipEventCreateWithFlags(&h->ev_join[i], hipEventDisableTiming));
            }
        HIPN(hipEventRecord(h->ev_fork, s));
        for (int i = 0; i < nstr; ++i) {
            const int a = (int)((int64_t)count * i / nstr), b = (int)((int64_t)count * (i + 1) / nstr);
            DecodeParams pi = p;
            MutHead mi = mh;
            ScreenArgs si_ = sa;
            ParentArgs pa_i = pa ? *pa : ParentArgs{};
            nicnes_decode_shift(&pi, a, nslabs, pa ? nullptr : &mi, &si_, pa ? &pa_i : nullptr);
            hipStream_t si = i == 0 ? s : h->sx[i - 1];
            if (i > 0) HIPN(hipStreamWaitEvent(si, h->ev_fork, 0));
            if (pa)
                HIPN(nicnes_launch_decode_es(&pi, &pa_i, b - a, nslabs, si, &si_));
            else
                HIPN(nicnes_launch_decode(&pi, &mi, b - a, nslabs, si, nullptr, nullptr, nullptr, &si_));
        }
        for (int i = 0; i < nstr - 1; ++i) {
            HIPN(hipEventRecord(h->ev_join[i], h->sx[i]));
            HIPN(hipStreamWaitEvent(s, h->ev_join[i], 0));
        }
    } else if (pa) {
        HIPN(nicnes_launch_decode_es(&p, pa, count, nslabs, s, &sa));
    } else {
        // (the step queue: only a decode in one part; the parts of a decode over several streams would share its ring)
        HIPN(nicnes_launch_decode(&p, &mh, count, nslabs, s, timed ? h->dev : nullptr, h->dev_kind, n_ev, &sa, qa));
    }
#undef HIPN
    return nstr;
}

// The tail both evaluates share, from the zeroed outputs to the last timing event: the decode of `count` members
// into p.seq / p.lp (out_rows rows), the log-prob exit pass, the counter read-back and the scoring of the n_cand
// rollouts of rows_total rows each (n_cand is also the lp pass's rollout count: 2 * count, or eval_theta's 1).
static int decode_and_score(nicnes_handle* h, const DecodeParams& p, const MutHead& mh, const ScreenArgs& sa,
                            const QueueArgs* qa, const ParentArgs* pa, int count, int nslabs, size_t out_rows, int n_cand,
                            int rows_total, int rpi, const int32_t* mb, const double* base, double* fitness_out,
                            double* scores_out, hipStream_t s) {
    // rows a member never writes (all finished early) must read as 0 (nets.py:188 zeros)
    HIPC(h, hipMemsetAsync(p.seq, 0, out_rows * h->cfg.seq_length * sizeof(int32_t), s));
    if (p.lp) HIPC(h, hipMemsetAsync(p.lp, 0, out_rows * h->cfg.seq_length * sizeof(float), s));
    if (h->timing) HIPC(h, hipEventRecord(h->ev[0], s));
    int n_ev = 0;
    const int nstr = launch_decode_parts(h, p, mh, sa, qa, pa, count, nslabs, s, h->timing, &n_ev);
    if (nstr < 0) return -nstr;
    h->n_dev = h->timing ? n_ev : 0;      // (nic_es launches record no events: 0)
    h->multi_stream = nstr > 1;
    // log-probs of a no_exit decode past the batch's last finishing step. Also with one slab: its workgroup holds both
    // signs and runs until the later of the two has finished, writing the earlier one's log-probs past that rollout's own
    // last step (eval_theta: the two halves are one rollout)
    if (p.lp) HIPC(h, nicnes_launch_lp_batch_exit(p.seq, p.lp, n_cand, rows_total, h->cfg.seq_length, s));
    if (h->timing) HIPC(h, hipEventRecord(h->ev[1], s));
    if (int rc = lse_arm(h, p.bounded_lse && !p.lp, s)) return rc;
    if (int rc = score_rollouts(h, p.seq, p.lp, n_cand, rows_total, rpi, mb, base, fitness_out, scores_out, s)) return rc;
    if (h->timing) HIPC(h, hipEventRecord(h->ev[2], s));
    return NICNES_OK;
}

// The teacher-forced forward of theta over the label rows [row0, row1) of (labels, row_img, fc [n_img, F]) as one flat
// range of pseudo-members over the zero noise slice: per-row results in w->lp_sum / n_tok, the sums in w->out.
static int xent_flat(nicnes_handle* h, XentWork* w, const int32_t* labels, const int32_t* row_img, const float* fc,
                     int32_t n_img, int32_t row0, int32_t row1, float* steps_out, hipStream_t s) {
    const int rows = row1 - row0, n_pm = (rows + 255) / 256;
    if (rows < 1) return fail(h, NICNES_ERR_INVALID, "xent: no label rows in the range");
    if (int rc = ensure_zero_noise(h)) return rc;
    if (int rc = xent_work_grow(h, w, n_pm, (int64_t)n_pm * 256, n_pm)) return rc;
    DecodeParams p = decode_base(h);
    p.theta = h->theta32;
    p.noise = h->zero_noise;
    p.noise_idx = w->zero_idx;
    p.fc = fc;
    p.scratch = w->scratch;
    const XentArgs xa{labels, row_img, nullptr, w->lp_sum, w->n_tok, steps_out, n_img, row0, row1, 0};
    if (steps_out) HIPC(h, hipMemsetAsync(steps_out, 0, (size_t)rows * (h->cfg.seq_length + 1) * sizeof(float), s));
    HIPC(h, nicnes_launch_xent(&p, &xa, n_pm, 1, 1, w->out, (long long*)(w->out + 3), w->out + 1, s));
    return NICNES_OK;
}

// NICNES_FITNESS_XENT: the evaluate of members member_begin .. + count on their batches' label rows (theta_batch < 0),
// or of theta itself on the rows of batch theta_batch. steps_out (nullable): nicnes_test_xent_steps.
static int xent_evaluate(nicnes_handle* h, uint64_t iteration, int32_t member_begin, int32_t count, float sigma,
                         const int32_t* member_batch_host, int theta_batch, double* fitness_out, float* steps_out,
                         hipStream_t s) {
    const bool theta = theta_batch >= 0;
    if (h->wide) return fail(h, NICNES_ERR_UNSUPPORTED, wide_what(h) + "the xent fitness is not supported (E = R = 128 only)");
    if (h->mut_mode)
        return fail(h, NICNES_ERR_UNSUPPORTED, "xent fitness: safe and proportional mutations are not supported (plain only)");
    if (!theta && (count < 1 || count > h->cfg.max_members)) return fail(h, NICNES_ERR_INVALID, "count out of [1, max_members]");
    if (!theta && !h->noise) return fail(h, NICNES_ERR_INVALID, "nicnes_set_noise_table first");
    if (!h->theta_set) return fail(h, NICNES_ERR_INVALID, "nicnes_set_theta first");
    if (!h->batch_set) return fail(h, NICNES_ERR_INVALID, "nicnes_set_batch first");
    if (theta && theta_batch >= h->n_batches) return fail(h, NICNES_ERR_INVALID, "batch outside [0, n_batches)");
    HIPC(h, hipSetDevice(h->device));
    if (h->timing) HIPC(h, hipEventRecord(h->ev[0], s));
    h->n_dev = 0;
    h->multi_stream = false;
    if (theta) {
        const int32_t r0 = h->x_row0[(size_t)theta_batch], r1 = h->x_row0[(size_t)theta_batch + 1];
        h->x_last_rows.clear();
        if (int rc = xent_flat(h, &h->xw, h->ref_tokens, h->x_row_img, h->fc, h->n_img, r0, r1, steps_out, s)) return rc;
        HIPC(h, hipMemcpyAsync(fitness_out, h->xw.out, sizeof(double), hipMemcpyDefault, s));
        h->x_last_rows.assign(1, r1 - r0);
        h->x_last_stride = r1 - r0;
    } else {
        const int32_t* mb = nullptr;
        if (int rc = stage_member_batch(h, member_batch_host, count, s, &mb)) return rc;
        std::vector<int32_t> rows((size_t)2 * count);
        int most = 0;
        for (int k = 0; k < count; ++k) {
            const int bk = member_batch_host ? member_batch_host[k] : 0;
            rows[2 * k] = rows[2 * k + 1] = h->x_row0[(size_t)bk + 1] - h->x_row0[(size_t)bk];
            most = std::max(most, rows[2 * k]);
        }
        const int nslabs = (most + 127) / 128, stride = h->x_max_rows;
        h->x_last_rows.clear();
        if (int rc = xent_work_grow(h, &h->xw, (int64_t)count * nslabs, (int64_t)2 * count * stride, 0)) return rc;
        HIPC(h, nicnes_launch_noise_index(h->cfg.noise_seed, iteration, (uint64_t)member_begin, count, h->cfg.noise_len,
                                          (uint64_t)h->D, h->nidx, s));
        if (int rc = ensure_noise_scaled(h, sigma, s)) return rc;
        DecodeParams p = decode_base(h);
        p.theta = h->theta32;
        p.noise = h->noise_sc;
        p.noise_idx = h->nidx;
        p.fc = h->fc;
        p.member_batch = mb;
        p.B_img = h->B;
        p.scratch = h->xw.scratch;
        const XentArgs xa{h->ref_tokens, h->x_row_img, h->img_ref_start, h->xw.lp_sum, h->xw.n_tok, steps_out, h->n_img,
                          0, 0, stride};
        if (steps_out)
            HIPC(h, hipMemsetAsync(steps_out, 0, (size_t)2 * count * stride * (h->cfg.seq_length + 1) * sizeof(float), s));
        HIPC(h, nicnes_launch_xent(&p, &xa, count, nslabs, 2 * count, fitness_out, nullptr, nullptr, s));
        h->x_last_rows = rows;
        h->x_last_stride = stride;
    }
    if (h->timing) {
        HIPC(h, hipEventRecord(h->ev[1], s));
        HIPC(h, hipEventRecord(h->ev[2], s));
    }
    return NICNES_OK;
}

// eval_theta: the sigma = 0 rollout of theta itself (count 1), decoded ONCE: sign + takes the first half of the
// batch's images and sign - the second (at sigma = 0 both signs are theta, so the halves are one decode of the
// batch), scored as one rollout of B rows
// scores_out (nullable, [n_cand, B]): every rollout row's CIDEr-D (the self-critical modes' greedy baseline)
static int evaluate_impl(nicnes_handle* h, uint64_t iteration, int32_t member_begin, int32_t count, float sigma,
                         const int32_t* member_batch_host, double* fitness_out, int32_t* seq_out, float* logprob_out,
                         void* stream, bool eval_theta, double* scores_out = nullptr) {
    if (!h || !fitness_out || member_begin < 0) return NICNES_ERR_INVALID;
    const int mode = h->fitness_mode;
    if (mode == NICNES_FITNESS_XENT) {
        if (seq_out || logprob_out)
            return fail(h, NICNES_ERR_INVALID, "xent fitness: nothing is decoded (seq_out and logprob_out must be NULL)");
        const int tb = !eval_theta ? -1 : (member_batch_host ? member_batch_host[0] : 0);
        return xent_evaluate(h, iteration, member_begin, count, sigma, member_batch_host, tb, fitness_out, nullptr,
                             (hipStream_t)stream);
    }
    const bool sampled = mode >= NICNES_FITNESS_SAMPLE;
    const bool self_critical = mode == NICNES_FITNESS_SELF_CRITICAL || mode == NICNES_FITNESS_SC_LOSS;
    if (self_critical && !scores_out) {
        // the greedy decode of the same rollouts first (compute_ciders, policies.py:174-180): its row scores
        // are the baseline the sampled rows' scores are reduced by
        const int64_t need = (int64_t)2 * h->cfg.max_members * h->cfg.max_batch;
        if (need > h->base_cap) {
            HIPC(h, hipDeviceSynchronize());
            if (h->base_scores) HIPC(h, hipFree(h->base_scores));
            h->base_scores = nullptr;
            h->base_cap = 0;
            int rc = dalloc(h, &h->base_scores, (size_t)need);
            if (rc) return rc;
            h->base_cap = need;
        }
        h->fitness_mode = NICNES_FITNESS_GREEDY;
        const int rc = evaluate_impl(h, iteration, member_begin, count, sigma, member_batch_host, fitness_out, nullptr,
                                     nullptr, stream, eval_theta, h->base_scores);
        h->fitness_mode = mode;
        if (rc) return rc;
    }
    if (count < 1 || count > h->cfg.max_members) return fail(h, NICNES_ERR_INVALID, "count out of [1, max_members]");
    if (!h->noise) return fail(h, NICNES_ERR_INVALID, "nicnes_set_noise_table first");
    if (!h->theta_set) return fail(h, NICNES_ERR_INVALID, "nicnes_set_theta first");
    if (!h->batch_set) return fail(h, NICNES_ERR_INVALID, "nicnes_set_batch first");
    if (h->wide && sampled)
        return fail(h, NICNES_ERR_UNSUPPORTED, wide_what(h) + "the sampled fitness "
                                               "modes are not supported (greedy, greedy_*)");
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    // rollout rows: the images, or rpi copies of each in the sampled modes (the reference's seq_per_img rows);
    // the row buffers grow before anything below takes their addresses
    const int rpi = sampled ? h->rpi : 1;
    const int rows_total = h->B * rpi;
    if (int rc = ensure_rows(h, rows_total)) return rc;
    const int32_t* mb = nullptr;
    if (int rc = stage_member_batch(h, member_batch_host, count, s, &mb)) return rc;
    DecodeParams p = decode_base(h);
    p.theta = h->theta32;
    if (eval_theta) {       // theta itself: a zero slice (the sigma-scaled table is left as it is)
        int rc = ensure_zero_noise(h);
        if (rc) return rc;
        p.noise = h->zero_noise;
        p.noise_idx = h->zero_idx;
    } else {
        HIPC(h, nicnes_launch_noise_index(h->cfg.noise_seed, iteration, (uint64_t)member_begin, count, h->cfg.noise_len,
                                          (uint64_t)h->D, h->nidx, s));
        if (h->mut_mode) {
            h->Dp = (h->D + 63) / 64 * 64;
            if (int rc = ensure_delta_rows(h, &h->dbuf, &h->didx, h->Dp, s)) return rc;
        }
        if (int rc = ensure_noise_scaled(h, sigma, s)) return rc;
        // safe / proportional mutations: the decode reads the members' delta' rows (materialised below, once the
        // decode path is known)
        p.noise = h->mut_mode ? h->dbuf : h->noise_sc;
        p.noise_idx = h->mut_mode ? h->didx : h->nidx;
    }
    MutHead mh{nullptr, nullptr, nullptr, 0};
    p.fc = h->fc;
    p.member_batch = mb;
    p.seq = seq_out ? seq_out : h->seq;
    const bool crit_lp = (mode >= NICNES_FITNESS_GREEDY_LOGPROB && mode <= NICNES_FITNESS_GREEDY_AVGPROB) ||
                         mode == NICNES_FITNESS_SC_LOSS;                // the criterion needs seq_logprobs
    p.lp = logprob_out ? logprob_out : (crit_lp ? h->lp : nullptr);
    p.scratch = h->dscratch;
    p.alive = h->alive;
    if (int rc = lse_poll(h)) return rc;          // the last decode's fallbacks
    const bool bounded = lse_decide(h, !p.lp);
    p.bounded_lse = bounded ? 1 : 0;
    // rows per sign: all of the rollout's rows, or the first half (eval_theta; sign - takes rows half + b)
    const int rows = eval_theta ? (rows_total + 1) / 2 : rows_total;
    int G = 0, nslabs = 0, S = 0;
    decode_shape(h, rows, count, &G, &nslabs, &S);
    if (sampled) {          // the sampled pick runs on the fused path (128-row slabs, one workgroup per slab)
        G = 4;
        S = 1;
        nslabs = nslabs_of(rows, 4);
        const int64_t need = (int64_t)count * 2 * rows * h->cfg.seq_length;
        if (need > h->su_cap) {
            HIPC(h, hipDeviceSynchronize());
            if (h->su) HIPC(h, hipFree(h->su));
            h->su = nullptr;
            h->su_cap = 0;
            int rc = dalloc(h, &h->su, (size_t)need);
            if (rc) return rc;
            h->su_cap = need;
        }
        if (!h->su_host.empty()) {
            if ((int64_t)h->su_host.size() != need)
                return fail(h, NICNES_ERR_INVALID, "nicnes_set_sample_draws: count x 2 x B x seq_length draws needed");
            HIPC(h, hipMemcpyAsync(h->su, h->su_host.data(), (size_t)need * sizeof(double), hipMemcpyHostToDevice, s));
        } else {
            // eval rollouts (eval_theta) draw from a member index no population reaches
            HIPC(h, nicnes_launch_sample_draws(h->cfg.noise_seed, iteration,
                                               eval_theta ? (uint64_t)0xffffffffu : (uint64_t)member_begin, count, rows,
                                               h->cfg.seq_length, h->su, s));
        }
        p.sample_u = h->su;
        if (!h->slog) {
            // a slot per resident workgroup (one per CU: the steps kernel's LDS) plus spares, each holding one
            // step's logits and stage sums of a workgroup's 2 x 128 rows (nst stages of 72 KiB)
            const int ns = h->test_slots > 0 ? h->test_slots : h->sample_occ * h->n_cu + 16;
            // 72 KiB per stage + 8 KiB per block of 8 stages (decode_kernel.hip, SLOG_*)
            const int nst = (h->V1 + 63) / 64;
            const size_t per = (size_t)nst * 18432 + (size_t)((nst + 7) / 8) * 2048;
            HIPC(h, hipDeviceSynchronize());
            int rc = dalloc(h, &h->slog, per * ns);
            if (!rc) rc = dalloc(h, &h->slog_slots, (size_t)ns);
            if (rc) return rc;
            HIPC(h, hipMemset(h->slog_slots, 0, ns * sizeof(int32_t)));
            h->slog_ns = ns;
        }
        p.slog = h->slog;
        p.slog_slots = h->slog_slots;
        p.slog_ns = h->slog_ns;
    }
    if ((int64_t)count * nslabs * S > h->part_cap)
        return fail(h, NICNES_ERR_INVALID, "decode split beyond the partial-state buffer (nicnes_set_decode_split)");
    const ScreenArgs sa = pick_screen(h, count, (int64_t)count * nslabs,
                                      !sampled && !p.lp && bounded && G == 4 && S == 1 && !(h->mut_mode && !eval_theta));
    // the screened decode from the step queue: more member slabs than workers (automatic), or forced on
    QueueArgs qa{nullptr, nullptr, 0, 0};
    {
        const int workers = h->queue_workers > 0 ? h->queue_workers : h->n_cu;
        if (sa.cap && h->queue_ring && (int64_t)count * nslabs <= h->queue_slots &&
            nicnes_queue_use(h->queue_mode, (int64_t)count * nslabs, workers))
            qa = QueueArgs{h->queue_ring, h->queue_ctl, h->queue_slots, workers};
    }
    p.G = G;
    p.S = S;
    p.part = h->part;
    p.coop = !sampled && coop_fits(h, G, nslabs, S, count) ? 1 : 0;
    if (!eval_theta && h->mut_mode) {
        // the members' delta' rows. On the fused greedy path only the parameters from off_log_w on (logit, i2h, h2h,
        // which every step re-reads) are materialised; the decode forms the image projection's and the embedding
        // rows' delta' itself from sigma z and the vector (DecodeParams::mut_head): 5.6 of the 11.5 MB per member
        const bool head = !sampled && !p.coop && G == 4 && S == 1 && !h->mut_full && !h->wide;
        const int64_t j0 = head ? h->off[3] : 0;
        HIPC(h, nicnes_launch_mutate(h->noise + j0, h->nidx, count, h->D - j0, sigma, h->mut_vec + j0, h->mut_mode,
                                     h->dbuf + j0, h->Dp, s));
        if (head) mh = MutHead{h->noise_sc, h->nidx, h->mut_vec, h->mut_mode};
    }
    p.test_stall_ms = h->test_stall_left != 0 ? h->test_stall_ms : 0;
    if (p.coop && h->test_stall_ms && h->test_stall_left > 0) --h->test_stall_left;
    // log-probs of a batch spread over several slabs: every slab runs to T, then the steps after the
    // batch's last finishing step are zeroed (nicnes_lp_batch_exit), as FCModel._sample leaves them
    p.no_exit = (p.lp && nslabs > 1) ? 1 : 0;
    p.coop_ctr = h->coop_ctr;
    p.alive2 = h->alive + h->alive_stride;
    p.alive_stride = h->alive_stride;
    p.B = rows;
    p.B_img = h->B;
    p.rpi = rpi;
    p.sign_off = eval_theta ? rows : 0;
    // eval_theta's output is the one rollout of rows_total rows (with an odd count sign - has one row fewer than
    // sign +), rows s * half + b = image s * half + b
    const size_t out_rows = eval_theta ? (size_t)rows_total : (size_t)count * 2 * rows;
    const int n_cand = eval_theta ? 1 : 2 * count;
    return decode_and_score(h, p, mh, sa, &qa, nullptr, count, nslabs, out_rows, n_cand, rows_total, rpi, mb,
                            self_critical ? h->base_scores : nullptr, fitness_out, scores_out, s);
}

int nicnes_evaluate_batches(nicnes_handle* h, uint64_t iteration, int32_t member_begin, int32_t count, float sigma,
                            const int32_t* member_batch_host, double* fitness_out, int32_t* seq_out, float* logprob_out,
                            void* stream) {
    return evaluate_impl(h, iteration, member_begin, count, sigma, member_batch_host, fitness_out, seq_out, logprob_out,
                         stream, false);
}

int nicnes_evaluate_theta(nicnes_handle* h, int32_t batch, uint64_t iteration, double* fitness_out, int32_t* seq_out,
                          float* logprob_out, void* stream) {
    if (!h) return NICNES_ERR_INVALID;
    if (batch < 0 || (h->batch_set && batch >= h->n_batches)) return fail(h, NICNES_ERR_INVALID, "batch outside [0, n_batches)");
    const int32_t mb = batch;
    return evaluate_impl(h, iteration, 0, 1, 0.f, h->n_batches > 1 ? &mb : nullptr, fitness_out, seq_out, logprob_out,
                         stream, true);
}

int nicnes_xent_rows(nicnes_handle* h, int32_t cand, int32_t rows, double* lp_sum_out, int32_t* n_tok_out, void* stream) {
    if (!h) return NICNES_ERR_INVALID;
    if (h->x_last_rows.empty()) return fail(h, NICNES_ERR_INVALID, "no xent evaluate to read rows of");
    if (cand < 0 || (size_t)cand >= h->x_last_rows.size() || rows < 0 || rows > h->x_last_rows[(size_t)cand])
        return fail(h, NICNES_ERR_INVALID, "candidate or rows outside the last xent evaluate");
    HIPC(h, hipSetDevice(h->device));
    const size_t o = (size_t)cand * (size_t)h->x_last_stride;
    if (lp_sum_out)
        HIPC(h, hipMemcpyAsync(lp_sum_out, h->xw.lp_sum + o, (size_t)rows * sizeof(double), hipMemcpyDefault, (hipStream_t)stream));
    if (n_tok_out)
        HIPC(h, hipMemcpyAsync(n_tok_out, h->xw.n_tok + o, (size_t)rows * sizeof(int32_t), hipMemcpyDefault, (hipStream_t)stream));
    return NICNES_OK;
}

int nicnes_xent_batch_rows(nicnes_handle* h, int32_t batch, int32_t* rows_out_host) {
    if (!h || !rows_out_host) return NICNES_ERR_INVALID;
    if (!h->batch_set) return fail(h, NICNES_ERR_INVALID, "nicnes_set_batch first");
    if (batch < 0 || batch >= h->n_batches) return fail(h, NICNES_ERR_INVALID, "batch outside [0, n_batches)");
    rows_out_host[0] = h->x_row0[(size_t)batch + 1] - h->x_row0[(size_t)batch];
    return NICNES_OK;
}

int nicnes_test_xent_steps(nicnes_handle* h, uint64_t iteration, int32_t member_begin, int32_t count, float sigma,
                           const int32_t* member_batch_host, int32_t theta_batch, double* fitness_out_dev,
                           float* lp_out_dev, void* stream) {
    if (!h || !fitness_out_dev || !lp_out_dev || member_begin < 0) return NICNES_ERR_INVALID;
    return xent_evaluate(h, iteration, member_begin, count, sigma, member_batch_host, theta_batch, fitness_out_dev,
                         lp_out_dev, (hipStream_t)stream);
}

// ---- resident evaluation splits ---------------------------------------------------------------------------------
static void split_free(nicnes_split* sp) {
    void* bufs[] = {sp->fc, sp->ref_tokens, sp->img_ref_start, sp->hash_keys, sp->hash_vals, sp->ref_keys, sp->ref_vec,
                    sp->ref_count, sp->ref_len2, sp->ref_norm, sp->img_stats, sp->img_rouge, sp->img_cider, sp->seq, sp->lp,
                    sp->scratch, sp->alive, sp->coop_ctr, sp->zero_idx, sp->block, sp->part, sp->beam_seq, sp->beam_score,
                    sp->beam_xscr, sp->row_img};
    for (void* q : bufs)
        if (q) (void)hipFree(q);
    xent_work_free(&sp->xw);
    delete sp;
}

static CiderTables split_tables(const nicnes_handle* h, const nicnes_split* sp) {
    CiderTables tb{};
    tb.hash_keys = sp->hash_keys;
    tb.hash_vals = sp->hash_vals;
    tb.hash_mask = sp->hash_mask;
    tb.ref_len = sp->ref_len;
    tb.ref_keys = sp->ref_keys;
    tb.ref_vec = sp->ref_vec;
    tb.ref_count = sp->ref_count;
    tb.ref_len2 = sp->ref_len2;
    tb.ref_norm = sp->ref_norm;
    tb.fault = h->stats;
    return tb;
}

static bool split_of(const nicnes_handle* h, const nicnes_split* sp) {
    return h && sp && std::find(h->splits.begin(), h->splits.end(), sp) != h->splits.end();
}

int nicnes_split_create(nicnes_handle* h, const float* fc, int32_t N, const int32_t* ref_tokens, int32_t n_refs,
                        const int32_t* img_ref_start, const uint64_t* df_keys, const double* df, int64_t n_df,
                        double ref_len_log, nicnes_split** out, void* stream) {
    if (!h || !fc || !out) return NICNES_ERR_INVALID;
    *out = nullptr;
    if (N < 1 || N > (1 << 20)) return fail(h, NICNES_ERR_INVALID, "N out of [1, 2^20]");
    if (n_refs < 0 || n_df < 0) return fail(h, NICNES_ERR_INVALID, "negative count");
    if (n_refs > 0 && (!ref_tokens || !img_ref_start)) return fail(h, NICNES_ERR_INVALID, "references without their arrays");
    if (n_refs > 0 && n_refs < N) return fail(h, NICNES_ERR_INVALID, "n_refs < images");
    if (n_refs > 0 && n_df > 0 && (!df_keys || !df)) return fail(h, NICNES_ERR_INVALID, "df table without its arrays");
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipStreamSynchronize(s));        // the caller's arrays may have been written on its stream
    const size_t F = (size_t)h->cfg.fc_feat_size, T = (size_t)h->cfg.seq_length;
    std::vector<int32_t> st;
    if (n_refs > 0) {                        // reference ranges as nicnes_set_batches checks them
        st.resize((size_t)N + 1);
        HIPC(h, hipMemcpy(st.data(), img_ref_start, st.size() * sizeof(int32_t), hipMemcpyDefault));
        bool ok = st[0] == 0 && st[N] == n_refs;
        for (int b = 0; b < N && ok; ++b) ok = st[b + 1] > st[b];
        if (!ok)
            return fail(h, NICNES_ERR_INVALID,
                        "img_ref_start must start at 0, end at n_refs and give every image >= 1 reference");
    }
    nicnes_split* sp = new nicnes_split();
    sp->h = h;
    sp->N = N;
    sp->n_refs = n_refs;
    sp->ref_len = ref_len_log;
    uint64_t* tk = nullptr;                  // the caller's df table on the device, while the hash copy is built
    double* tv = nullptr;
    auto run = [&]() -> int {
        const size_t pad = 2 * SPLIT_ROWS;
        int rc = dalloc(h, &sp->fc, ((size_t)N + pad) * F);
        if (rc) return rc;
        HIPC(h, hipMemcpy(sp->fc, fc, (size_t)N * F * sizeof(float), hipMemcpyDefault));
        HIPC(h, hipMemset(sp->fc + (size_t)N * F, 0, pad * F * sizeof(float)));
        if (n_refs == 0) return NICNES_OK;  // a decode-only split
        const size_t NR = (size_t)n_refs;
        rc = dalloc(h, &sp->ref_tokens, NR * T);
        if (!rc) rc = dalloc(h, &sp->img_ref_start, (size_t)N + 1);
        if (!rc) rc = dalloc(h, &sp->ref_keys, NR * 64);
        if (!rc) rc = dalloc(h, &sp->ref_vec, NR * 64);
        if (!rc) rc = dalloc(h, &sp->ref_count, NR);
        if (!rc) rc = dalloc(h, &sp->ref_len2, NR);
        if (!rc) rc = dalloc(h, &sp->ref_norm, NR * 4);
        if (!rc) rc = dalloc(h, &sp->img_stats, (size_t)N * 10);
        if (!rc) rc = dalloc(h, &sp->img_rouge, (size_t)N);
        if (!rc) rc = dalloc(h, &sp->img_cider, (size_t)N);
        const uint64_t cap = nicnes_df_hash_capacity(n_df);
        if (!rc) rc = dalloc(h, &sp->hash_keys, cap);
        if (!rc) rc = dalloc(h, &sp->hash_vals, cap);
        if (rc) return rc;
        HIPC(h, hipMemcpy(sp->ref_tokens, ref_tokens, NR * T * sizeof(int32_t), hipMemcpyDefault));
        HIPC(h, hipMemcpy(sp->img_ref_start, st.data(), st.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        sp->start_host = st;
        rc = dalloc(h, &sp->row_img, NR);
        if (rc) return rc;
        HIPC(h, nicnes_launch_xent_row_map(sp->img_ref_start, N, sp->row_img, s));
        HIPC(h, hipMemset(sp->hash_keys, 0, cap * sizeof(uint64_t)));
        sp->hash_mask = cap - 1;
        if (n_df > 0) {
            rc = dalloc(h, &tk, (size_t)n_df);
            if (!rc) rc = dalloc(h, &tv, (size_t)n_df);
            if (rc) return rc;
            HIPC(h, hipMemcpy(tk, df_keys, (size_t)n_df * sizeof(uint64_t), hipMemcpyDefault));
            HIPC(h, hipMemcpy(tv, df, (size_t)n_df * sizeof(double), hipMemcpyDefault));
            HIPC(h, nicnes_launch_df_hash_build(tk, tv, n_df, sp->hash_keys, sp->hash_vals, sp->hash_mask, s));
        }
        const CiderTables tb = split_tables(h, sp);
        HIPC(h, nicnes_launch_cook_refs(sp->ref_tokens, n_refs, (int)T, &tb, s, 1));
        HIPC(h, hipStreamSynchronize(s));
        return NICNES_OK;
    };
    const int rc = run();
    if (tk) (void)hipFree(tk);
    if (tv) (void)hipFree(tv);
    if (rc) {
        split_free(sp);
        return rc;
    }
    h->splits.push_back(sp);
    *out = sp;
    return NICNES_OK;
}

int nicnes_split_destroy(nicnes_handle* h, nicnes_split* sp) {
    if (!h) return NICNES_ERR_INVALID;
    if (!sp) return NICNES_OK;
    if (!split_of(h, sp)) return fail(h, NICNES_ERR_INVALID, "not a split of this handle");
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipDeviceSynchronize());
    h->splits.erase(std::find(h->splits.begin(), h->splits.end(), sp));
    split_free(sp);
    return NICNES_OK;
}

// the decode work buffers for n_pm pseudo-members and n_lwg logit workgroups (grown outside every launch)
static int split_grow(nicnes_handle* h, nicnes_split* sp, int n_pm, int64_t n_lwg) {
    const size_t T = (size_t)h->cfg.seq_length;
    if (n_pm > sp->pm_cap) {
        HIPC(h, hipDeviceSynchronize());
        void* old[] = {sp->seq, sp->lp, sp->scratch, sp->alive, sp->coop_ctr, sp->zero_idx, sp->block};
        for (void* q : old)
            if (q) (void)hipFree(q);
        sp->seq = nullptr; sp->lp = nullptr; sp->scratch = nullptr; sp->alive = nullptr; sp->coop_ctr = nullptr;
        sp->zero_idx = nullptr; sp->block = nullptr;
        sp->pm_cap = 0;
        const size_t PM = (size_t)n_pm, rows = PM * 2 * SPLIT_ROWS;
        // a pseudo-member is one 128-row slab or two 64-row slabs: 8 row waves of lane scratch, <= 2 workgroups
        int rc = dalloc(h, &sp->seq, rows * T);
        if (!rc) rc = dalloc(h, &sp->lp, rows * T);
        const size_t wide_fl = !h->wide ? 0 : nicnes_wide_scratch_floats(n_pm, h->cfg.input_encoding_size,
                                                                         h->cfg.rnn_size, h->ln);
        if (!rc) rc = dalloc(h, &sp->scratch, std::max(nicnes_decode_scratch_floats(n_pm, 8), wide_fl));
        if (!rc) rc = dalloc(h, &sp->alive, 3 * 2 * PM);
        if (!rc) rc = dalloc(h, &sp->coop_ctr, 2 * PM * COOP_CTR_STRIDE);
        if (!rc) rc = dalloc(h, &sp->zero_idx, PM);
        if (!rc) rc = dalloc(h, &sp->block, PM);
        if (rc) return rc;
        std::vector<int32_t> iota(PM);
        for (size_t k = 0; k < PM; ++k) iota[k] = (int32_t)k;
        HIPC(h, hipMemcpy(sp->block, iota.data(), PM * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPC(h, hipMemset(sp->zero_idx, 0, PM * sizeof(uint64_t)));
        sp->pm_cap = n_pm;
    }
    if (n_lwg > sp->wg_cap) {
        HIPC(h, hipDeviceSynchronize());
        if (sp->part) (void)hipFree(sp->part);
        sp->part = nullptr;
        sp->wg_cap = 0;
        int rc = dalloc(h, &sp->part, (size_t)n_lwg * PART_FLOATS);
        if (rc) return rc;
        sp->wg_cap = n_lwg;
    }
    return NICNES_OK;
}

// log-probs of the steps after a row's end token are 0 (a decode leaves what its workgroup's other rows still ran)
__global__ void split_lp_mask_kernel(const int32_t* seq, float* lp, int rows, int T) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= rows) return;
    bool ended = false;
    for (int t = 0; t < T; ++t) {
        if (ended) lp[(size_t)b * T + t] = 0.f;
        if (seq[(size_t)b * T + t] == 0) ended = true;
    }
}

// The greedy decode of theta on images [first, first + count), every slab in one enqueue: nicnes_evaluate_theta's
// halves (sign_off, the zero noise slice, member_batch) over ceil(count / 256) pseudo-members, pseudo-member k
// decoding images first + 256 k + (0..127) as its sign + and the next 128 as its sign -. Rows past the range are
// decoded (other images of the split, or the zero rows behind it) and dropped. *seq_dev: the tokens in the split's
// own buffer [count, T]; seq_out / lp_out (nullable) receive copies.
static int split_decode_impl(nicnes_handle* h, nicnes_split* sp, int32_t first, int32_t count, int32_t* seq_out,
                             float* lp_out, hipStream_t s, const int32_t** seq_dev) {
    if (!split_of(h, sp)) return fail(h, NICNES_ERR_INVALID, "not a split of this handle");
    if (first < 0 || count < 1 || (int64_t)first + count > sp->N)
        return fail(h, NICNES_ERR_INVALID, "range outside the split's images");
    if (!h->theta_set) return fail(h, NICNES_ERR_INVALID, "nicnes_set_theta first");
    HIPC(h, hipSetDevice(h->device));
    const int per = 2 * SPLIT_ROWS, n_pm = (count + per - 1) / per;
    if (n_pm > SPLIT_MAX_PM) return fail(h, NICNES_ERR_INVALID, "range beyond the decode buffers");
    int G = 0, nslabs = 0, S = 0;
    decode_shape(h, SPLIT_ROWS, n_pm, &G, &nslabs, &S);
    if (int rc = ensure_zero_noise(h)) return rc;
    if (int rc = split_grow(h, sp, n_pm, (int64_t)n_pm * nslabs * S)) return rc;
    const int T = h->cfg.seq_length;
    DecodeParams p = decode_base(h);
    p.theta = h->theta32;
    p.noise = h->zero_noise;
    p.noise_idx = sp->zero_idx;
    p.fc = sp->fc + (size_t)first * h->cfg.fc_feat_size;
    p.member_batch = sp->block;
    p.seq = sp->seq;
    p.lp = lp_out ? sp->lp : nullptr;
    p.scratch = sp->scratch;
    p.alive = sp->alive;
    p.alive_stride = 2 * sp->pm_cap;
    p.alive2 = sp->alive + p.alive_stride;
    p.part = sp->part;
    p.coop_ctr = sp->coop_ctr;
    // the lse mode of the engine's policy as it stands; the policy's own state and the counter read-back belong to the
    // evaluates
    const bool bounded = lse_bounded_now(h);
    p.bounded_lse = bounded ? 1 : 0;
    const ScreenArgs sa = pick_screen(h, n_pm, (int64_t)n_pm * nslabs, !p.lp && bounded && G == 4 && S == 1);
    p.G = G;
    p.S = S;
    p.coop = coop_fits(h, G, nslabs, S, n_pm) ? 1 : 0;
    // (no_exit stays 0: a row's log-probs up to its own end token are written before its workgroup exits)
    p.B = SPLIT_ROWS;
    p.B_img = per;
    p.rpi = 1;
    p.sign_off = SPLIT_ROWS;
    const size_t out_rows = (size_t)n_pm * per;
    HIPC(h, hipMemsetAsync(p.seq, 0, out_rows * T * sizeof(int32_t), s));
    if (p.lp) HIPC(h, hipMemsetAsync(p.lp, 0, out_rows * T * sizeof(float), s));
    const MutHead mh{nullptr, nullptr, nullptr, 0};
    const int nstr = launch_decode_parts(h, p, mh, sa, nullptr, nullptr, n_pm, nslabs, s, false, nullptr);
    if (nstr < 0) return -nstr;
    if (p.lp) {
        hipLaunchKernelGGL(split_lp_mask_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s,
                           (const int32_t*)p.seq, p.lp, count, T);
        HIPC(h, hipGetLastError());
        HIPC(h, hipMemcpyAsync(lp_out, p.lp, (size_t)count * T * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    if (seq_out) HIPC(h, hipMemcpyAsync(seq_out, p.seq, (size_t)count * T * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (seq_dev) *seq_dev = p.seq;
    return NICNES_OK;
}

int nicnes_split_decode(nicnes_handle* h, nicnes_split* sp, int32_t first, int32_t count, int32_t* seq_out,
                        float* lp_out, void* stream) {
    if (!h || !sp || !seq_out) return NICNES_ERR_INVALID;
    return split_decode_impl(h, sp, first, count, seq_out, lp_out, (hipStream_t)stream, nullptr);
}

static int split_score_impl(nicnes_handle* h, nicnes_split* sp, int32_t first, int32_t count, const int32_t* seq,
                            int64_t* totals_out, double* metrics_out, double* row_cider_out, hipStream_t s) {
    if (!split_of(h, sp)) return fail(h, NICNES_ERR_INVALID, "not a split of this handle");
    if (sp->n_refs == 0) return fail(h, NICNES_ERR_INVALID, "a decode-only split has no references to score against");
    if (first < 0 || count < 1 || (int64_t)first + count > sp->N)
        return fail(h, NICNES_ERR_INVALID, "range outside the split's images");
    HIPC(h, hipSetDevice(h->device));
    const CiderTables tb = split_tables(h, sp);
    HIPC(h, nicnes_launch_split_metrics(seq, first, count, h->cfg.seq_length, &tb, sp->img_ref_start, sp->ref_tokens,
                                        sp->img_stats, sp->img_rouge, sp->img_cider, totals_out, metrics_out, s));
    if (row_cider_out)
        HIPC(h, hipMemcpyAsync(row_cider_out, sp->img_cider, (size_t)count * sizeof(double), hipMemcpyDeviceToDevice, s));
    return NICNES_OK;
}

int nicnes_split_score(nicnes_handle* h, nicnes_split* sp, int32_t first, int32_t count, const int32_t* seq_dev,
                       int64_t* totals_out_dev, double* metrics_out_dev, double* row_cider_out_dev, void* stream) {
    if (!h || !sp || !seq_dev || !totals_out_dev || !metrics_out_dev) return NICNES_ERR_INVALID;
    return split_score_impl(h, sp, first, count, seq_dev, totals_out_dev, metrics_out_dev, row_cider_out_dev,
                            (hipStream_t)stream);
}

int nicnes_split_evaluate(nicnes_handle* h, nicnes_split* sp, int32_t first, int32_t count, int64_t* totals_out_dev,
                          double* metrics_out_dev, double* row_cider_out_dev, int32_t* seq_out, void* stream) {
    if (!h || !sp || !totals_out_dev || !metrics_out_dev) return NICNES_ERR_INVALID;
    if (split_of(h, sp) && sp->n_refs == 0)
        return fail(h, NICNES_ERR_INVALID, "a decode-only split has no references to score against");
    const int32_t* seq = nullptr;
    if (int rc = split_decode_impl(h, sp, first, count, seq_out, nullptr, (hipStream_t)stream, &seq)) return rc;
    return split_score_impl(h, sp, first, count, seq, totals_out_dev, metrics_out_dev, row_cider_out_dev,
                            (hipStream_t)stream);
}

int nicnes_split_xent(nicnes_handle* h, nicnes_split* sp, int32_t first, int32_t count, double* out2_dev,
                      int64_t* tokens_out_dev, double* lp_sum_out_dev, int32_t* n_tok_out_dev, void* stream) {
    if (!h || !sp || !out2_dev) return NICNES_ERR_INVALID;
    if (!split_of(h, sp)) return fail(h, NICNES_ERR_INVALID, "not a split of this handle");
    if (h->wide) return fail(h, NICNES_ERR_UNSUPPORTED, wide_what(h) + "the xent loss is not supported (E = R = 128 only)");
    if (sp->n_refs == 0) return fail(h, NICNES_ERR_UNSUPPORTED, "a decode-only split has no label rows for the xent loss");
    if (first < 0 || count < 1 || (int64_t)first + count > sp->N)
        return fail(h, NICNES_ERR_INVALID, "range outside the split's images");
    if (!h->theta_set) return fail(h, NICNES_ERR_INVALID, "nicnes_set_theta first");
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    const int32_t r0 = sp->start_host[(size_t)first], r1 = sp->start_host[(size_t)first + count];
    if (int rc = xent_flat(h, &sp->xw, sp->ref_tokens, sp->row_img, sp->fc, sp->N, r0, r1, nullptr, s)) return rc;
    const size_t rows = (size_t)(r1 - r0);
    HIPC(h, hipMemcpyAsync(out2_dev, sp->xw.out + 1, 2 * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (tokens_out_dev) HIPC(h, hipMemcpyAsync(tokens_out_dev, sp->xw.out + 3, sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    if (lp_sum_out_dev)
        HIPC(h, hipMemcpyAsync(lp_sum_out_dev, sp->xw.lp_sum, rows * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (n_tok_out_dev)
        HIPC(h, hipMemcpyAsync(n_tok_out_dev, sp->xw.n_tok, rows * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return NICNES_OK;
}

// ---- beam-search decode of a split (evaluation only; beam_kernels.hip) ------------------------------------------------
static int split_beam_grow(nicnes_handle* h, nicnes_split* sp, int32_t count, int32_t beam) {
    const size_t T = (size_t)h->cfg.seq_length;
    if (count > sp->beam_rows) {
        HIPC(h, hipDeviceSynchronize());
        if (sp->beam_seq) (void)hipFree(sp->beam_seq);
        if (sp->beam_score) (void)hipFree(sp->beam_score);
        sp->beam_seq = nullptr; sp->beam_score = nullptr;
        sp->beam_rows = 0;
        int rc = dalloc(h, &sp->beam_seq, (size_t)count * T);
        if (!rc) rc = dalloc(h, &sp->beam_score, (size_t)count);
        if (rc) return rc;
        sp->beam_rows = count;
    }
    const size_t need = nicnes_beam_scratch_floats(count, beam);
    if (need > sp->beam_scr) {
        HIPC(h, hipDeviceSynchronize());
        if (sp->beam_xscr) (void)hipFree(sp->beam_xscr);
        sp->beam_xscr = nullptr;
        sp->beam_scr = 0;
        int rc = dalloc(h, &sp->beam_xscr, need);
        if (rc) return rc;
        sp->beam_scr = need;
    }
    return NICNES_OK;
}

// The beam decode of theta on images [first, first + count) in one enqueue. *seq_dev: the tokens in the split's own
// buffer [count, T]; seq_out / score_out (nullable) receive copies.
static int split_decode_beam_impl(nicnes_handle* h, nicnes_split* sp, int32_t first, int32_t count, int32_t beam,
                                  int32_t* seq_out, double* score_out, hipStream_t s, const int32_t** seq_dev) {
    if (!split_of(h, sp)) return fail(h, NICNES_ERR_INVALID, "not a split of this handle");
    if (beam < 1 || beam > 8) return fail(h, NICNES_ERR_INVALID, "beam out of [1, 8]");
    if (h->wide)
        return fail(h, NICNES_ERR_UNSUPPORTED, wide_what(h) + "the beam decode is "
                                               "not supported");
    if (first < 0 || count < 1 || (int64_t)first + count > sp->N)
        return fail(h, NICNES_ERR_INVALID, "range outside the split's images");
    if (!h->theta_set) return fail(h, NICNES_ERR_INVALID, "nicnes_set_theta first");
    HIPC(h, hipSetDevice(h->device));
    if (int rc = split_beam_grow(h, sp, count, beam)) return rc;
    const size_t T = (size_t)h->cfg.seq_length;
    DecodeParams p = decode_base(h);
    p.theta = h->theta32;
    p.fc = sp->fc + (size_t)first * h->cfg.fc_feat_size;
    HIPC(h, nicnes_launch_beam_decode(&p, sp->beam_seq, sp->beam_score, sp->beam_xscr, count, beam, h->n_cu,
                                      h->beam_waves, s));
    if (seq_out)
        HIPC(h, hipMemcpyAsync(seq_out, sp->beam_seq, (size_t)count * T * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (score_out)
        HIPC(h, hipMemcpyAsync(score_out, sp->beam_score, (size_t)count * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (seq_dev) *seq_dev = sp->beam_seq;
    return NICNES_OK;
}

int nicnes_split_decode_beam(nicnes_handle* h, nicnes_split* sp, int32_t first, int32_t count, int32_t beam,
                             int32_t* seq_out, double* score_out, void* stream) {
    if (!h || !sp || !seq_out) return NICNES_ERR_INVALID;
    return split_decode_beam_impl(h, sp, first, count, beam, seq_out, score_out, (hipStream_t)stream, nullptr);
}

int nicnes_split_evaluate_beam(nicnes_handle* h, nicnes_split* sp, int32_t first, int32_t count, int32_t beam,
                               int64_t* totals_out_dev, double* metrics_out_dev, double* row_cider_out_dev,
                               int32_t* seq_out, void* stream) {
    if (!h || !sp || !totals_out_dev || !metrics_out_dev) return NICNES_ERR_INVALID;
    if (split_of(h, sp) && sp->n_refs == 0)
        return fail(h, NICNES_ERR_INVALID, "a decode-only split has no references to score against");
    const int32_t* seq = nullptr;
    if (int rc = split_decode_beam_impl(h, sp, first, count, beam, seq_out, nullptr, (hipStream_t)stream, &seq)) return rc;
    return split_score_impl(h, sp, first, count, seq, totals_out_dev, metrics_out_dev, row_cider_out_dev,
                            (hipStream_t)stream);
}

int nicnes_set_beam_waves(nicnes_handle* h, int32_t waves) {
    if (!h || (waves != 0 && waves != 4 && waves != 8)) return NICNES_ERR_INVALID;
    h->beam_waves = waves;
    return NICNES_OK;
}

int nicnes_test_beam_select(nicnes_handle* h, const float* lp_dev, const double* score_dev, const int32_t* live_dev,
                            int32_t n_img, int32_t beam, int32_t V1, int32_t* out_dev, void* stream) {
    if (!h || !lp_dev || !score_dev || !live_dev || !out_dev) return NICNES_ERR_INVALID;
    if (beam < 1 || beam > 8) return fail(h, NICNES_ERR_INVALID, "beam out of [1, 8]");
    if (n_img < 1 || V1 < 1) return fail(h, NICNES_ERR_INVALID, "n_img and V1 must be positive");
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipMemsetAsync(out_dev, 0xff, (size_t)n_img * beam * 2 * sizeof(int32_t), s));
    HIPC(h, nicnes_launch_test_beam_select(lp_dev, score_dev, live_dev, n_img, beam, V1, out_dev, s));
    return NICNES_OK;
}

// The SM-G-SUM sensitivity of `theta` (the handle's theta32, or a parent row of nicnes_sensitivity_es) on the first
// `rows` images of the batch held, into out [D]
static const int SENS_L = 5;                                       // forward_for_sensitivity's length (nets.py:22)

// the embedding kernels list every (cell, row) pair in LDS: SENS_L * rows <= NICNES_SENS_MAX_PAIRS, refused by name
// before anything is allocated or enqueued (nicnes_sens_run keeps its own check)
static int sens_rows_fit(nicnes_handle* h, int32_t rows) {
    const int max_rows = NICNES_SENS_MAX_PAIRS / SENS_L;
    if (rows > max_rows)
        return fail(h, NICNES_ERR_UNSUPPORTED, "the SM-G-SUM sensitivity takes rows <= " + std::to_string(max_rows) +
                                               " (" + std::to_string(SENS_L) + " * rows <= " +
                                               std::to_string(NICNES_SENS_MAX_PAIRS) + " token cells), got " +
                                               std::to_string(rows));
    return NICNES_OK;
}

static int sens_of_theta(nicnes_handle* h, const float* theta, int32_t rows, float underflow, float* out, hipStream_t s) {
    const int L = SENS_L, split = 100;                             // forward_for_sensitivity defaults (nets.py:22)
    if (!h->sens_tok) {
        HIPC(h, hipDeviceSynchronize());
        int rc = dalloc(h, &h->sens_tok, (size_t)2 * h->cfg.max_batch * (L - 1));
        if (rc) return rc;
        h->sens = nicnes_sens_create();
    }
    SensParams sp;
    sp.theta = theta;
    sp.fc = h->fc;
    sp.tok = h->sens_tok;                                          // [rows, L - 1], written by the forward
    sp.tok_stride = L - 1;
    sp.tok_internal = 1;
    sp.Bs = rows;
    sp.V1 = h->V1;
    sp.E = h->cfg.input_encoding_size;
    sp.R = h->cfg.rnn_size;
    sp.F = h->cfg.fc_feat_size;
    sp.L = L;
    sp.split = split;
    sp.K = h->V1 / split + 1;
    sp.D = h->D;
    sp.off_img_w = h->off[0]; sp.off_img_b = h->off[1]; sp.off_emb_w = h->off[2]; sp.off_log_w = h->off[3];
    sp.off_log_b = h->off[4]; sp.off_i2h_w = h->off[5]; sp.off_i2h_b = h->off[6]; sp.off_h2h_w = h->off[7];
    sp.off_h2h_b = h->off[8];
    sp.underflow = underflow;
    sp.out = out;
    const int rc = nicnes_sens_run(h->sens, &sp, s);
    if (rc) return fail(h, NICNES_ERR_HIP, "sensitivity kernels failed (code " + std::to_string(rc) + ")");
    return NICNES_OK;
}

int nicnes_sum_sensitivity(nicnes_handle* h, int32_t rows, float underflow, float* out, void* stream) {
    if (!h || !out || rows < 1) return NICNES_ERR_INVALID;
    if (h->wide)
        return fail(h, NICNES_ERR_UNSUPPORTED, wide_what(h) + "the SM-G-SUM "
                                               "sensitivity is not supported");
    if (!h->theta_set) return fail(h, NICNES_ERR_INVALID, "nicnes_set_theta first");
    if (!h->batch_set) return fail(h, NICNES_ERR_INVALID, "nicnes_set_batch first");
    if (rows > h->B) return fail(h, NICNES_ERR_INVALID, "rows beyond the batch held");
    if (int rc = sens_rows_fit(h, rows)) return rc;
    HIPC(h, hipSetDevice(h->device));
    return sens_of_theta(h, h->theta32, rows, underflow, out, (hipStream_t)stream);
}

int nicnes_sens_paths(nicnes_handle* h, int32_t* out_host) {
    if (!h || !out_host) return NICNES_ERR_INVALID;
    if (!h->sens || nicnes_sens_last_paths(h->sens, out_host))
        return fail(h, NICNES_ERR_INVALID, "nicnes_sum_sensitivity or nicnes_sensitivity_es first");
    return NICNES_OK;
}

int nicnes_rank_weights(nicnes_handle* h, const double* fitness, int32_t P, double* cr_out, float* w_out, void* stream) {
    if (!h || !fitness || !w_out || P < 1) return NICNES_ERR_INVALID;
    if (P > (1 << 29)) return fail(h, NICNES_ERR_UNSUPPORTED, "P > 2^29");
    HIPC(h, hipSetDevice(h->device));
    const size_t need = nicnes_rank_scratch_pairs(2 * P);
    if (need > h->rank_cap) {       // the first call at a larger population grows the sort scratch
        HIPC(h, hipStreamSynchronize((hipStream_t)stream));
        if (h->rank_key) (void)hipFree(h->rank_key);
        if (h->rank_idx) (void)hipFree(h->rank_idx);
        h->rank_key = nullptr;
        h->rank_idx = nullptr;
        h->rank_cap = 0;
        int rc = dalloc(h, &h->rank_key, need);
        if (!rc) rc = dalloc(h, &h->rank_idx, need);
        if (rc) return rc;
        h->rank_cap = need;
    }
    HIPC(h, nicnes_launch_rank(fitness, 2 * P, h->rank_key, h->rank_idx, cr_out, w_out, (hipStream_t)stream));
    return NICNES_OK;
}

int nicnes_grad_partial(nicnes_handle* h, uint64_t iteration, int32_t member_begin, int32_t count, const float* w,
                        float sigma, float* gsum_out, void* stream) {
    if (!h || !w || !gsum_out || member_begin < 0 || count < 0) return NICNES_ERR_INVALID;
    if (count > h->cfg.max_members) return fail(h, NICNES_ERR_INVALID, "count > max_members");
    if (!h->noise) return fail(h, NICNES_ERR_INVALID, "nicnes_set_noise_table first");
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, nicnes_launch_noise_index(h->cfg.noise_seed, iteration, (uint64_t)member_begin, count, h->cfg.noise_len,
                                      (uint64_t)h->D, h->nidx, s));
    // with a mutation the reference sums the mutated noise vectors it was sent (nic_nes_worker.py:156-161):
    // the kernel transforms each delta on the fly
    HIPC(h, nicnes_launch_grad(h->noise, h->nidx, w, count, sigma, h->D, h->mut_vec, h->mut_mode, gsum_out, s,
                               h->stats));
    return NICNES_OK;
}

int nicnes_grad_partial_range(nicnes_handle* h, uint64_t iteration, int32_t member_begin, int32_t count, const float* w,
                              float sigma, int64_t j0, int64_t j1, float* gsum_out, void* stream) {
    if (!h || !w || !gsum_out || member_begin < 0 || count < 0) return NICNES_ERR_INVALID;
    if (j0 < 0 || j1 > h->D || j0 >= j1 || (j0 & 63)) return fail(h, NICNES_ERR_INVALID, "range: 0 <= j0 < j1 <= D, j0 % 64 == 0");
    if (count > h->cfg.max_members) return fail(h, NICNES_ERR_INVALID, "count > max_members");
    if (!h->noise) return fail(h, NICNES_ERR_INVALID, "nicnes_set_noise_table first");
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, nicnes_launch_noise_index(h->cfg.noise_seed, iteration, (uint64_t)member_begin, count, h->cfg.noise_len,
                                      (uint64_t)h->D, h->nidx, s));
    // the same kernel on the parameter range (slices are 64-float aligned, so j0 % 64 keeps the f32x4 loads aligned)
    HIPC(h, nicnes_launch_grad(h->noise + j0, h->nidx, w, count, sigma, j1 - j0, h->mut_vec ? h->mut_vec + j0 : nullptr,
                               h->mut_mode, gsum_out + j0, s, h->stats));
    return NICNES_OK;
}

// A skipped optimizer step (NaN ratio, nicnes_adam_kernel): say why. This handle's decode lost rows (its
// counters), or another rank's did (the all-reduced noise sum came back NaN).
static int fault_error(nicnes_handle* h, bool from_noise_sum = true) {
    int32_t st[4];
    HIPC(h, hipMemcpy(st, h->stats, sizeof st, hipMemcpyDeviceToHost));
    if (st[2] != 0) return fail(h, NICNES_ERR_FAULT, "coop decode: a workgroup's partners never arrived (hand-off timeout); "
                                                     "the iteration's fitness is NaN and the optimizer step was skipped");
    if (st[3] != 0) return fail(h, NICNES_ERR_FAULT, "sampled decode: a workgroup found no free logit slot; "
                                                     "the iteration's fitness is NaN and the optimizer step was skipped");
    if (!from_noise_sum) return NICNES_OK;      // Optimizer.update(globalg) with a NaN globalg: as the reference
    return fail(h, NICNES_ERR_FAULT, "optimizer step skipped: the noise sum is NaN (a faulted decode on another rank)");
}

// the newest step was skipped (its flag read back as set): undo its host-side state once
static void rollback_skipped_step(nicnes_handle* h) {
    if (!h->step_pending_check) return;
    h->t = h->t_prev;
    h->theta_is_fp32 = h->theta_fp32_prev;
    h->step_pending_check = false;
}

// one optimizer update (kind 0 Adam, 1 SGD), from the fused NES form (gsum, P, l2coeff) or from a
// given globalg (Optimizer.update(globalg), optimizers.py:15-22)
static int opt_step(nicnes_handle* h, int kind, const float* gsum, int32_t P, double l2coeff, const double* globalg,
                    int globalg_fp32, double stepsize, double b1, double b2, double epsilon, double* ratio_out_host, void* stream) {
    if (!h->theta_set) return fail(h, NICNES_ERR_INVALID, "nicnes_set_theta first");
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    h->t_prev = h->t;
    h->theta_fp32_prev = h->theta_is_fp32;
    h->step_pending_check = true;
    h->t += 1;
    AdamParams p;
    p.theta64 = h->theta64;
    p.theta32 = h->theta32;
    p.m = h->m;
    p.v = h->v;
    p.gsum = gsum;
    p.globalg = globalg;
    p.partials = h->partials;
    p.dim = h->D;
    p.two_f = (float)(2 * (P > 0 ? P : 1));
    p.theta_is_fp32 = h->theta_is_fp32;
    p.l2coeff = l2coeff;
    p.l2coeff32 = (float)l2coeff;
    p.kind = kind;
    // fused form: g' is fp32 exactly while theta is (nic_nes_master.py:126-133)
    p.g_is_fp32 = globalg ? (globalg_fp32 != 0) : h->theta_is_fp32;
    // Adam: a = stepsize * sqrt(1 - b2^t) / (1 - b1^t)   (optimizers.py:79, Python float arithmetic)
    p.a = kind == 0 ? stepsize * std::sqrt(1.0 - std::pow(b2, (double)h->t)) / (1.0 - std::pow(b1, (double)h->t)) : 0.0;
    p.neg_stepsize = -stepsize;
    p.beta1 = b1;                      // SGD: momentum
    p.beta2 = b2;
    p.one_minus_beta1 = 1.0 - b1;
    p.one_minus_beta2 = 1.0 - b2;
    p.one_minus_beta1_32 = (float)(1.0 - b1);
    p.one_minus_beta2_32 = (float)(1.0 - b2);
    p.epsilon = epsilon;
    p.fault = h->stats;
    p.skip_out = h->norms + 2;
    h->last_nes_form = globalg == nullptr;
    HIPC(h, nicnes_launch_adam(&p, h->norms, s));
    h->theta_is_fp32 = 0;
    if (ratio_out_host) {
        double n3[3];
        HIPC(h, hipMemcpyAsync(n3, h->norms, sizeof n3, hipMemcpyDeviceToHost, s));
        HIPC(h, hipStreamSynchronize(s));
        *ratio_out_host = std::sqrt(n3[0]) / std::sqrt(n3[1]);
        if (n3[2] != 0.0) {
            rollback_skipped_step(h);
            return fault_error(h, globalg == nullptr);
        }
        h->step_pending_check = false;
    }
    return NICNES_OK;
}

int nicnes_last_ratio(nicnes_handle* h, double* ratio_out_host, void* stream) {
    if (!h || !ratio_out_host) return NICNES_ERR_INVALID;
    if (h->t == 0) return fail(h, NICNES_ERR_INVALID, "no optimizer step yet");
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    double n3[3];
    HIPC(h, hipMemcpyAsync(n3, h->norms, sizeof n3, hipMemcpyDeviceToHost, s));
    HIPC(h, hipStreamSynchronize(s));
    *ratio_out_host = std::sqrt(n3[0]) / std::sqrt(n3[1]);
    if (n3[2] != 0.0) {
        rollback_skipped_step(h);
        return fault_error(h, h->last_nes_form);
    }
    h->step_pending_check = false;
    return NICNES_OK;
}

int nicnes_clear_faults(nicnes_handle* h, int64_t* counters_out_host) {
    if (!h) return NICNES_ERR_INVALID;
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipDeviceSynchronize());            // every launch that could still count has finished
    int32_t st[4];
    HIPC(h, hipMemcpy(st, h->stats, sizeof st, hipMemcpyDeviceToHost));
    if (h->step_pending_check) {                 // the newest step's skip flag was not read yet
        double skip = 0.0;
        HIPC(h, hipMemcpy(&skip, h->norms + 2, sizeof skip, hipMemcpyDeviceToHost));
        if (skip != 0.0) rollback_skipped_step(h);
        else h->step_pending_check = false;
    }
    if (counters_out_host) {
        counters_out_host[0] = st[2];
        counters_out_host[1] = st[3];
    }
    // zero the fault words only (the fallback counters [0], [1] keep counting) and the logit-slot claim flags
    // (the coop hand-off counters are zeroed before every coop launch), then forget the pending read-back
    // that carried the fault
    HIPC(h, hipMemset(h->stats + 2, 0, 2 * sizeof(int32_t)));
    if (h->slog_slots) HIPC(h, hipMemset(h->slog_slots, 0, (size_t)h->slog_ns * sizeof(int32_t)));
    HIPC(h, hipDeviceSynchronize());
    h->stats_pending = false;
    return NICNES_OK;
}

int nicnes_adam_step(nicnes_handle* h, const float* gsum, int32_t P, double l2coeff, double stepsize, double beta1,
                     double beta2, double epsilon, double* ratio_out_host, void* stream) {
    if (!h || !gsum || P < 1) return NICNES_ERR_INVALID;
    return opt_step(h, 0, gsum, P, l2coeff, nullptr, 0, stepsize, beta1, beta2, epsilon, ratio_out_host, stream);
}

int nicnes_sgd_step(nicnes_handle* h, const float* gsum, int32_t P, double l2coeff, double stepsize, double momentum,
                    double* ratio_out_host, void* stream) {
    if (!h || !gsum || P < 1) return NICNES_ERR_INVALID;
    return opt_step(h, 1, gsum, P, l2coeff, nullptr, 0, stepsize, momentum, 0.0, 0.0, ratio_out_host, stream);
}

int nicnes_optimizer_update(nicnes_handle* h, int kind, const double* globalg, int globalg_fp32, double stepsize,
                            double beta1, double beta2, double epsilon, double* ratio_out_host, void* stream) {
    if (!h || !globalg || (kind != 0 && kind != 1)) return NICNES_ERR_INVALID;
    return opt_step(h, kind, nullptr, 0, 0.0, globalg, globalg_fp32, stepsize, beta1, beta2, epsilon, ratio_out_host, stream);
}

int nicnes_stats(nicnes_handle* h, int64_t* out8_host) {
    if (!h || !out8_host) return NICNES_ERR_INVALID;
    int32_t st[4];
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipMemcpy(st, h->stats, sizeof st, hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) out8_host[i] = st[i];
    // the step queue: tasks run and timeouts (over the handle's life), then the state the last queue launch left: member
    // slabs finished, tasks still in the ring
    uint32_t q[QUEUE_CTL_WORDS] = {0};
    if (h->queue_ctl) HIPC(h, hipMemcpy(q, h->queue_ctl, sizeof q, hipMemcpyDeviceToHost));
    out8_host[4] = q[QUEUE_STEPS];
    out8_host[5] = q[QUEUE_TIMEOUTS];
    out8_host[6] = q[QUEUE_DONE];
    out8_host[7] = (int64_t)(int32_t)(q[QUEUE_HEAD] + q[QUEUE_GRID] - q[QUEUE_TAIL]);   // (each worker ends on an unfilled ticket)
    return NICNES_OK;
}

int nicnes_set_decode_queue(nicnes_handle* h, int32_t mode, int32_t workers) {
    if (!h || mode < 0 || mode > 2 || workers < 0) return NICNES_ERR_INVALID;
    h->queue_mode = mode;
    h->queue_workers = workers;
    return NICNES_OK;
}

int nicnes_decode_queue_plan(int32_t mode, int32_t workers, int32_t n_cu, int32_t members, int32_t slabs,
                             int32_t* out3_host) {
    if (!out3_host || n_cu < 1 || members < 1 || slabs < 1 || mode > 2 || workers < 0) return NICNES_ERR_INVALID;
    int m = mode < 0 ? 2 : mode, w = workers;
    if (mode < 0) queue_env(&m, &w);
    if (w < 1) w = n_cu;
    const int64_t items = (int64_t)members * slabs;
    out3_host[0] = nicnes_queue_use(m, items, w) ? 1 : 0;
    out3_host[1] = (int32_t)std::min<int64_t>(items, w);
    out3_host[2] = nicnes_queue_ring_slots(items);
    return NICNES_OK;
}

int nicnes_screen_stats(nicnes_handle* h, int64_t* out2_host) {
    if (!h || !out2_host) return NICNES_ERR_INVALID;
    unsigned long long st[2] = {0, 0};
    HIPC(h, hipSetDevice(h->device));
    if (h->screen_ctr) HIPC(h, hipMemcpy(st, h->screen_ctr, sizeof st, hipMemcpyDeviceToHost));
    out2_host[0] = (int64_t)st[0];
    out2_host[1] = (int64_t)st[1];
    return NICNES_OK;
}

int nicnes_screen_reasons(nicnes_handle* h, int64_t* out16_host) {
    if (!h || !out16_host) return NICNES_ERR_INVALID;
    unsigned long long st[SCREEN_CTR_WORDS] = {0};
    HIPC(h, hipSetDevice(h->device));
    if (h->screen_ctr) HIPC(h, hipMemcpy(st, h->screen_ctr, sizeof st, hipMemcpyDeviceToHost));
    for (int i = 2; i < SCREEN_CTR_WORDS; ++i) out16_host[i - 2] = (int64_t)st[i];
    return NICNES_OK;
}

int nicnes_set_decode_screen(nicnes_handle* h, int32_t mode) {
    if (!h || mode < 0 || mode > 2) return NICNES_ERR_INVALID;
    HIPC(h, hipSetDevice(h->device));
    h->screen_mode = mode;
    ensure_screen(h);
    return NICNES_OK;
}

int nicnes_set_timing(nicnes_handle* h, int on) {
    if (!h) return NICNES_ERR_INVALID;
    HIPC(h, hipSetDevice(h->device));
    if (on && !h->ev[0])
    {
        for (auto& e : h->ev) HIPC(h, hipEventCreate(&e));
        for (auto& e : h->dev) HIPC(h, hipEventCreate(&e));
    }
    h->timing = on != 0;
    return NICNES_OK;
}

int nicnes_kernel_times(nicnes_handle* h, float* out2_host) {
    if (!h || !out2_host || !h->ev[0]) return NICNES_ERR_INVALID;
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipEventSynchronize(h->ev[2]));
    HIPC(h, hipEventElapsedTime(&out2_host[0], h->ev[0], h->ev[1]));
    HIPC(h, hipEventElapsedTime(&out2_host[1], h->ev[1], h->ev[2]));
    return NICNES_OK;
}

int nicnes_decode_phase_times(nicnes_handle* h, float* out8_host) {
    if (!h || !out8_host) return NICNES_ERR_INVALID;
    if (h->timing && h->n_dev == 0 && h->multi_stream) {      // multi-stream decode: no per-launch events
        for (int i = 0; i < 8; ++i) out8_host[i] = 0.f;
        return NICNES_OK;
    }
    if (h->n_dev < 2) return NICNES_ERR_INVALID;
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipEventSynchronize(h->dev[h->n_dev - 1]));
    // event k follows launch k. Fused: img, then steps (one launch), or step(t) for t = -1..T (the first
    // two launches run only a cell). Split: img, cell(-1), cell(0), then logit(t), cell(t) for t = 1..T.
    float o[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ms = 0.f;
    int n_cell_only = 0;
    for (int k = 1; k < h->n_dev; ++k) {
        HIPC(h, hipEventElapsedTime(&ms, h->dev[k - 1], h->dev[k]));
        switch (h->dev_kind[k]) {
            case DK_IMG: o[0] += ms; break;
            case DK_STEP:
                o[2] += ms; o[3] += 1;
                if (n_cell_only < 2) { o[1] += ms; ++n_cell_only; }
                break;
            case DK_STEPS: o[2] += ms; o[3] += 1; break;      // every step in one launch
            case DK_COOP: o[2] += ms; o[3] += 1; break;       // the split shape, every step in one launch
            case DK_STEPS2: o[2] += ms; o[3] += 1; break;     // 64-row slabs, every step in one launch
            case DK_LOGIT: o[4] += ms; o[5] += 1; break;
            default:
                o[6] += ms; o[7] += 1;
                if (n_cell_only < 2) { o[1] += ms; ++n_cell_only; }
                break;
        }
    }
    for (int i = 0; i < 8; ++i) out8_host[i] = o[i];
    return NICNES_OK;
}

int nicnes_set_decode_streams(nicnes_handle* h, int32_t n) {
    if (!h || n < 0 || n > 4) return NICNES_ERR_INVALID;
    if (h->wide && n > 1)
        return fail(h, NICNES_ERR_UNSUPPORTED, wide_what(h) + "the decode runs on "
                                               "one stream, more are not supported");
    h->dec_streams = n;
    return NICNES_OK;
}

int nicnes_set_decode_coop(nicnes_handle* h, int32_t mode) {
    if (!h || (mode != 0 && mode != 1)) return NICNES_ERR_INVALID;
    h->coop_mode = mode;
    return NICNES_OK;
}

int nicnes_last_decode_lse(nicnes_handle* h, int32_t* bounded_host) {
    if (!h || !bounded_host) return NICNES_ERR_INVALID;
    *bounded_host = h->last_decode_bounded;
    return NICNES_OK;
}

int nicnes_test_logit_chain(nicnes_handle* h, uint64_t iteration, int32_t member, float sigma, int32_t sign,
                            const float* h_rows, float* out_mfma, float* out_chain, void* stream) {
    if (!h || !h_rows || !out_mfma || !out_chain || member < 0 || (sign != 0 && sign != 1)) return NICNES_ERR_INVALID;
    if (!h->noise) return fail(h, NICNES_ERR_INVALID, "nicnes_set_noise_table first");
    if (!h->theta_set) return fail(h, NICNES_ERR_INVALID, "nicnes_set_theta first");
    if (h->mut_mode) return fail(h, NICNES_ERR_UNSUPPORTED, "nicnes_test_logit_chain: plain mutations only");
    if (h->wide)
        return fail(h, NICNES_ERR_UNSUPPORTED, wide_what(h) +
                                               "nicnes_test_logit_chain takes a 128-wide h: not supported");
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    if (int rc = ensure_noise_scaled(h, sigma, s)) return rc;
    DecodeParams p = decode_base(h);
    p.theta = h->theta32;
    p.noise = h->noise_sc;
    p.scratch = h->dscratch;        // one wave's lane scratch holds the rows of h (no decode runs beside this)
    const uint64_t nidx = nn_noise_index(h->cfg.noise_seed, iteration, (uint64_t)member, h->cfg.noise_len, (uint64_t)h->D);
    HIPC(h, nicnes_launch_test_logit_chain(&p, nidx, sign, h_rows, out_mfma, out_chain, s));
    return NICNES_OK;
}

int nicnes_test_ln_cell(nicnes_handle* h, const float* x_dev, const float* h_dev, const float* c_dev, int32_t rows,
                        float* h_out, float* c_out, void* stream) {
    if (!h || !x_dev || !h_dev || !c_dev || !h_out || !c_out || rows < 1 || rows > 128) return NICNES_ERR_INVALID;
    if (!h->ln) return fail(h, NICNES_ERR_UNSUPPORTED, "nicnes_test_ln_cell: the handle has no layer_n");
    if (!h->theta_set) return fail(h, NICNES_ERR_INVALID, "nicnes_set_theta first");
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    if (int rc = ensure_zero_noise(h)) return rc;
    DecodeParams p = decode_base(h);
    p.theta = h->theta32;
    p.noise = h->zero_noise;        // theta itself
    p.scratch = h->dscratch;        // one workgroup's lane scratch (no decode runs beside this)
    HIPC(h, nicnes_launch_test_ln_cell(&p, h->cfg.input_encoding_size, h->cfg.rnn_size,
                                       h->ln_affine ? h->ln_off : nullptr, x_dev, h_dev, c_dev, rows, h_out, c_out, s));
    return NICNES_OK;
}

int nicnes_test_certify_items(nicnes_handle* h, uint64_t iteration, int32_t member, float sigma, int32_t sign,
                              const float* h_rows, const int32_t* items_host, int32_t n_items, float* out, void* stream) {
    return nicnes_test_certify_items_owned(h, iteration, member, sigma, sign, 0, h_rows, items_host, n_items, out, stream);
}

int nicnes_test_certify_items_owned(nicnes_handle* h, uint64_t iteration, int32_t member, float sigma, int32_t sign,
                                    int32_t owner_by_id, const float* h_rows, const int32_t* items_host, int32_t n_items,
                                    float* out, void* stream) {
    if (!h || !h_rows || n_items < 0 || (n_items && (!items_host || !out)) || member < 0 || (sign != 0 && sign != 1) ||
        (owner_by_id != 0 && owner_by_id != 1))
        return NICNES_ERR_INVALID;
    if (!h->noise) return fail(h, NICNES_ERR_INVALID, "nicnes_set_noise_table first");
    if (!h->theta_set) return fail(h, NICNES_ERR_INVALID, "nicnes_set_theta first");
    if (h->mut_mode) return fail(h, NICNES_ERR_UNSUPPORTED, "nicnes_test_certify_items: plain mutations only");
    if (h->wide)
        return fail(h, NICNES_ERR_UNSUPPORTED, wide_what(h) +
                                               "nicnes_test_certify_items takes a 128-wide h: not supported");
    for (int32_t i = 0; i < n_items; ++i) {
        const int32_t row = items_host[2 * i], id = items_host[2 * i + 1];
        if (row < 0 || row >= 128) return fail(h, NICNES_ERR_INVALID, "nicnes_test_certify_items: row outside [0, 128)");
        if (id < 0 || id >= h->V1) return fail(h, NICNES_ERR_INVALID, "nicnes_test_certify_items: id outside [0, vocab_size]");
    }
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    if (int rc = ensure_noise_scaled(h, sigma, s)) return rc;
    // the items grouped by owner lane (group 2 row + half; half 0, or the id's bit 2 as the decode's lists have it):
    // lane_start [257] | ids [n] | positions [n]. Inside a group the caller's order, or increasing ids (by id: the order
    // a decode's lane meets them in; repeats keep the caller's order)
    std::vector<int32_t> host(257 + 2 * (size_t)n_items, 0);
    int32_t* lane_start = host.data();
    int32_t* ids = lane_start + 257;
    int32_t* pos_of = ids + n_items;
    auto group = [&](int32_t i) { return 2 * items_host[2 * i] + (owner_by_id ? (items_host[2 * i + 1] >> 2) & 1 : 0); };
    std::vector<int32_t> order((size_t)n_items);
    for (int32_t i = 0; i < n_items; ++i) order[i] = i;
    if (owner_by_id)
        std::stable_sort(order.begin(), order.end(),
                         [&](int32_t a, int32_t b) { return items_host[2 * a + 1] < items_host[2 * b + 1]; });
    for (int32_t i = 0; i < n_items; ++i) ++lane_start[group(i) + 1];
    for (int g = 0; g < 256; ++g) lane_start[g + 1] += lane_start[g];
    std::vector<int32_t> fill(lane_start, lane_start + 256);
    for (int32_t i : order) {
        const int32_t at = fill[group(i)]++;
        ids[at] = items_host[2 * i + 1];
        pos_of[at] = i;
    }
    int32_t* dev = nullptr;
    HIPC(h, hipMalloc((void**)&dev, host.size() * sizeof(int32_t)));
    hipError_t e = hipMemcpyAsync(dev, host.data(), host.size() * sizeof(int32_t), hipMemcpyHostToDevice, s);
    DecodeParams p = decode_base(h);
    p.theta = h->theta32;
    p.noise = h->noise_sc;
    p.scratch = h->dscratch;        // eight waves' lane scratch hold the rows of h (no decode runs beside this)
    const uint64_t nidx = nn_noise_index(h->cfg.noise_seed, iteration, (uint64_t)member, h->cfg.noise_len, (uint64_t)h->D);
    if (e == hipSuccess)
        e = nicnes_launch_test_certify_items(&p, nidx, sign, h_rows, dev, dev + 257, dev + 257 + n_items, out, s);
    const hipError_t e2 = hipStreamSynchronize(s);    // host and dev live until the kernel has read them
    (void)hipFree(dev);
    HIPC(h, e);
    HIPC(h, e2);
    return NICNES_OK;
}

int nicnes_test_score_rows(nicnes_handle* h, const int32_t* seq, int32_t n_cand, int32_t rows,
                           const int32_t* member_batch_host, const float* lp, const double* base, double* scores_out,
                           double* fitness_out, void* stream) {
    if (!h || !seq || !scores_out || !fitness_out) return NICNES_ERR_INVALID;
    if (!h->batch_set) return fail(h, NICNES_ERR_INVALID, "nicnes_set_batch first");
    if (h->fitness_mode == NICNES_FITNESS_XENT)
        return fail(h, NICNES_ERR_UNSUPPORTED, "nicnes_test_score_rows: the xent fitness scores no token rows");
    const int rpi = h->fitness_mode >= NICNES_FITNESS_SAMPLE ? h->rpi : 1;
    if (rows != h->B * rpi) return fail(h, NICNES_ERR_INVALID, "rows must be B * rows_per_image (B in the greedy modes)");
    // h->row_scores holds [2 * max_members, rows] and h->mbatch [max_members] (the evaluate's 2 * count candidates)
    if (n_cand < 1 || n_cand > 2 * h->cfg.max_members)
        return fail(h, NICNES_ERR_INVALID, "n_cand out of [1, 2 * max_members]");
    if (member_batch_host && (n_cand & 1))
        return fail(h, NICNES_ERR_INVALID, "member_batch maps members: n_cand must be even (two candidates each)");
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    if (int rc = ensure_rows(h, rows)) return rc;
    const int32_t* mb = nullptr;
    if (int rc = stage_member_batch(h, member_batch_host, n_cand / 2, s, &mb)) return rc;
    return score_rollouts(h, seq, lp, n_cand, rows, rpi, mb, base, fitness_out, scores_out, s);
}

int nicnes_decode_path(nicnes_handle* h, int32_t B, int32_t count, int32_t* out_host) {
    if (!h || !out_host || B < 1 || count < 1) return NICNES_ERR_INVALID;
    int G = 0, nslabs = 0, S = 0;
    decode_shape(h, B, count, &G, &nslabs, &S);
    *out_host = h->ln ? 4 : h->wide ? 3 : S == 1 ? 0 : coop_fits(h, G, nslabs, S, count) ? 2 : 1;
    return NICNES_OK;
}

int nicnes_set_decode_split(nicnes_handle* h, int32_t S, int32_t G) {
    if (!h || S < 0 || S > 64 || (G != 0 && G != 2 && G != 4)) return NICNES_ERR_INVALID;
    if (h->wide && (S > 1 || G == 2))
        return fail(h, NICNES_ERR_UNSUPPORTED, wide_what(h) + "one workgroup per "
                                               "member and 128-row slab, a forced split shape is not supported");
    HIPC(h, hipSetDevice(h->device));
    if (S > 0) {
        const int ns = std::max(nslabs_of(h->cfg.max_batch, 2), nslabs_of(h->cfg.max_batch, 4));
        const int64_t need = (int64_t)h->cfg.max_members * ns * S;
        if (need > h->part_cap) {
            float* np = nullptr;
            int rc = dalloc(h, &np, (size_t)need * PART_FLOATS);
            if (rc) return rc;
            HIPC(h, hipDeviceSynchronize());
            (void)hipFree(h->part);
            h->part = np;
            h->part_cap = need;
        }
    }
    h->dec_S = S;
    h->dec_G = G;
    return NICNES_OK;
}

// ---- multi-GPU exchange over RCCL (the data plane of SURVEY.md 8(e)) ---------------------------
#define NCCLC(h, expr)                                                                          \
    do {                                                                                        \
        ncclResult_t r_ = (expr);                                                               \
        if (r_ != ncclSuccess)                                                                  \
            return fail((h), NICNES_ERR_HIP, std::string(#expr) + ": " + ncclGetErrorString(r_)); \
    } while (0)

int nicnes_comm_unique_id(uint8_t* id_out_host) {
    if (!id_out_host) return NICNES_ERR_INVALID;
    static_assert(sizeof(ncclUniqueId) == NICNES_COMM_ID_BYTES, "RCCL unique id size");
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return NICNES_ERR_HIP;
    std::memcpy(id_out_host, &id, sizeof id);
    return NICNES_OK;
}

int nicnes_comm_init(nicnes_handle* h, int32_t nranks, int32_t rank, const uint8_t* id_host) {
    if (!h || !id_host || nranks < 1 || rank < 0 || rank >= nranks) return NICNES_ERR_INVALID;
    if (h->comm) return fail(h, NICNES_ERR_INVALID, "a communicator is already bound (nicnes_comm_destroy first)");
    HIPC(h, hipSetDevice(h->device));
    ncclUniqueId id;
    std::memcpy(&id, id_host, sizeof id);
    ncclComm_t c = nullptr;
    NCCLC(h, ncclCommInitRank(&c, nranks, id, rank));
    h->comm = c;
    h->comm_owned = true;
    h->comm_nranks = nranks;
    return NICNES_OK;
}

int nicnes_comm_attach(nicnes_handle* h, void* nccl_comm) {
    if (!h || !nccl_comm) return NICNES_ERR_INVALID;
    if (h->comm) return fail(h, NICNES_ERR_INVALID, "a communicator is already bound (nicnes_comm_destroy first)");
    int n = 0;
    NCCLC(h, ncclCommCount((ncclComm_t)nccl_comm, &n));
    h->comm = (ncclComm_t)nccl_comm;
    h->comm_owned = false;
    h->comm_nranks = n;
    return NICNES_OK;
}

int nicnes_comm_destroy(nicnes_handle* h) {
    if (!h) return NICNES_ERR_INVALID;
    if (h->comm && h->comm_owned) NCCLC(h, ncclCommDestroy(h->comm));
    h->comm = nullptr;
    h->comm_owned = false;
    h->comm_nranks = 1;
    return NICNES_OK;
}

int nicnes_comm_count(nicnes_handle* h, int32_t* nranks_out_host, int32_t* rank_out_host) {
    if (!h || !nranks_out_host || !rank_out_host) return NICNES_ERR_INVALID;
    int n = 1, r = 0;
    if (h->comm) {
        NCCLC(h, ncclCommCount(h->comm, &n));
        NCCLC(h, ncclCommUserRank(h->comm, &r));
    }
    *nranks_out_host = n;
    *rank_out_host = r;
    return NICNES_OK;
}

int nicnes_allgather_fitness(nicnes_handle* h, const double* fit_local, int32_t P_local, double* fit_all, void* stream) {
    if (!h || !fit_local || !fit_all || P_local < 1) return NICNES_ERR_INVALID;
    if (!h->comm) return fail(h, NICNES_ERR_INVALID, "no communicator (nicnes_comm_init / nicnes_comm_attach)");
    HIPC(h, hipSetDevice(h->device));
    NCCLC(h, ncclAllGather(fit_local, fit_all, (size_t)P_local * 2, ncclDouble, h->comm, (hipStream_t)stream));
    return NICNES_OK;
}

int nicnes_allreduce_grad(nicnes_handle* h, float* gsum, void* stream) {
    if (!h || !gsum) return NICNES_ERR_INVALID;
    if (!h->comm) return fail(h, NICNES_ERR_INVALID, "no communicator (nicnes_comm_init / nicnes_comm_attach)");
    HIPC(h, hipSetDevice(h->device));
    NCCLC(h, ncclAllReduce(gsum, gsum, (size_t)h->D, ncclFloat, ncclSum, h->comm, (hipStream_t)stream));
    return NICNES_OK;
}

int nicnes_decode_shape(nicnes_handle* h, int32_t B, int32_t count, int32_t* out3_host) {
    if (!h || !out3_host || B < 1 || count < 1) return NICNES_ERR_INVALID;
    int G, ns, S;
    decode_shape(h, B, count, &G, &ns, &S);
    out3_host[0] = G;
    out3_host[1] = ns;
    out3_host[2] = S;
    return NICNES_OK;
}

// ---- nic_es (src/algorithm/nic_es/) -------------------------------------------------------------------------------
// A caller's host int32 array checked against [0, bound) and copied to dst on s through the pinned ring of
// stage_member_batch (no wait for queued GPU work).
static int es_stage_i32(nicnes_handle* h, const int32_t* host, int count, int32_t bound, int32_t* dst, hipStream_t s,
                        const char* what) {
    for (int k = 0; k < count; ++k)
        if (host[k] < 0 || host[k] >= bound) return fail(h, NICNES_ERR_INVALID, std::string(what) + " entry out of range");
    const int slot = h->mb_next;
    h->mb_next = (slot + 1) % MB_RING;
    if (h->mb_used[slot]) HIPC(h, hipEventSynchronize(h->mb_ev[slot]));
    std::memcpy(h->mb_pin[slot], host, (size_t)count * sizeof(int32_t));
    HIPC(h, hipMemcpyAsync(dst, h->mb_pin[slot], (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPC(h, hipEventRecord(h->mb_ev[slot], s));
    h->mb_used[slot] = true;
    return NICNES_OK;
}

int nicnes_es_free(nicnes_handle* h) {
    if (!h) return NICNES_ERR_INVALID;
    nicnes_es* es = h->es;
    if (!es) return NICNES_OK;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    void* bufs[] = {es->ptab[0], es->ptab[1], es->etab, es->pmean[0], es->pmean[1], es->pzero[0], es->pzero[1], es->emean,
                    es->ezero, es->part_sum, es->part_zero, es->parent_of, es->neg, es->dbuf, es->didx, es->gat, es->stab,
                    es->svec};
    for (void* q : bufs)
        if (q) (void)hipFree(q);
    delete es;
    h->es = nullptr;
    return NICNES_OK;
}

int nicnes_es_create(nicnes_handle* h, int32_t max_parents, int32_t max_elites) {
    if (!h || max_parents < 1 || max_elites < 1 || max_elites > max_parents) return NICNES_ERR_INVALID;
    if (h->wide)
        return fail(h, NICNES_ERR_UNSUPPORTED, wide_what(h) + "nic_es is not "
                                               "supported");
    if (h->es) return fail(h, NICNES_ERR_INVALID, "nicnes_es_create: the handle has an ES state (nicnes_es_free first)");
    HIPC(h, hipSetDevice(h->device));
    nicnes_es* es = new nicnes_es();
    h->es = es;
    es->max_parents = max_parents;
    es->max_elites = max_elites;
    es->Dp = (h->D + 63) / 64 * 64;
    es->sens_valid.assign((size_t)max_parents, 0);
    const size_t MP = (size_t)max_parents, ME = (size_t)max_elites, MM = (size_t)h->cfg.max_members;
    int rc = NICNES_OK;
    for (int t = 0; t < 2 && !rc; ++t) {
        rc = dalloc(h, &es->ptab[t], MP * (size_t)es->Dp);
        if (!rc) rc = dalloc(h, &es->pmean[t], MP);
        if (!rc) rc = dalloc(h, &es->pzero[t], MP);
    }
    if (!rc) rc = dalloc(h, &es->etab, ME * (size_t)es->Dp);
    if (!rc) rc = dalloc(h, &es->emean, ME);
    if (!rc) rc = dalloc(h, &es->ezero, ME);
    if (!rc) rc = dalloc(h, &es->part_sum, nicnes_es_stats_scratch(max_parents));
    if (!rc) rc = dalloc(h, &es->part_zero, nicnes_es_stats_scratch(max_parents));
    if (!rc) rc = dalloc(h, &es->parent_of, MM);
    if (!rc) rc = dalloc(h, &es->neg, 2 * MM);
    if (rc) {
        (void)nicnes_es_free(h);
        return rc;
    }
    // rows no one has set read as zeros (the pad columns D .. Dp are never read)
    for (int t = 0; t < 2; ++t) {
        HIPC(h, hipMemset(es->ptab[t], 0, MP * (size_t)es->Dp * sizeof(float)));
        HIPC(h, hipMemset(es->pmean[t], 0, MP * sizeof(float)));
        HIPC(h, hipMemset(es->pzero[t], 0, MP * sizeof(int64_t)));
    }
    HIPC(h, hipMemset(es->etab, 0, ME * (size_t)es->Dp * sizeof(float)));
    HIPC(h, hipMemset(es->emean, 0, ME * sizeof(float)));
    HIPC(h, hipMemset(es->ezero, 0, ME * sizeof(int64_t)));
    HIPC(h, hipDeviceSynchronize());
    return NICNES_OK;
}

#define ES_STATE(h)                                                                  \
    if (!(h)) return NICNES_ERR_INVALID;                                             \
    nicnes_es* es = (h)->es;                                                         \
    if (!es) return fail((h), NICNES_ERR_INVALID, "nicnes_es_create first")

int nicnes_es_set_mutation(nicnes_handle* h, int32_t mode) {
    ES_STATE(h);
    if (mode != NICNES_MUTATION_PLAIN && mode != NICNES_MUTATION_SCALE)
        return fail(h, NICNES_ERR_UNSUPPORTED,
                    "nic_es mutation: this entry sets plain and SM-PROPORTIONAL (the divide of SM-G-SUM / SM-VECTOR, which "
                    "needs the parents' sensitivities: nicnes_set_mutation_divide_es)");
    es->mode = mode;
    return NICNES_OK;
}

int nicnes_set_mutation_divide_es(nicnes_handle* h) {
    ES_STATE(h);
    es->mode = NICNES_MUTATION_DIVIDE;
    return NICNES_OK;
}

int nicnes_es_set_parent(nicnes_handle* h, int32_t slot, const float* theta32, void* stream) {
    ES_STATE(h);
    if (!theta32 || slot < 0 || slot >= es->max_parents) return fail(h, NICNES_ERR_INVALID, "parent slot out of range");
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    float* row = es->ptab[es->cur] + (size_t)slot * (size_t)es->Dp;
    es->sens_valid[(size_t)slot] = 0;  // the slot's sensitivity row was another theta's
    HIPC(h, hipMemcpyAsync(row, theta32, (size_t)h->D * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPC(h, nicnes_launch_es_parent_stats(row, 1, es->Dp, h->D, es->part_sum, es->part_zero, es->pmean[es->cur] + slot,
                                          es->pzero[es->cur] + slot, s));
    return NICNES_OK;
}

int nicnes_es_set_parent_count(nicnes_handle* h, int32_t count) {
    ES_STATE(h);
    if (count < 1 || count > es->max_parents) return fail(h, NICNES_ERR_INVALID, "parent count out of [1, max_parents]");
    es->n_parents = count;
    return NICNES_OK;
}

// ---- the parents' sensitivities (NICNES_MUTATION_DIVIDE: SM-G-SUM, SM-VECTOR) ----
// The table [max_parents, Dp], allocated at the first use (synchronising then), the pad columns written 1.0 once.
static int es_sens_table(nicnes_handle* h, nicnes_es* es, hipStream_t s) {
    if (es->stab) return NICNES_OK;
    HIPC(h, hipDeviceSynchronize());
    if (int rc = dalloc(h, &es->stab, (size_t)es->max_parents * (size_t)es->Dp)) return rc;
    HIPC(h, nicnes_launch_es_sens_pad(es->stab, es->max_parents, es->Dp, h->D, s));
    return NICNES_OK;
}

// DIVIDE needs a sensitivity for every parent a call names: the shared vector, or a valid row per slot. Checked on the
// host before anything is enqueued (n slots, each also checked against the parent count).
static int es_sens_ready(nicnes_handle* h, const nicnes_es* es, const int32_t* slots, int n) {
    if (es->mode != NICNES_MUTATION_DIVIDE || es->sens_shared) return NICNES_OK;
    for (int k = 0; k < n; ++k) {
        const int32_t p = slots[k];
        if (p < 0 || p >= es->n_parents) return fail(h, NICNES_ERR_INVALID, "parent_of entry out of range");
        if (!es->stab || !es->sens_valid[(size_t)p])
            return fail(h, NICNES_ERR_INVALID, "divide mutation: parent " + std::to_string(p) +
                                                   " has no valid sensitivity (nicnes_sensitivity_es / "
                                                   "nicnes_set_sensitivity_es after the parents were written)");
    }
    return NICNES_OK;
}

int nicnes_sensitivity_es(nicnes_handle* h, const int32_t* slots_host, int32_t n_slots, int32_t rows, float underflow,
                          void* stream) {
    ES_STATE(h);
    if (!slots_host || n_slots < 1) return NICNES_ERR_INVALID;
    if (!h->batch_set) return fail(h, NICNES_ERR_INVALID, "nicnes_set_batch first");
    if (rows < 1 || rows > h->B) return fail(h, NICNES_ERR_INVALID, "rows out of [1, B] of the batch held");
    if (int rc = sens_rows_fit(h, rows)) return rc;
    if (!(underflow > 0.f)) return fail(h, NICNES_ERR_INVALID, "underflow must be > 0 (calc_sensitivity divides by it)");
    for (int k = 0; k < n_slots; ++k)
        if (slots_host[k] < 0 || slots_host[k] >= es->n_parents)
            return fail(h, NICNES_ERR_INVALID, "sensitivity slot outside [0, parent count)");
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    if (int rc = es_sens_table(h, es, s)) return rc;
    es->sens_shared = false;
    for (int k = 0; k < n_slots; ++k) {            // one parent after the other on the caller's stream
        const size_t at = (size_t)slots_host[k] * (size_t)es->Dp;
        es->sens_valid[(size_t)slots_host[k]] = 0;
        if (int rc = sens_of_theta(h, es->ptab[es->cur] + at, rows, underflow, es->stab + at, s)) return rc;
        es->sens_valid[(size_t)slots_host[k]] = 1;
    }
    return NICNES_OK;
}

int nicnes_set_sensitivity_es(nicnes_handle* h, int32_t slot, const float* vec_dev, void* stream) {
    ES_STATE(h);
    if (!vec_dev || slot < -1 || slot >= es->max_parents)
        return fail(h, NICNES_ERR_INVALID, "sensitivity slot out of range (-1: the shared vector)");
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    if (slot < 0) {                    // one vector for every parent: the kernels read it with row stride 0
        if (!es->svec) {
            HIPC(h, hipDeviceSynchronize());
            if (int rc = dalloc(h, &es->svec, (size_t)es->Dp)) return rc;
            HIPC(h, nicnes_launch_es_sens_pad(es->svec, 1, es->Dp, h->D, s));
        }
        HIPC(h, hipMemcpyAsync(es->svec, vec_dev, (size_t)h->D * sizeof(float), hipMemcpyDeviceToDevice, s));
        es->sens_shared = true;
        return NICNES_OK;
    }
    if (int rc = es_sens_table(h, es, s)) return rc;
    HIPC(h, hipMemcpyAsync(es->stab + (size_t)slot * (size_t)es->Dp, vec_dev, (size_t)h->D * sizeof(float),
                           hipMemcpyDeviceToDevice, s));
    es->sens_shared = false;
    es->sens_valid[(size_t)slot] = 1;
    return NICNES_OK;
}

int nicnes_get_sensitivity_es(nicnes_handle* h, int32_t slot, float* out_dev, void* stream) {
    ES_STATE(h);
    if (!out_dev || slot < 0 || slot >= es->max_parents) return fail(h, NICNES_ERR_INVALID, "sensitivity slot out of range");
    const float* row = nullptr;
    if (es->sens_shared)
        row = es->svec;
    else if (es->stab && es->sens_valid[(size_t)slot])
        row = es->stab + (size_t)slot * (size_t)es->Dp;
    if (!row) return fail(h, NICNES_ERR_INVALID, "the slot has no valid sensitivity");
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipMemcpyAsync(out_dev, row, (size_t)h->D * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return NICNES_OK;
}

// a row of table 0 (current parents) or 1 (elites), with its statistics
static int es_row(nicnes_handle* h, nicnes_es* es, int table, int slot, float** row, float** mean, int64_t** zeros) {
    if (table == 0 && slot >= 0 && slot < es->max_parents) {
        *row = es->ptab[es->cur] + (size_t)slot * (size_t)es->Dp;
        *mean = es->pmean[es->cur] + slot;
        *zeros = es->pzero[es->cur] + slot;
        return NICNES_OK;
    }
    if (table == 1 && slot >= 0 && slot < es->max_elites) {
        *row = es->etab + (size_t)slot * (size_t)es->Dp;
        *mean = es->emean + slot;
        *zeros = es->ezero + slot;
        return NICNES_OK;
    }
    return fail(h, NICNES_ERR_INVALID, "table (0 parents, 1 elites) or slot out of range");
}

int nicnes_es_get_row(nicnes_handle* h, int32_t table, int32_t slot, float* theta32_out, void* stream) {
    ES_STATE(h);
    if (!theta32_out) return NICNES_ERR_INVALID;
    float *row, *mean;
    int64_t* zeros;
    if (int rc = es_row(h, es, table, slot, &row, &mean, &zeros)) return rc;
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipMemcpyAsync(theta32_out, row, (size_t)h->D * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return NICNES_OK;
}

int nicnes_es_row_stats(nicnes_handle* h, int32_t table, int32_t slot, float* mean_abs_out_host, int64_t* zeros_out_host,
                        void* stream) {
    ES_STATE(h);
    float *row, *mean;
    int64_t* zeros;
    if (int rc = es_row(h, es, table, slot, &row, &mean, &zeros)) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    if (mean_abs_out_host) HIPC(h, hipMemcpyAsync(mean_abs_out_host, mean, sizeof(float), hipMemcpyDeviceToHost, s));
    if (zeros_out_host) HIPC(h, hipMemcpyAsync(zeros_out_host, zeros, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPC(h, hipStreamSynchronize(s));
    return NICNES_OK;
}

int nicnes_es_set_elite(nicnes_handle* h, int32_t elite_slot, int32_t table, int32_t slot, void* stream) {
    ES_STATE(h);
    if (elite_slot < 0 || elite_slot >= es->max_elites) return fail(h, NICNES_ERR_INVALID, "elite slot out of range");
    float *row, *mean;
    int64_t* zeros;
    if (int rc = es_row(h, es, table, slot, &row, &mean, &zeros)) return rc;
    if (table == 1 && slot == elite_slot) return NICNES_OK;
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipMemcpyAsync(es->etab + (size_t)elite_slot * (size_t)es->Dp, row, (size_t)h->D * sizeof(float),
                           hipMemcpyDeviceToDevice, s));
    HIPC(h, hipMemcpyAsync(es->emean + elite_slot, mean, sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPC(h, hipMemcpyAsync(es->ezero + elite_slot, zeros, sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    return NICNES_OK;
}

int nicnes_es_load_theta(nicnes_handle* h, int32_t table, int32_t slot, void* stream) {
    ES_STATE(h);
    float *row, *mean;
    int64_t* zeros;
    if (int rc = es_row(h, es, table, slot, &row, &mean, &zeros)) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    HIPC(h, hipMemcpyAsync(h->theta32, row, (size_t)h->D * sizeof(float), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(f32_to_f64_kernel, dim3((unsigned)((h->D + 255) / 256)), dim3(256), 0, s, h->theta32, h->theta64,
                       h->D);
    HIPC(h, hipGetLastError());
    h->theta_is_fp32 = 1;
    h->step_pending_check = false;
    h->theta_set = true;
    return NICNES_OK;
}

// the arguments of the materialise kernel common to an advance and a single offspring
static EsMaterialise es_mat_args(const nicnes_handle* h, const nicnes_es* es, uint64_t generation, float sigma) {
    EsMaterialise a{};
    a.noise = h->noise;
    a.parents = es->ptab[es->cur];
    a.mean_abs = es->pmean[es->cur];
    a.elites = es->etab;
    a.sens = es->sens_shared ? es->svec : es->stab;
    a.sens_stride = es->sens_shared ? 0 : es->Dp;
    a.stride = es->Dp;
    a.dim = h->D;
    a.seed = h->cfg.noise_seed;
    a.generation = generation;
    a.table_len = h->cfg.noise_len;
    a.sigma = sigma;
    a.mode = es->mode;
    return a;
}

int nicnes_es_offspring(nicnes_handle* h, uint64_t generation, int32_t pair, int32_t sign, float sigma, int32_t parent,
                        float* theta32_out, void* stream) {
    ES_STATE(h);
    if (!theta32_out || pair < 0 || (sign != 0 && sign != 1)) return NICNES_ERR_INVALID;
    if (parent < 0 || parent >= es->n_parents) return fail(h, NICNES_ERR_INVALID, "parent outside [0, parent count)");
    if (!h->noise) return fail(h, NICNES_ERR_INVALID, "nicnes_set_noise_table first");
    if (int rc = es_sens_ready(h, es, &parent, 1)) return rc;
    HIPC(h, hipSetDevice(h->device));
    EsMaterialise a = es_mat_args(h, es, generation, sigma);
    a.out = theta32_out;
    a.pair0 = pair;
    a.sign0 = sign;
    a.parent0 = parent;
    HIPC(h, nicnes_launch_es_materialise(&a, 1, (hipStream_t)stream));
    return NICNES_OK;
}

int nicnes_es_select(nicnes_handle* h, const double* fitness, int32_t n, int32_t n_keep, int32_t* order_out,
                     void* stream) {
    ES_STATE(h);
    if (!fitness || !order_out) return NICNES_ERR_INVALID;
    if (n < 1 || n > 2 * h->cfg.max_members) return fail(h, NICNES_ERR_INVALID, "n out of [1, 2 max_members]");
    if (n_keep < 1 || n_keep > n) return fail(h, NICNES_ERR_INVALID, "n_keep out of [1, n]");
    HIPC(h, hipSetDevice(h->device));
    // (the rank scratch holds nicnes_rank_scratch_pairs(2 max_members) pairs from nicnes_create on)
    HIPC(h, nicnes_launch_es_select(fitness, n, n_keep, es->neg, h->rank_key, h->rank_idx, order_out, (hipStream_t)stream));
    return NICNES_OK;
}

int nicnes_es_advance(nicnes_handle* h, uint64_t generation, float sigma, const int32_t* parent_of_host, int32_t n_pairs,
                      const int32_t* order, int32_t n_keep, int32_t n_front, void* stream) {
    ES_STATE(h);
    if (!parent_of_host || !order) return NICNES_ERR_INVALID;
    if (n_pairs < 1 || n_pairs > h->cfg.max_members) return fail(h, NICNES_ERR_INVALID, "n_pairs out of [1, max_members]");
    if (n_keep < 1 || n_keep > 2 * n_pairs || n_front < 0 || n_front > es->max_elites ||
        n_front + n_keep > es->max_parents)
        return fail(h, NICNES_ERR_INVALID, "n_keep / n_front: out of range or beyond max_parents");
    if (!h->noise) return fail(h, NICNES_ERR_INVALID, "nicnes_set_noise_table first");
    // (every pair's parent: which of them the survivors name is known only on the device)
    if (int rc = es_sens_ready(h, es, parent_of_host, n_pairs)) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    if (int rc = es_stage_i32(h, parent_of_host, n_pairs, es->n_parents, es->parent_of, s, "parent_of")) return rc;
    const int nxt = 1 - es->cur, rows = n_front + n_keep;
    EsMaterialise a = es_mat_args(h, es, generation, sigma);
    a.parent_of = es->parent_of;
    a.order = order;
    a.out = es->ptab[nxt];
    a.n_front = n_front;
    a.n_pairs = n_pairs;
    HIPC(h, nicnes_launch_es_materialise(&a, rows, s));
    HIPC(h, nicnes_launch_es_parent_stats(es->ptab[nxt], rows, es->Dp, h->D, es->part_sum, es->part_zero, es->pmean[nxt],
                                          es->pzero[nxt], s));
    es->cur = nxt;
    es->n_parents = rows;
    std::fill(es->sens_valid.begin(), es->sens_valid.end(), 0);   // the rows were the old table's (a shared vector stays)
    return NICNES_OK;
}

// The path of an ES evaluate of `count` pairs of a B-image batch under nicnes_set_decode_es: *coop_S = 0 (fused) or the
// coop path's S. Mode 1 takes the coop path only where the handle's own shape rule picks 128-row slabs with S = 2 or 4
// and the grid fits (coop_fits, which nicnes_set_decode_coop(h, 0) turns off); it never takes the split path or 64-row
// slabs. Mode 2 fails, before anything is enqueued, when its grid cannot be resident at once.
static int es_decode_choice(nicnes_handle* h, int B, int count, int* coop_S) {
    *coop_S = 0;
    if (h->es_dec_mode == 0) return NICNES_OK;
    if (h->es_dec_mode == 1) {
        int G = 0, nslabs = 0, S = 0;
        decode_shape(h, B, count, &G, &nslabs, &S);
        if (G == 4 && (S == 2 || S == 4) && coop_fits(h, G, nslabs, S, count) &&
            (int64_t)count * nslabs * S <= h->part_cap)
            *coop_S = S;
        return NICNES_OK;
    }
    const int S = h->es_dec_S, nslabs = nslabs_of(B, 4);
    const int64_t wgs = (int64_t)count * nslabs * S, bound = (int64_t)h->coop_occ * h->n_cu;
    if (!h->coop_mode)
        return fail(h, NICNES_ERR_INVALID, "nic_es coop decode: the coop path is off (nicnes_set_decode_coop(h, 0))");
    if (wgs > bound)
        return fail(h, NICNES_ERR_INVALID,
                    "nic_es coop decode: count x slabs x S = " + std::to_string(wgs) +
                        " workgroups cannot be resident at once: the bound is occupancy x CUs = " + std::to_string(bound));
    if (!coop_fits(h, 4, nslabs, S, count))
        return fail(h, NICNES_ERR_INVALID, "nic_es coop decode: the vocabulary has fewer 64-row stages than S");
    if (wgs > h->part_cap)
        return fail(h, NICNES_ERR_INVALID, "nic_es coop decode: beyond the partial-state buffer (nicnes_set_decode_es)");
    *coop_S = S;
    return NICNES_OK;
}

int nicnes_set_decode_es(nicnes_handle* h, int32_t mode, int32_t S) {
    if (!h) return NICNES_ERR_INVALID;
    if (mode < 0 || mode > 2) return fail(h, NICNES_ERR_INVALID, "nicnes_set_decode_es: mode 0 fused, 1 automatic, 2 coop");
    if (mode == 2 ? (S != 2 && S != 4) : S != 0)
        return fail(h, NICNES_ERR_INVALID, "nicnes_set_decode_es: S is 2 or 4 with mode 2, and 0 otherwise");
    HIPC(h, hipSetDevice(h->device));
    if (mode) {                        // the partial states of the widest coop shape asked for, as nicnes_set_decode_split
        const int64_t need = (int64_t)h->cfg.max_members * nslabs_of(h->cfg.max_batch, 4) * (mode == 2 ? S : 4);
        if (need > h->part_cap) {
            float* np = nullptr;
            int rc = dalloc(h, &np, (size_t)need * PART_FLOATS);
            if (rc) return rc;
            HIPC(h, hipDeviceSynchronize());
            (void)hipFree(h->part);
            h->part = np;
            h->part_cap = need;
        }
    }
    h->es_dec_mode = mode;
    h->es_dec_S = S;
    return NICNES_OK;
}

int nicnes_decode_path_es(nicnes_handle* h, int32_t B, int32_t count, int32_t* out_host) {
    if (!h || !out_host || B < 1 || count < 1) return NICNES_ERR_INVALID;
    int coop_S = 0;
    if (int rc = es_decode_choice(h, B, count, &coop_S)) return rc;
    *out_host = coop_S ? 2 : 0;
    return NICNES_OK;
}

int nicnes_allgather_fitness_es(nicnes_handle* h, const double* fit_local, int32_t count_local, int32_t n_pairs,
                                double* fit_all, void* stream) {
    ES_STATE(h);
    if (!fit_local || !fit_all || count_local < 1 || n_pairs < 1) return NICNES_ERR_INVALID;
    if (!h->comm) return fail(h, NICNES_ERR_INVALID, "no communicator (nicnes_comm_init / nicnes_comm_attach)");
    int world = 1, rank = 0;
    NCCLC(h, ncclCommCount(h->comm, &world));
    NCCLC(h, ncclCommUserRank(h->comm, &rank));
    if (n_pairs < world) return fail(h, NICNES_ERR_INVALID, "nicnes_allgather_fitness_es: fewer pairs than ranks");
    int begin = 0, share = 0;
    nn_es_shard(n_pairs, rank, world, &begin, &share);
    if (count_local != share)
        return fail(h, NICNES_ERR_INVALID, "nicnes_allgather_fitness_es: count_local is not this rank's share of n_pairs (" +
                                               std::to_string(share) + ")");
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    const int pad = (n_pairs + world - 1) / world;             // the largest share: every rank sends this many pairs
    const size_t need = (size_t)(world + 1) * pad * 2;
    if (need > es->gat_cap) {                                  // (grown at the first gather of a larger generation)
        double* np = nullptr;
        int rc = dalloc(h, &np, need);
        if (rc) return rc;
        if (es->gat) {
            HIPC(h, hipDeviceSynchronize());
            (void)hipFree(es->gat);
        }
        es->gat = np;
        es->gat_cap = need;
    }
    double* send = es->gat;
    double* recv = es->gat + (size_t)pad * 2;
    HIPC(h, hipMemsetAsync(send, 0, (size_t)pad * 2 * sizeof(double), s));
    HIPC(h, hipMemcpyAsync(send, fit_local, (size_t)share * 2 * sizeof(double), hipMemcpyDeviceToDevice, s));
    NCCLC(h, ncclAllGather(send, recv, (size_t)pad * 2, ncclDouble, h->comm, s));
    hipLaunchKernelGGL(es_compact_fitness_kernel, dim3((unsigned)((2 * n_pairs + 255) / 256)), dim3(256), 0, s, recv, fit_all,
                       n_pairs, world, pad);
    HIPC(h, hipGetLastError());
    return NICNES_OK;
}

int nicnes_es_evaluate(nicnes_handle* h, uint64_t generation, int32_t pair_begin, int32_t count, float sigma,
                       const int32_t* parent_of_host, const int32_t* member_batch_host, double* fitness_out,
                       int32_t* seq_out, float* logprob_out, void* stream) {
    ES_STATE(h);
    if (!fitness_out || !parent_of_host || pair_begin < 0) return NICNES_ERR_INVALID;
    const int mode = h->fitness_mode;
    if (mode == NICNES_FITNESS_XENT)
        return fail(h, NICNES_ERR_UNSUPPORTED, "nic_es: the xent fitness is not implemented (greedy, greedy_*)");
    if (mode >= NICNES_FITNESS_SAMPLE)
        return fail(h, NICNES_ERR_UNSUPPORTED, "nic_es: the sampled fitness modes are not implemented (greedy, greedy_*)");
    if ((h->dec_S != 0 && h->dec_S != 1) || (h->dec_G != 0 && h->dec_G != 4))
        return fail(h, NICNES_ERR_UNSUPPORTED, "nic_es decodes on the fused path only: nicnes_set_decode_split(1, 4) or (0, 0)");
    if (count < 1 || count > h->cfg.max_members) return fail(h, NICNES_ERR_INVALID, "count out of [1, max_members]");
    if (!h->noise) return fail(h, NICNES_ERR_INVALID, "nicnes_set_noise_table first");
    if (!h->batch_set) return fail(h, NICNES_ERR_INVALID, "nicnes_set_batch first");
    if (es->n_parents < 1) return fail(h, NICNES_ERR_INVALID, "nicnes_es_set_parent_count first");
    int coop_S = 0;                    // 0: the fused path; 2 or 4: the coop path (nicnes_set_decode_es)
    if (int rc = es_decode_choice(h, h->B, count, &coop_S)) return rc;
    if (int rc = es_sens_ready(h, es, parent_of_host, count)) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIPC(h, hipSetDevice(h->device));
    const int32_t* mb = nullptr;
    if (int rc = stage_member_batch(h, member_batch_host, count, s, &mb)) return rc;
    if (int rc = es_stage_i32(h, parent_of_host, count, es->n_parents, es->parent_of, s, "parent_of")) return rc;
    HIPC(h, nicnes_launch_noise_index(h->cfg.noise_seed, generation, (uint64_t)pair_begin, count, h->cfg.noise_len,
                                      (uint64_t)h->D, h->nidx, s));
    DecodeParams p = decode_base(h);
    p.theta = es->ptab[es->cur];       // (every *_es kernel sets its workgroup's base from ParentArgs)
    if (es->mode) {                    // proportional or divide: the pairs' delta' rows
        if (int rc = ensure_delta_rows(h, &es->dbuf, &es->didx, es->Dp, s)) return rc;
        if (es->mode == NICNES_MUTATION_DIVIDE)
            HIPC(h, nicnes_launch_es_mutate_divide(h->noise, h->nidx, count, es->sens_shared ? es->svec : es->stab,
                                                   es->parent_of, es->sens_shared ? 0 : es->Dp, es->Dp, h->D, sigma,
                                                   es->dbuf, s));
        else
            HIPC(h, nicnes_launch_es_mutate(h->noise, h->nidx, count, es->ptab[es->cur], es->parent_of, es->pmean[es->cur],
                                            es->Dp, h->D, sigma, es->dbuf, s));
        p.noise = es->dbuf;
        p.noise_idx = es->didx;
    } else {                           // plain: the sigma-scaled table
        if (int rc = ensure_noise_scaled(h, sigma, s)) return rc;
        p.noise = h->noise_sc;
        p.noise_idx = h->nidx;
    }
    p.fc = h->fc;
    p.member_batch = mb;
    p.seq = seq_out ? seq_out : h->seq;
    const bool crit_lp = mode >= NICNES_FITNESS_GREEDY_LOGPROB && mode <= NICNES_FITNESS_GREEDY_AVGPROB;
    p.lp = logprob_out ? logprob_out : (crit_lp ? h->lp : nullptr);
    p.scratch = h->dscratch;
    p.alive = h->alive;
    if (int rc = lse_poll(h)) return rc;
    const bool bounded = lse_decide(h, !p.lp);
    p.bounded_lse = bounded ? 1 : 0;
    const int rows = h->B, nslabs = nslabs_of(rows, 4);
    // (screening is a property of the fused path)
    const ScreenArgs sa = pick_screen(h, count, (int64_t)count * nslabs, !coop_S && !p.lp && bounded);
    p.G = 4;
    p.S = coop_S ? coop_S : 1;
    p.part = h->part;
    p.coop = coop_S ? 1 : 0;
    p.test_stall_ms = h->test_stall_left != 0 ? h->test_stall_ms : 0;
    if (p.coop && h->test_stall_ms && h->test_stall_left > 0) --h->test_stall_left;
    p.no_exit = (p.lp && nslabs > 1) ? 1 : 0;
    p.coop_ctr = h->coop_ctr;
    p.alive2 = h->alive + h->alive_stride;
    p.alive_stride = h->alive_stride;
    p.B = rows;
    p.B_img = h->B;
    p.rpi = 1;
    const ParentArgs pa{es->ptab[es->cur], es->parent_of, es->Dp};
    return decode_and_score(h, p, MutHead{}, sa, nullptr, &pa, count, nslabs, (size_t)count * 2 * rows, 2 * count, rows, 1,
                            mb, nullptr, fitness_out, nullptr, s);
}

}  // extern "C"
