// beam_kernels.hip -- beam-search decode of theta over images of a split (nicnes_split_decode_beam), for evaluation.
// Not a translation unit of its own: decode_kernel.hip #includes this file ahead of its last kernel (the Makefile lists
// it as a dependency), so the library keeps its five code objects and this file uses that unit's tile helpers.
//
// Definition (DESIGN.md "Beam-search decode"): K hypotheses per image, candidates ordered by (fp64 score descending,
// parent ascending, id ascending), the first K taken, a candidate with id 0 or at step T finishes; the result is the
// finished hypothesis of the largest score (ties: earlier step, then earlier selection). No length normalisation.
//
// Layout. One workgroup = NW waves (8, or 4 while the range has too few waves to fill the CUs: the launch picks NW,
// the result does not depend on it); a wave's 32 batch rows (the MFMA's columns) hold floor(32 / K) images x K hypotheses
// in adjacent rows, spare rows dead. Every dense product is the transposed 32x32x2 fp32 MFMA tile of the greedy decode
// (weights of theta staged unperturbed in LDS, activations the B operand), so every chain keeps nn_kperm's k order and
// K = 1 walks the greedy decode's arithmetic. The waves share the staged tiles (workgroup barriers only; no workgroup
// waits on another). Selection, the parent gather of h and c (wave permutes), the token history and the finished pool
// (LDS rows of the wave) stay inside a wave. h' of a cell and x of t = 0 pass through lane-PRIVATE global scratch: a
// lane reloads only values it stored itself, so no other lane's store has to be visible.
#define BEAM_MAX 8
#define BM_NONE 0x7fffffff
#define BM_TILE_FLOATS (32 * LDS_ROW + 32)             // one 32-row tile of theta | its 32 biases
#define BM_HIST_AT (2 * BM_TILE_FLOATS)                // uint16 [NW waves][32 rows][16]: tokens of each hypothesis
#define BM_FIN_AT(NW) (BM_HIST_AT + (NW) * 32 * 16 / 2)        // uint16 [NW waves][32 images][16]: the best finished
#define BM_LDS_FLOATS(NW) (BM_FIN_AT(NW) + (NW) * 32 * 16 / 2) // 50,432 bytes at NW = 8
#define BM_SCR_SLOTS 128                               // per lane: x of t = 0 (64) | h' (64)

struct BeamArgs {
    int32_t* seq;        // out [count, T]
    double* score;       // out [count]
    float* xscr;         // [workgroups][BM_SCR_SLOTS][64 NW] lane-private scratch
    int32_t count, K;
};

template <int NT>
struct BmRegs {
    f32x4 w[1024 / NT];      // a tile is 32 rows x 32 quads over the workgroup's NT threads
    float b;
};

// the unperturbed tile: stage_load / stage_store without the noise slice (theta_r bounds every read to theta)
template <int NT>
__device__ __forceinline__ void bm_load(rsrc_t theta_r, const TileDesc& d, int tid, BmRegs<NT>& s) {
#pragma unroll
    for (int u = 0; u < 1024 / NT; ++u) {
        const int f = tid + NT * u, row = f >> 5, q = f & 31;
        const int rc = row < d.nvalid ? row : max(d.nvalid - 1, 0);
        const f32x4 w = ld4(theta_r, 4u * (d.w_off + (uint32_t)((d.row0 + rc) * d.ld + d.k0 + 4 * q)));
        s.w[u] = row < d.nvalid ? w : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int r = tid & 31;
    s.b = ld1(theta_r, 4u * (d.b_off + (uint32_t)(d.row0 + (r < d.nvalid ? r : 0))));
}

template <int NT>
__device__ __forceinline__ void bm_store(float* buf, const TileDesc& d, int tid, const BmRegs<NT>& s) {
#pragma unroll
    for (int u = 0; u < 1024 / NT; ++u) {
        const int f = tid + NT * u, row = f >> 5, q = f & 31;
        const int T = q >> 3, hh = q & 1, a = (q & 7) >> 1;
        *reinterpret_cast<f32x4*>(buf + row * LDS_ROW + T * 32 + hh * 16 + 4 * a) = s.w[u];
    }
    if (tid < 32) buf[32 * LDS_ROW + tid] = tid < d.nvalid ? s.b : d.pad_bias;
}

// n tiles through the two LDS buffers, one barrier per tile: tile i + 1 is loaded before and stored after the MFMAs of
// tile i. N > 0: n = N and the loop is unrolled (compute sees i as a constant).
template <int NT, int N, class Desc, class Compute>
__device__ __forceinline__ void bm_tiles(float* lds, rsrc_t theta_r, int tid, int n, Desc desc, Compute compute) {
    BmRegs<NT> r;
    __syncthreads();                         // every wave has read the previous phase's last tile
    {
        const TileDesc d = desc(0);
        bm_load(theta_r, d, tid, r);
        bm_store(lds, d, tid, r);
    }
    auto body = [&](int i) __attribute__((always_inline)) {
        __syncthreads();                     // tile i stored; tile i - 1 (the buffer tile i + 1 goes to) read by all
        const bool more = i + 1 < n;
        TileDesc dn{};
        if (more) {
            dn = desc(i + 1);
            bm_load(theta_r, dn, tid, r);
        }
        compute(i, lds + (i & 1) * BM_TILE_FLOATS);
        if (more) bm_store(lds + ((i + 1) & 1) * BM_TILE_FLOATS, dn, tid, r);
    };
    if constexpr (N > 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) body(i);
    } else {
        for (int i = 0; i < n; ++i) body(i);
    }
}

// ---- per-lane sorted top-K of (logit, id) ------------------------------------------------------------------------
// A lane's ids only grow (tile by tile, and inside a tile with r), so a strict > keeps the earlier id first on ties.
// Entries from K on stay empty (-inf, BM_NONE).
struct BmTop {
    float x[BEAM_MAX];
    int v[BEAM_MAX];
    float kth;            // x[K - 1]
};

__device__ __forceinline__ void bm_top_init(BmTop& t) {
#pragma unroll
    for (int j = 0; j < BEAM_MAX; ++j) {
        t.x[j] = NEG_INF;
        t.v[j] = BM_NONE;
    }
    t.kth = NEG_INF;
}

__device__ __forceinline__ void bm_top_insert(BmTop& t, float x, int v, int K) {
#pragma unroll
    for (int j = BEAM_MAX - 1; j >= 0; --j) {      // descending: x[j - 1] is still the old entry
        const bool cj = j < K && x > t.x[j];
        const bool cp = j > 0 && x > t.x[j > 0 ? j - 1 : 0];
        t.v[j] = cj ? (cp ? t.v[j > 0 ? j - 1 : 0] : v) : t.v[j];
        t.x[j] = cj ? (cp ? t.x[j > 0 ? j - 1 : 0] : x) : t.x[j];
    }
}

// one 32-id tile: P[r] is id vbase + (r & 3) + 8 (r >> 2) + 4 hh. The tile is scanned only when its maximum beats some
// lane's K-th entry (the records_scan pattern of the greedy epilogue).
__device__ __forceinline__ void bm_top_tile(BmTop& t, const f32x16& P, int vbase, int hh, int K) {
    const float tmax = vmax16(P);
    if (!__any(tmax > t.kth)) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) bm_top_insert(t, P[r], vbase + (r & 3) + 8 * (r >> 2) + 4 * hh, K);
    float k = NEG_INF;
#pragma unroll
    for (int j = 0; j < BEAM_MAX; ++j) k = j == K - 1 ? t.x[j] : k;
    t.kth = k;
}

// ---- selection: the first min(K, candidates) of an image's candidates, in order ------------------------------------
// The rows of an image are K adjacent batch rows of the wave; both lane halves of a row hold a sorted list. Log-probs
// are lp = fl32(fl32(x - m) - lse); a lane's list is put in (lp descending, id ascending) order (rounding can merge
// different logits into one log-prob), then K rounds each take the best head of the image's 2K lanes by (score
// descending, row ascending, id ascending). pick(k, ok, row, id, score) is called by every lane with its image's k-th
// selection (ok false: the image has no candidate left). The membership cut of a lane's list is by logit: it differs
// from the definition only if the K-th and a later logit of one lane round to the same log-prob with the later id
// smaller -- neighbours closer than the tests' fragility bound.
template <class Pick>
__device__ __forceinline__ void bm_select(const BmTop& t, float m, float lse, bool live, double score, int K, int lane,
                                          Pick pick) {
    const int base = ((lane & 31) / K) * K;
    float lp[BEAM_MAX];
    int id[BEAM_MAX];
#pragma unroll
    for (int j = 0; j < BEAM_MAX; ++j) {
        const bool ok = live && j < K && t.v[j] != BM_NONE;
        lp[j] = ok ? (t.x[j] - m) - lse : NEG_INF;
        id[j] = ok ? t.v[j] : BM_NONE;
    }
#pragma unroll
    for (int pass = 0; pass < BEAM_MAX - 1; ++pass)
#pragma unroll
        for (int j = 0; j < BEAM_MAX - 1 - pass; ++j) {
            const bool sw = lp[j] == lp[j + 1] && id[j] > id[j + 1];      // equal log-probs: only the ids move
            const int a = id[j], b = id[j + 1];
            id[j] = sw ? b : a;
            id[j + 1] = sw ? a : b;
        }
    int ptr = 0;
    for (int k = 0; k < K; ++k) {
        float hl = NEG_INF;
        int hv = BM_NONE;
#pragma unroll
        for (int j = 0; j < BEAM_MAX; ++j) {
            hl = ptr == j ? lp[j] : hl;
            hv = ptr == j ? id[j] : hv;
        }
        const double hs = score + (double)hl;
        double ws = 0.0;
        int wv = BM_NONE, wl = 0;
        for (int jj = 0; jj < 2 * K; ++jj) {      // rows ascending, the two halves of a row side by side
            const int src = (base + (jj >> 1) + 32 * (jj & 1)) & 63;
            const double s = __shfl(hs, src);
            const int v = __shfl(hv, src);
            const bool same_row = ((src ^ wl) & 31) == 0;
            const bool better = v != BM_NONE && (wv == BM_NONE || s > ws || (s == ws && same_row && v < wv));
            ws = better ? s : ws;
            wv = better ? v : wv;
            wl = better ? src : wl;
        }
        if (wv != BM_NONE && lane == wl) ++ptr;
        pick(k, wv != BM_NONE, wl & 31, wv, ws);
    }
}

// ---- the decode ----------------------------------------------------------------------------------------------------
template <int NW>
__global__ __launch_bounds__(64 * NW) void nicnes_beam_decode_kernel(DecodeParams p, BeamArgs ba) {
    constexpr int NT = 64 * NW;
    __shared__ float lds[BM_LDS_FLOATS(NW)];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 31, hh = lane >> 5;
    const int K = ba.K, T = p.T, ipw = 32 / K, ipwg = NW * ipw;
    const int g = n / K, r = n - g * K;
    const bool rowuse = g < ipw;
    const int wg_img0 = (int)blockIdx.x * ipwg;
    const int li = wave * ipw + g;                       // the image inside the workgroup
    const int img = wg_img0 + li;
    const bool valid = rowuse && img < ba.count;
    const int wg_imgs = min(ipwg, ba.count - wg_img0);   // >= 1: the grid is ceil(count / ipwg)
    const rsrc_t theta_r = make_rsrc(p.theta, 4u * (uint32_t)p.D);
    const rsrc_t fc_r = make_rsrc(p.fc + (size_t)wg_img0 * (size_t)p.F, 4u * (uint32_t)wg_imgs * (uint32_t)p.F);
    float* const scr = ba.xscr + (size_t)blockIdx.x * (BM_SCR_SLOTS * NT) + tid;   // slot s at scr[s * NT]
    uint16_t* const hist = reinterpret_cast<uint16_t*>(lds + BM_HIST_AT) + wave * (32 * 16);
    uint16_t* const fin = reinterpret_cast<uint16_t*>(lds + BM_FIN_AT(NW)) + wave * (32 * 16);

    // ---- image step: x0 = img_embed(fc), unit tile by unit tile, into the lane's own scratch --------------------------
    {
        const int nK = p.F >> 7;
        const uint32_t frow = 4u * (uint32_t)((valid ? li : 0) * p.F + 4 * hh);
        f32x16 acc;
        bm_tiles<NT, 0>(lds, theta_r, tid, 4 * nK,
                    [&](int i) __attribute__((always_inline)) {
                        TileDesc d;
                        d.w_off = (uint32_t)p.off_img_w; d.ld = p.F; d.row0 = 32 * (i / nK); d.nvalid = 32;
                        d.k0 = 128 * (i % nK); d.b_off = (uint32_t)p.off_img_b; d.pad_bias = 0.f;
                        return d;
                    },
                    [&](int i, const float* buf) __attribute__((always_inline)) {
                        const int U = i / nK, kc = i - U * nK;
                        if (kc == 0) acc = bias_init(buf + 32 * LDS_ROW, hh);
                        acc = mfma_tile_fc(acc, buf, fc_r, frow + 4u * 128u * (uint32_t)kc, lane);
                        if (kc == nK - 1) {
#pragma unroll
                            for (int e = 0; e < 16; ++e) scr[(16 * U + e) * NT] = acc[e];
                        }
                    });
    }

    float Bh[64], c[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        Bh[i] = 0.f;
        c[i] = 0.f;
    }

    // ---- one LSTM cell: gate sums i2h(x) + h2h(h) tile by tile (order g1, g2, in, forget, out per 32-unit block), c in
    // place, h' through the lane's scratch (h stays the B operand until the last gate tile) -----------------------------
    auto cell = [&](bool first, int tok) __attribute__((always_inline)) {
        const uint32_t xrow = 4u * (uint32_t)((uint32_t)p.off_emb_w + (uint32_t)tok * 128u + 4u * (uint32_t)hh);
        f32x16 accx, gA;
        bm_tiles<NT, 40>(lds, theta_r, tid, 40,
                     [&](int i) __attribute__((always_inline)) {
                         const int m = i >> 1;
                         TileDesc d;
                         d.ld = 128; d.row0 = (int)gate_row(m); d.nvalid = 32; d.k0 = 0; d.pad_bias = 0.f;
                         d.w_off = (uint32_t)((i & 1) ? p.off_h2h_w : p.off_i2h_w);
                         d.b_off = (uint32_t)((i & 1) ? p.off_h2h_b : p.off_i2h_b);
                         return d;
                     },
                     [&](int i, const float* buf) __attribute__((always_inline)) {
                         const int m = i >> 1, ub = m / 5, j = m % 5;
                         if (!(i & 1)) {
                             accx = bias_init(buf + 32 * LDS_ROW, hh);
                             if (first) {         // x of t = 0: the lane's own accumulators of the image step
                                 const float* row = buf + (lane & 31) * LDS_ROW + (lane >> 5) * 16;
                                 for (int Tb = 0; Tb < 4; ++Tb) {
                                     f32x4 a[4];
                                     float bq[16];
#pragma unroll
                                     for (int q = 0; q < 4; ++q) a[q] = *reinterpret_cast<const f32x4*>(row + Tb * 32 + 4 * q);
#pragma unroll
                                     for (int e = 0; e < 16; ++e) bq[e] = scr[(16 * Tb + e) * NT];
#pragma unroll
                                     for (int jj = 0; jj < 16; ++jj)
                                         accx = __builtin_amdgcn_mfma_f32_32x32x2f32(a[jj >> 2][jj & 3], bq[jj], accx, 0, 0, 0);
                                 }
                             } else {             // the token's embedding row, read as the image step reads fc
                                 accx = mfma_tile_fc(accx, buf, theta_r, xrow, lane);
                             }
                             return;
                         }
                         f32x16 s = bias_init(buf + 32 * LDS_ROW, hh);
                         s = mfma_tile(s, buf, Bh, lane);
                         s = accx + s;                                         // i2h(x) + h2h(h), nets.py:109-111
                         if (j == 0) {
                             gA = s;
                         } else if (j == 1) {
#pragma unroll
                             for (int e = 0; e < 16; ++e) gA[e] = gA[e] > s[e] ? gA[e] : s[e];
                         } else if (j == 2) {
#pragma unroll
                             for (int e = 0; e < 16; ++e) gA[e] = nn_sigmoidf(s[e]) * gA[e];
                         } else if (j == 3) {
#pragma unroll
                             for (int e = 0; e < 16; ++e) {
                                 const float fcv = nn_sigmoidf(s[e]) * c[16 * ub + e];
                                 c[16 * ub + e] = fcv + gA[e];
                             }
                         } else {
#pragma unroll
                             for (int e = 0; e < 16; ++e)
                                 scr[(64 + 16 * ub + e) * NT] = nn_sigmoidf(s[e]) * nn_tanhf(c[16 * ub + e]);
                         }
                     });
#pragma unroll
        for (int e = 0; e < 64; ++e) Bh[e] = scr[(64 + e) * NT];
    };

    // the image's result row starts as the empty caption: an image that never finishes a hypothesis (non-finite
    // logits give no candidate) reports zeros and a score of -inf, not stale LDS
    if (rowuse && r == 0 && hh == 0)
        for (int t = 0; t < 16; ++t) fin[g * 16 + t] = 0;
    bool live = valid && r == 0;
    double score = 0.0, bestfin = -__builtin_inf();
    const int nst = (p.V1 + 31) >> 5;
    int ntok = 0;

    // s = 0: the image (FCModel._sample t = 0); s = 1: BOS (embedding row 0), then the first logits
    for (int s = 0;; ++s) {
        cell(s == 0, ntok);
        if (s == 0) continue;
        // ---- logits of step s over h: per lane the sorted top-K and the online exp-sum ------------------------------
        BmTop top;
        bm_top_init(top);
        float lm = -1.0e30f, ls = 0.f;
        bm_tiles<NT, 0>(lds, theta_r, tid, nst,
                    [&](int i) __attribute__((always_inline)) {
                        TileDesc d;
                        d.w_off = (uint32_t)p.off_log_w; d.ld = 128; d.row0 = 32 * i; d.nvalid = min(32, p.V1 - 32 * i);
                        d.k0 = 0; d.b_off = (uint32_t)p.off_log_b; d.pad_bias = NEG_INF;
                        return d;
                    },
                    [&](int i, const float* buf) __attribute__((always_inline)) {
                        f32x16 P = bias_init(buf + 32 * LDS_ROW, hh);
                        P = mfma_tile(P, buf, Bh, lane);
                        bm_top_tile(top, P, 32 * i, hh, K);
                        const float mnew = vmax2(lm, vmax16(P));
                        const float ml = mnew * LOG2E;
                        float sum = ls * __builtin_amdgcn_exp2f((lm - mnew) * LOG2E);
                        expsum16(sum, P, ml);
                        ls = sum;
                        lm = mnew;
                    });
        const float m_o = __shfl_xor(lm, 32), s_o = __shfl_xor(ls, 32);
        const float m = fmaxf(lm, m_o);
        const float stot = ls * __builtin_amdgcn_exp2f((lm - m) * LOG2E) + s_o * __builtin_amdgcn_exp2f((m_o - m) * LOG2E);
        const float lse = logf(stot);

        // ---- selection ------------------------------------------------------------------------------------------------
        int nlive = 0, npar = n;
        double nscore = 0.0;
        ntok = 0;
        bm_select(top, m, lse, live, score, K, lane, [&](int k, bool ok, int prow, int v, double ws) __attribute__((always_inline)) {
            if (!ok) return;
            if (v == 0 || s == T) {                  // finishes: the parent's tokens, and v at step T
                if (ws > bestfin) {                  // strict: an earlier finisher keeps a tie
                    bestfin = ws;
                    if (rowuse && r == 0 && hh == 0)
                        for (int t = 0; t < T; ++t)
                            fin[g * 16 + t] = t < s - 1 ? hist[prow * 16 + t] : (uint16_t)(t == s - 1 ? v : 0);
                }
            } else {
                if (r == nlive) {
                    npar = prow;
                    ntok = v;
                    nscore = ws;
                }
                ++nlive;
            }
        });
        // the first live selection has the largest live score: the image stops once the best finished one is at least it
        const double top_live = __shfl(nscore, ((n - r) + 32 * hh) & 63);
        const bool done = nlive == 0 || bestfin >= top_live;
        live = rowuse && !done && r < nlive;
        score = nscore;
        if (!live) {
            npar = n;
            ntok = 0;
        }
        if (!__syncthreads_or(live ? 1 : 0)) break;

        // ---- parent gather: h, c by wave permutes, the token history through the wave's LDS rows ----------------------
        const int pl = npar + 32 * hh;
#pragma unroll
        for (int i = 0; i < 64; ++i) {
            Bh[i] = __shfl(Bh[i], pl);
            c[i] = __shfl(c[i], pl);
        }
        uint16_t hv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) hv[e] = hist[npar * 16 + 8 * hh + e];
        wave_lds_order();
#pragma unroll
        for (int e = 0; e < 8; ++e) hist[n * 16 + 8 * hh + e] = (8 * hh + e == s - 1) ? (uint16_t)ntok : hv[e];
        wave_lds_order();
    }

    if (valid && r == 0 && hh == 0) {
        for (int t = 0; t < T; ++t) ba.seq[(size_t)img * T + t] = (int32_t)fin[g * 16 + t];
        ba.score[img] = bestfin;
    }
}

// both shapes are emitted here, in source order (an implicit instantiation would land behind the unit's other kernels)
template __global__ void nicnes_beam_decode_kernel<4>(DecodeParams, BeamArgs);
template __global__ void nicnes_beam_decode_kernel<8>(DecodeParams, BeamArgs);

// test entry (nicnes_test_beam_select): bm_top_tile and bm_select over given log-prob rows [n_img, K, V1], scores and
// live flags [n_img, K]; out [n_img, K, 2] receives the selected (row of the image, id) pairs in order (the host fills
// it with -1). One wave per workgroup, floor(32 / K) images per wave, as the decode lays them out.
__global__ __launch_bounds__(64) void nicnes_test_beam_select_kernel(const float* __restrict__ lp,
                                                                     const double* __restrict__ score,
                                                                     const int32_t* __restrict__ live_in, int n_img, int K,
                                                                     int V1, int32_t* __restrict__ out) {
    const int lane = (int)threadIdx.x, n = lane & 31, hh = lane >> 5;
    const int ipw = 32 / K, g = n / K, r = n - g * K;
    const int img = (int)blockIdx.x * ipw + g;
    const bool valid = g < ipw && img < n_img;
    const size_t row = valid ? (size_t)img * K + r : 0;
    BmTop top;
    bm_top_init(top);
    for (int i = 0; i < (V1 + 31) >> 5; ++i) {
        f32x16 P;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int v = 32 * i + (e & 3) + 8 * (e >> 2) + 4 * hh;
            P[e] = valid && v < V1 ? lp[row * (size_t)V1 + v] : NEG_INF;
        }
        bm_top_tile(top, P, 32 * i, hh, K);
    }
    const bool live = valid && live_in[row] != 0;
    const double sc = valid ? score[row] : 0.0;
    bm_select(top, 0.f, 0.f, live, sc, K, lane, [&](int k, bool ok, int prow, int v, double) __attribute__((always_inline)) {
        if (ok && valid && r == 0 && hh == 0) {
            out[((size_t)img * K + k) * 2] = prow - g * K;
            out[((size_t)img * K + k) * 2 + 1] = v;
        }
    });
}

// every workgroup shape needs the same scratch: 64 BM_SCR_SLOTS floats per wave
extern "C" size_t nicnes_beam_scratch_floats(int count, int K) {
    const int ipw = 32 / K;
    return (size_t)((count + ipw - 1) / ipw + 7) * BM_SCR_SLOTS * 64;
}

template <int NW>
static hipError_t bm_launch(const DecodeParams* p, const BeamArgs& ba, int waves, hipStream_t s) {
    hipLaunchKernelGGL(nicnes_beam_decode_kernel<NW>, dim3((unsigned)((waves + NW - 1) / NW)), dim3(64 * NW), 0, s, *p, ba);
    return hipGetLastError();
}

// Waves per workgroup: 8 (two per SIMD, every staged tile shared by eight) or 4 (one per SIMD). A workgroup of 4
// finishes in 0.70 of the time a workgroup of 8 takes (21.5 ms against 30.7 ms at the default dims, measured:
// DESIGN.md "Beam-search decode"; one workgroup of either shape is resident per CU), so the launch takes the shape whose
// rounds over the CUs cost less: 4 while the range's waves leave CUs idle, 8 for long ranges. n_cu <= 0: always 8.
extern "C" int nicnes_beam_waves_per_wg(int count, int K, int n_cu) {
    if (n_cu <= 0) return 8;
    const int ipw = 32 / K, waves = (count + ipw - 1) / ipw;
    const int r4 = ((waves + 3) / 4 + n_cu - 1) / n_cu, r8 = ((waves + 7) / 8 + n_cu - 1) / n_cu;
    return 7 * r4 < 10 * r8 ? 4 : 8;
}

extern "C" hipError_t nicnes_launch_beam_decode(const DecodeParams* p, int32_t* seq, double* score, float* xscr,
                                                int count, int K, int n_cu, int force_nw, hipStream_t s) {
    if (count < 1 || K < 1 || K > BEAM_MAX) return hipErrorInvalidValue;
    const int ipw = 32 / K, waves = (count + ipw - 1) / ipw;
    const BeamArgs ba{seq, score, xscr, count, K};
    if ((force_nw > 0 ? force_nw : nicnes_beam_waves_per_wg(count, K, n_cu)) == 4) return bm_launch<4>(p, ba, waves, s);
    return bm_launch<8>(p, ba, waves, s);
}

extern "C" hipError_t nicnes_launch_test_beam_select(const float* lp, const double* score, const int32_t* live, int n_img,
                                                     int K, int V1, int32_t* out, hipStream_t s) {
    if (n_img < 1 || K < 1 || K > BEAM_MAX || V1 < 1) return hipErrorInvalidValue;
    const int ipw = 32 / K;
    hipLaunchKernelGGL(nicnes_test_beam_select_kernel, dim3((unsigned)((n_img + ipw - 1) / ipw)), dim3(64), 0, s, lp,
                       score, live, n_img, K, V1, out);
    return hipGetLastError();
}
