// The body of nicnes_decode_coop_kernel<PAIRS, S> (decode_kernel.hip), included where `PAIRS`, `S`, `p` (DecodeParams),
// `nslabs` and `lds` (the dynamic LDS) are in scope: once per __global__ entry, so that an entry added beside it leaves
// its machine code as it was.
    const int L = blockIdx.x, q = L % S, gi = L / S;
    Ctx c;
    c.tid = threadIdx.x;
    c.lane = c.tid & 63;
    c.wave = __builtin_amdgcn_readfirstlane(c.tid >> 6);
    c.sgn = c.wave >> 2;
    c.grp = c.wave & 3;
    c.hh = c.lane >> 5;
    c.member = gi / nslabs;
    c.slab = gi % nslabs;
    c.wg = gi;
    c.b = c.slab * 128 + c.grp * 32 + (c.lane & 31);
    c.row_valid = row_ok(p, c.b, c.sgn);
    c.bc = c.row_valid ? c.b : 0;
    const uint64_t nidx = p.noise_idx[c.member];
    const uint32_t Dbytes = 4u * (uint32_t)p.D;
    c.theta_r = make_rsrc(p.theta, Dbytes);
    c.noise_r = make_rsrc(p.noise + nidx, Dbytes);
    float* wscr = p.scratch + ((size_t)c.wg * 8 + c.wave) * (SCR_SLOTS * 64);
    c.scr_r = make_rsrc(wscr, SCR_SLOTS * 64 * 4);
    uint32_t* ctr = p.coop_ctr + (size_t)gi * COOP_CTR_STRIDE;
    uint32_t phase = 0;
    if (p.test_stall_ms && L == 0) {               // test hook: a partner that arrives past the spin bound
        if (c.tid == 0) {
            const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
            while (__builtin_amdgcn_s_memrealtime() - t0 < 100000ull * p.test_stall_ms) __builtin_amdgcn_s_sleep(127);
        }
        __syncthreads();
    }
    Stage64Regs s64;
    bool pre = false;
    float hB[64];
    for (int t = -1; t <= p.T; ++t)
        if (!coop_step<PAIRS, S>(p, c, q, lds, t, s64, pre, hB, ctr, phase)) break;
