"""The worlds of the screened decode's misorder tests: tests/test_screen_worlds_host.py (their preconditions, on the CPU)
and tests/test_gpu_screen_misorder.py (the GPU). TEST INFRASTRUCTURE ONLY. Everything is made from numpy PCG64 seeds
and the CPU references, once per process, and never modified afterwards.

What the worlds are for. The bf16-screened logit loop is right only if every id that can win the fp32
greedy pick survives the screen. On random theta the fp32 winner is the screened maximum too, and rows that share one
logit row share one bf16 error: there the screened maximum's own hit carries the right token whatever happens to the
rest of the window. Here the screen ranks the exact winner `a` BELOW another id `b`.

The plant. h is the target image's hidden state at the first logit step (ln_ref.Model(layer_n=False): the oracle bit
for bit). `base` is a bf16-exact logit row, d_k = rel |base_k| sign(h_k), and the two fp32 rows
    W_a = base + d,  W_b = base - d       (bf16(W_a) == bf16(W_b) == base: rel < 2^-9)
have the same bf16 products, while exactly L_a - L_b = G - (b_b - b_a) with G = 2 sum_k |d_k h_k| > 0. With b_a set so
that L_a is the row's old top logit + 4 and b_b = b_a + frac G (the screen does not round biases), the screen sees b
ahead of a by frac G and the fp32 chain a ahead of b by (1 - frac) G.
  shallow   base = bf16(the logit row of the target's old first token), rel = 2^-10, frac = 0.5
  aligned   base = bf16(kappa h) with ||base|| = 1.05 x the largest logit-row norm, rel = 0.99 2^-9, frac = 0.75:
            Cauchy-Schwarz is tight, the depth of a below the screened maximum is the largest share of the window
            (2 eps) a weight-side plant can reach.
  triple    rows base + d, base, base - d at a, a + 8, a + 16 with biases b0, b0 + frac G / 2, b0 + frac G: the exact
            order is a > a + 8 > a + 16, the screened order its reverse.
  sigma     the plant is made on the theta of member 1, sign -, at sigma = 0.01: the rows and biases of theta itself
            are solved for (row + delta), and the preconditions are checked on theta - delta as the engine forms it.

Id layout (ListItems, csrc/decode_kernel.hip): v = 64 s + 32 c + 4 hh + (x & 3) + 8 (x >> 2), x in 0 .. 15: stage s,
tile c (P0 / P1 of one epilogue), lane half hh, and the lane-stage's pair pr = 8 c + (x >> 1) (x = 2 (pr & 7), + 1).
One word per lane and stage points at the pair of the lane-stage's maximum, or carries the crowded flag.

Batch: B = 130 (a second slab), the target image at slab rows TARGET_ROWS (every wave's 32-row group and slab 1), the
other rows random images. Vocabularies: 9487 (149 stages, the last with 16 ids), 999 (16 stages, the last with tile 0
full and 8 ids of tile 1), 63 (one stage)."""
import numpy as np

from oracle import oracle as O
from tests import ln_ref as L
from tests.test_screen_bound import bf16

E = R = 128
F, T, B = 2048, 16, 130
TARGET_ROWS = (0, 31, 32, 63, 64, 96, 127, 129)
FRAGILE_CAP = 0.05
NOISE_LEN, TABLE_SEED, NOISE_SEED, IT = 1 << 23, 123, 11, 5
SIGMA, SIGMA_MEMBER, SIGMA_SIGN = 0.01, 1, -1
MEMBERS = 3                                   # the members a sigma case is decoded for (the step queue's three)
THETA_SEED, FC_SEED = 0, {9487: 4321, 999: 4322, 63: 4323}
VARIANTS = {'shallow': dict(rel=2.0 ** -10, frac=0.5, floor=0.02), 'aligned': dict(rel=0.99 * 2.0 ** -9, frac=0.75, floor=0.10)}
F32 = np.float32

_cache = {}


def once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---------------------------------------------------------------------------------------------- the id layout
def vid(s, c, hh, x):
    return 64 * s + 32 * c + 4 * hh + (x & 3) + 8 * (x >> 2)


def stage(v):
    return v >> 6


def tile(v):
    return (v >> 5) & 1


def lane_half(v):
    return (v >> 2) & 1


def group(v):
    return (v >> 3) & 3


def pair(v):
    """the pair of v's lane-stage that holds it, 0 .. 15"""
    return 8 * tile(v) + 2 * group(v) + ((v >> 1) & 1)


def lane_stage(v):
    return stage(v), lane_half(v)


def pair_id(s, pr, hh, odd=1):
    """the even (odd = 0) or odd id of pair pr of lane half hh in stage s"""
    return vid(s, pr >> 3, hh, 2 * (pr & 7) + odd)


# ---------------------------------------------------------------------------------------------- the references
def noise_table():
    return once('table', lambda: O.noise_table(NOISE_LEN, TABLE_SEED))


def member_theta(theta, member, sign):
    dims_D = theta.size
    return O.perturb(theta, noise_table(), O.noise_index(NOISE_SEED, IT, member, NOISE_LEN, dims_D), SIGMA, sign)


def logit_rows(dims, theta):
    """writable views (weight [V1, R], bias [V1]) of the logit layer inside theta"""
    o = dims.offsets()
    w0, b0 = o['logit.weight'][0], o['logit.bias'][0]
    return theta[w0:w0 + dims.V1 * dims.R].reshape(dims.V1, dims.R), theta[b0:b0 + dims.V1]


def step1_h(dims, theta, fc):
    """h [rows, R] at the first logit step (the image cell, then the cell on BOS)"""
    m = L.Model(dims, theta, layer_n=False)
    z = np.zeros((fc.shape[0], dims.R), F32)
    h, c = m.cell(m.product(m.Wimg, m.bimg, fc), z, z)
    h, c = m.cell(m.emb[np.zeros(fc.shape[0], np.int64)], h, c)
    return h


def world(vocab):
    """the unplanted world of a vocabulary: dims, theta, the batch, the target's h and logits at the first step"""
    def make():
        dims = O.Dims(vocab_size=vocab, E=E, R=R, F=F, T=T)
        theta = O.make_theta(dims, THETA_SEED, 4.0, 0.1)
        fc = np.random.Generator(np.random.PCG64(FC_SEED[vocab])).standard_normal((B, F)).astype(F32)
        fc[list(TARGET_ROWS)] = fc[0]
        h = step1_h(dims, theta, fc[:1])[0]
        lw, lb = logit_rows(dims, theta)
        z = O.gemv(lw, lb, h)
        return _freeze(dict(dims=dims, theta=theta, fc=fc, h=h, z=z, tok=int(L.greedy_pick(z)[0])))
    return once(('world', vocab), make)


# ---------------------------------------------------------------------------------------------- the plant
def _dot(w, h):
    return float(w.astype(np.float64) @ h.astype(np.float64))


def plant_rows(lw, lb, h, ids, variant, tok):
    """Plants the rows of `ids` = (a, b) or (a, a + 8, a + 16) into the logit layer (lw, lb) for the hidden row h.
    -> G. tok: the id whose row is the shallow base (the row's first token before the plant)."""
    v = VARIANTS[variant]
    top = float(O.gemv(lw, lb, h).max())
    if variant == 'shallow':
        base = bf16(lw[tok])
    else:
        want = 1.05 * float(np.sqrt((lw.astype(np.float64) ** 2).sum(1).max()))
        kappa = want / float(np.linalg.norm(h.astype(np.float64)))
        for _ in range(3):                                            # (bf16 rounding moves the norm a little)
            base = bf16((kappa * h.astype(np.float64)).astype(F32))
            kappa *= want / float(np.linalg.norm(base.astype(np.float64)))
    d = (F32(v['rel']) * np.abs(base) * np.sign(h)).astype(F32)
    rows = [(base + d).astype(F32), (base - d).astype(F32)]
    if len(ids) == 3:
        rows.insert(1, base.copy())
    G = _dot(rows[0], h) - _dot(rows[-1], h)
    b0 = top + 4.0 - _dot(rows[0], h)
    n = len(ids) - 1
    for j, (i, w) in enumerate(zip(ids, rows)):
        lw[i] = w
        lb[i] = F32(b0 + v['frac'] * G * j / n)
    return G


# case -> (ids at V = 999, ids at V = 9487 or None, starred); ids = (a, b) or the triple; V1: 1000 / 9488
def _cases():
    c = {}

    def add(name, ids, star=False, big=True, small=True):
        c[name] = dict(ids=ids, star=star, big=big and star, small=small)
    a = vid(5, 1, 1, 10)                                   # pair 13 of half 1
    add('same_pair_lo', lambda V1: (a, a ^ 1), star=True)
    add('same_pair_hi', lambda V1: (a ^ 1, a), star=True)
    add('other_pair_same_group', lambda V1: (vid(7, 0, 1, 5), vid(7, 0, 1, 5) ^ 2))
    add('other_group_same_tile', lambda V1: (vid(5, 0, 0, 4), vid(5, 0, 0, 4) + 8), star=True)
    add('other_tile', lambda V1: (vid(6, 1, 1, 9), vid(6, 1, 1, 9) ^ 32), star=True)
    add('pair_15_wins', lambda V1: (64 * 3 + 32 + 24 + 2, 64 * 3 + 1))
    add('pair_15_leads', lambda V1: (64 * 3 + 1, 64 * 3 + 32 + 24 + 2))
    add('other_half', lambda V1: (vid(5, 0, 0, 6), vid(5, 0, 0, 6) ^ 4), star=True)
    add('next_stage', lambda V1: (vid(8, 1, 0, 11), vid(8, 1, 0, 11) + 64), star=True)
    add('far_stage', lambda V1: (vid(20, 0, 1, 13), vid(20, 0, 1, 13) + 64 * 17), star=True, small=False)
    add('last_id_wins', lambda V1: (V1 - 1, vid(0, 0, 0, 6)), star=True)
    add('last_id_leads', lambda V1: (vid(0, 0, 0, 6), V1 - 1))
    add('end_token_wins', lambda V1: (0, vid(2, 1, 1, 12)))
    add('triple_reversed', lambda V1: (vid(4, 0, 1, 2), vid(4, 0, 1, 2) + 8, vid(4, 0, 1, 2) + 16), star=True)
    add('negative_logits', lambda V1: (vid(4, 0, 1, 11), vid(4, 0, 1, 11) + 64))
    add('sigma_member', lambda V1: (vid(9, 1, 0, 13), vid(9, 1, 0, 13) - 64 * 3), star=True)
    return c


CASES = _cases()
NEG_SHIFT = 40.0


def plant_list():
    """every (case, vocab, variant) that is planted"""
    out = [(n, 999, 'shallow') for n, c in CASES.items() if c['small']]
    out += [(n, 9487, v) for n, c in CASES.items() if c['big'] for v in VARIANTS]
    return out


def starred_list():
    return [(n, 9487, v) for n, c in CASES.items() if c['big'] for v in VARIANTS]


def planted(case, vocab, variant):
    """A planted world. theta: what the engine is given; ids: (a, b[, c]) with a the exact winner and ids[-1] the
    screened leader; sigma: what the decode runs at (0, or SIGMA for sigma_member); W, b, h: the logit layer and the
    target's hidden row the preconditions hold on (of member SIGMA_MEMBER, sign SIGMA_SIGN in the sigma case); oseq,
    ofr [members, 2, B, T]: the oracle's decode of every member and sign (one decode repeated at sigma = 0)."""
    def make():
        w = world(vocab)
        dims, fc = w['dims'], w['fc']
        ids = CASES[case]['ids'](dims.V1)
        assert len(set(ids)) == len(ids) and all(0 <= v < dims.V1 for v in ids), (case, vocab, ids)
        theta = w['theta'].copy()
        if case == 'negative_logits':
            logit_rows(dims, theta)[1][:] -= F32(NEG_SHIFT)
        if case == 'sigma_member':
            sigma = SIGMA
            th_m = member_theta(theta, SIGMA_MEMBER, SIGMA_SIGN)
            delta = O.member_delta(noise_table(), O.noise_index(NOISE_SEED, IT, SIGMA_MEMBER, NOISE_LEN, theta.size),
                                   SIGMA, theta.size)                            # what the engine subtracts / adds
            h = step1_h(dims, th_m, fc[:1])[0]                                   # (the logit layer does not enter h)
            lw_m, lb_m = logit_rows(dims, th_m)
            tok = int(L.greedy_pick(O.gemv(lw_m, lb_m, h))[0])
            G = plant_rows(lw_m, lb_m, h, ids, variant, tok)
            (lw, lb), (dw, db) = logit_rows(dims, theta), logit_rows(dims, delta)
            for v in ids:                                                        # theta -+ delta = the planted rows
                lw[v] = (lw_m[v] + dw[v]) if SIGMA_SIGN < 0 else (lw_m[v] - dw[v])
                lb[v] = (lb_m[v] + db[v]) if SIGMA_SIGN < 0 else (lb_m[v] - db[v])
            W, b = (x.copy() for x in logit_rows(dims, member_theta(theta, SIGMA_MEMBER, SIGMA_SIGN)))
            outs = [[O.decode(dims, member_theta(theta, k, sg), fc) for sg in (+1, -1)] for k in range(MEMBERS)]
            oseq = np.stack([np.stack([o[0] for o in pr]) for pr in outs])
            ofr = np.stack([np.stack([o[2] for o in pr]) for pr in outs])
        else:
            sigma = 0.0
            h = w['h']
            lw, lb = logit_rows(dims, theta)
            tok = w['tok'] if case != 'negative_logits' else int(L.greedy_pick(O.gemv(lw, lb, h))[0])
            G = plant_rows(lw, lb, h, ids, variant, tok)
            W, b = lw.copy(), lb.copy()
            seq, _, fr = O.decode(dims, theta, fc)
            oseq = np.broadcast_to(seq, (MEMBERS, 2) + seq.shape).copy()
            ofr = np.broadcast_to(fr, (MEMBERS, 2) + fr.shape).copy()
        return _freeze(dict(case=case, vocab=vocab, variant=variant, dims=dims, theta=theta, fc=fc, ids=ids, a=ids[0],
                            lead=ids[-1], sigma=sigma, G=G, h=h, W=W, b=b, oseq=oseq, ofr=ofr,
                            tsel=(SIGMA_MEMBER, 0 if SIGMA_SIGN > 0 else 1) if sigma else None))
    return once(('plant', case, vocab, variant), make)


def target_first(seq, tsel):
    """the first tokens of the target rows in seq [members, 2, B, T]: of every member and sign, or of tsel's"""
    s = seq[:, :, list(TARGET_ROWS), 0]
    return s if tsel is None else s[tsel[0], tsel[1]]


# ---------------------------------------------------------------------------------------------- positional ties
TIE_RAISE = 4.0


def tie_hh(pr, vocab):
    """pr's lane half: alternating at V = 999, the other one at V = 63"""
    return (pr & 1) if vocab == 999 else 1 - (pr & 1)


def tie_list():
    return [(pr, vocab) for vocab in (999, 63) for pr in range(16)]


def tie_ids(pr, vocab):
    """-> (twin, other): the twin at pair pr of its lane half. V = 999: the twin in stage 1 + pr % 3, the other copy in
    stage 9 at pair 15 - pr of the other half: the twin is the lower id and has its lane-stage to itself. V = 63 has one
    stage: the other copy is the twin + 4 (another lane: the same pair of half 1, or the next group of half 0), or
    the twin - 4 where + 4 leaves the vocabulary (then the twin is the higher id)."""
    hh = tie_hh(pr, vocab)
    if vocab == 999:
        return pair_id(1 + pr % 3, pr, hh), pair_id(9, 15 - pr, 1 - hh)
    twin = pair_id(0, pr, hh)
    return twin, (twin + 4 if twin + 4 <= vocab else twin - 4)


def tie_case(pr, vocab):
    """tok's logit row and bias, raised by TIE_RAISE, at the twin and at the other copy: bit-equal logits on every row
    of the batch; the lower id wins."""
    def make():
        w = world(vocab)
        dims, fc = w['dims'], w['fc']
        twin, other = tie_ids(pr, vocab)
        theta = w['theta'].copy()
        lw, lb = logit_rows(dims, theta)
        src_w, src_b = lw[w['tok']].copy(), F32(lb[w['tok']] + F32(TIE_RAISE))
        for v in (twin, other):
            lw[v] = src_w
            lb[v] = src_b
        seq, _, fr = O.decode(dims, theta, fc)
        return _freeze(dict(pr=pr, vocab=vocab, dims=dims, theta=theta, fc=fc, twin=twin, other=other,
                            pick=min(twin, other), h=w['h'], W=lw.copy(), b=lb.copy(), sigma=0.0, tsel=None,
                            oseq=np.broadcast_to(seq, (MEMBERS, 2) + seq.shape).copy(),
                            ofr=np.broadcast_to(fr, (MEMBERS, 2) + fr.shape).copy()))
    return once(('tie', pr, vocab), make)
