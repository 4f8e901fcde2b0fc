"""The worlds of the edge tests of the wide / layer-norm step-loop frame (wide_decode in csrc/decode_wide_kernels.hip
with its cells wide_cell and ln_cell): tests/test_wide_edges_host.py on the CPU, tests/test_gpu_wide_edges.py on the GPU.
TEST INFRASTRUCTURE ONLY. Everything is made from numpy PCG64 seeds and the CPU references, once per process, and never
modified afterwards.

The reference of a cell: oracle.decode for the plain cell ('plain'), tests/ln_ref.py for the layer-norm cell without
('ln') and with ('ln_affine') the six affine tensors behind theta. Step logits on the CPU come from ln_ref.Model, which
with layer_n=False is the oracle bit for bit (tests/test_layernorm_host.py).

Conventions. fin[b] is the index of row b's first end token (0 .. T - 1), T for a caption of full length; "finishes by
step s" is fin <= s. The frame works on ids in lanes, tiles and stages: lane half (id >> 2) & 1, 32-id tile id >> 5,
64-id stage id >> 6.

1. Tie worlds (TIE_WORLDS x TIE_CASES). Flat xavier logits (|z| < 2, lse = 4 .. 5.3), so that the log-softmax window
   (half an ulp of lse, 2^-22) is several logit ulps (2^-24 .. 2^-23) wide. `tok` is the first greedy token of row 0; a
   case copies tok's logit row to its twin ids and sets each twin's bias to bias[tok] + k * step. The chain of a logit
   starts at its bias, so k = 0 gives a bit-equal logit and a small k one a few ulps away.
2. Early-exit worlds (EXIT_WORLDS x EXIT_BATCHES). Decoding is row-independent: a pool of rows is decoded once with
   logit.bias[0] raised, and batches are put together from it by finishing step.
3. Full-slab worlds (FULL_WORLDS): the widest dims with valid rows in every 32-row group and every slab.
4. Vocabulary-edge worlds (vocab_world): V1 at and around whole 32-id tiles, random theta and theta with the last valid
   id planted as a winner."""
import numpy as np

from oracle import oracle as O
from tests import ln_ref as L

F, T = 128, 16
FRAGILE_CAP = 0.05
NOISE_SEED, TABLE_SEED, IT, SIGMA = 7, 123, 3, 0.01

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


# ---------------------------------------------------------------------------------------------- the references
def make_dims(E, R, V1):
    return O.Dims(vocab_size=V1 - 1, E=E, R=R, F=F, T=T)


def make_theta(cell, dims, seed, gain, bias_std):
    th = O.make_theta(dims, seed, gain, bias_std)
    return np.concatenate([th, L.make_tail(dims.R, 1500, 0.1)]) if cell == 'ln_affine' else th


def make_fc(rows, seed):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((rows, F)).astype(np.float32)


def decode(cell, dims, theta, fc):
    """(seq, lp, fragile) of the whole batch fc by the cell's reference"""
    if cell == 'plain':
        return O.decode(dims, theta, fc)
    return L.Model(dims, theta).decode(fc)


def step1_logits(cell, dims, theta, fc):
    """the logits [B, V1] of the first decode step (the image cell, then the cell on BOS)"""
    m = L.Model(dims, theta, layer_n=cell != 'plain')
    z = np.zeros((fc.shape[0], dims.R), np.float32)
    h, c = m.cell(m.product(m.Wimg, m.bimg, fc), z, z)
    h, c = m.cell(m.emb[np.zeros(fc.shape[0], np.int64)], h, c)
    return m.product(m.Wl, m.bl, h)


def first_end(seq):
    """fin: the index of each row's first end token, T for a caption of full length"""
    return np.where((seq == 0).any(1), (seq == 0).argmax(1), seq.shape[1])


def live(seq):
    """the steps at which a row has not yet emitted its end token"""
    return np.concatenate([np.ones((len(seq), 1), bool), seq[:, :-1] > 0], 1)


def fragile_rows(*fr):
    return np.concatenate([f.any(-1).ravel() for f in fr])


def logit_rows(dims, theta):
    """writable views (weight [V1, R], bias [V1]) of the logit layer inside theta"""
    o = dims.offsets()
    V1, R = dims.V1, dims.R
    w0, b0 = o['logit.weight'][0], o['logit.bias'][0]
    return theta[w0:w0 + V1 * R].reshape(V1, R), theta[b0:b0 + V1]


def references(base, dims, seed=11):
    """(gts, df, n, scorer) around the captions `base` (the engine's batch and the CPU scorer)"""
    import nicnes.synthetic as S
    from oracle import cider_ref as CR
    gts, df, n = S.build_references(base, dims.vocab_size, seed=seed, df_sets=64, T=dims.T)
    return gts, df, n, CR.CiderDOracle(df, n)


# ---------------------------------------------------------------------------------------------- 1. tie worlds
TIE_V1, TIE_B = 200, 40
# step: the bias step of a near twin. Chosen by the preconditions of tests/test_wide_edges_host.py; the figures that
# chose them are in that file's docstring.
TIE_WORLDS = {
    'plain': dict(cell='plain', E=256, R=384, seed=0, fc_seed=140, step=2.0 ** -25, near=2, triple=(2, 4)),
    'ln': dict(cell='ln_affine', E=128, R=256, seed=10, fc_seed=140, step=2.0 ** -24, near=2, triple=(1, 3)),
}
# case -> (the multiples k of the step for its twins: 0, the world's near (+-) or its triple; near: the raw argmax must
# differ from the pick)
TIE_CASES = {
    'exact_lower_other_half': ('exact', False),
    'exact_other_tile': ('exact', False),
    'exact_other_stage': ('exact', False),
    'near_lower': ('lower', True),
    'near_higher_same_half': ('higher', True),
    'triple_same_half': ('triple', True),
    'exact_end_token': ('exact', False),
    'last_id': ('higher', True),
}


def tie_steps(world, case):
    w = TIE_WORLDS[world]
    return {'exact': (0,), 'lower': (-w['near'],), 'higher': (w['near'],), 'triple': w['triple']}[TIE_CASES[case][0]]


def lane_half(v):
    return (v >> 2) & 1


def tie_world(world):
    """the unedited world: theta, fc, tok and the rows whose first token is tok"""
    def make():
        w = TIE_WORLDS[world]
        dims = make_dims(w['E'], w['R'], TIE_V1)
        theta = make_theta(w['cell'], dims, w['seed'], 1.0, 0.0)
        fc = make_fc(TIE_B, w['fc_seed'])
        z1 = step1_logits(w['cell'], dims, theta, fc)
        first = np.array([L.greedy_pick(z)[0] for z in z1])
        tok = int(first[0])
        return _freeze(dict(cell=w['cell'], dims=dims, theta=theta, fc=fc, z1=z1, tok=tok,
                            rows=np.flatnonzero(first == tok), step=np.float32(w['step'])))
    return once(('tie', world), make)


def tie_plan(case, tok, V1):
    """-> (twin ids, pick): the ids relative to tok, with a fallback in the other direction where there is one"""
    def either(a, b):
        return a if 0 < a < V1 - 1 else b
    if case == 'exact_lower_other_half':
        tw = [either(tok - 4, tok + 4)]
    elif case == 'exact_other_tile':
        tw = [tok ^ 32]                            # +- 32 inside tok's 64-id stage: the P0 / P1 of one epilogue
    elif case == 'exact_other_stage':
        tw = [either(tok + 64, tok - 64)]
    elif case == 'near_lower':
        tw = [either(tok - 8, tok - 1)]
    elif case == 'near_higher_same_half':
        tw = [tok + 8]
    elif case == 'triple_same_half':
        tw = [tok + 8, tok + 16]
    elif case == 'exact_end_token':
        tw = [0]
    elif case == 'last_id':
        tw = [V1 - 1]
    else:
        raise KeyError(case)
    assert all(0 <= v < V1 and v != tok for v in tw), (case, tok, tw, 'change the seed')
    assert case == 'exact_end_token' or min(tw) > 0, (case, tok, tw, 'change the seed')
    if case in ('near_higher_same_half', 'triple_same_half', 'last_id'):
        pick = tok
    else:
        pick = min(tw + [tok])
    return tw, pick


def tie_case(world, case):
    """a planted world: the edited theta, the twins, the pick, its step-1 logits and its reference decode"""
    def make():
        tw_ = tie_world(world)
        dims, tok = tw_['dims'], tw_['tok']
        ks, near = tie_steps(world, case), TIE_CASES[case][1]
        twins, pick = tie_plan(case, tok, dims.V1)
        theta = tw_['theta'].copy()
        lw, lb = logit_rows(dims, theta)
        for v, k in zip(twins, ks):
            lw[v] = lw[tok]
            lb[v] = lb[tok] + np.float32(k) * tw_['step']
        z1 = step1_logits(tw_['cell'], dims, theta, tw_['fc'])
        seq, lp, fr = decode(tw_['cell'], dims, theta, tw_['fc'])
        return _freeze(dict(cell=tw_['cell'], dims=dims, theta=theta, fc=tw_['fc'], tok=tok, rows=tw_['rows'],
                            twins=twins, pick=pick, near=near, z1=z1, seq=seq, lp=lp, fr=fr))
    return once(('tie', world, case), make)


def check_tie_case(world, case):
    """The CPU preconditions of a planted case; returns, per row whose first token was tok, the distances of the twins'
    logits from tok's in ulps of tok's logit."""
    c = tie_case(world, case)
    tok, twins, pick, rows, z1 = c['tok'], c['twins'], c['pick'], c['rows'], c['z1']
    V1 = c['dims'].V1
    assert len(rows) >= 2, 'fewer than two rows start with tok: change the seed'
    if case == 'exact_lower_other_half':
        assert lane_half(twins[0]) != lane_half(tok)
    elif case == 'exact_other_tile':
        assert twins[0] >> 6 == tok >> 6 and twins[0] >> 5 != tok >> 5
    elif case == 'exact_other_stage':
        assert twins[0] >> 6 != tok >> 6
    elif case == 'near_lower':
        assert twins[0] < tok
    elif case in ('near_higher_same_half', 'triple_same_half'):
        assert all(lane_half(v) == lane_half(tok) and v > tok for v in twins)
    elif case == 'last_id':
        assert twins[0] == V1 - 1 and (V1 - 1) >> 5 == (V1 + 31) // 32 - 1 and V1 % 32 != 0
    ulps = []
    for b in rows:
        z = z1[b]
        got, _, fragile = L.greedy_pick(z)
        assert got == pick and fragile == 0, (world, case, int(b), got, pick, fragile)
        u = np.spacing(np.abs(z[tok]))
        d = [float((z[v].astype(np.float64) - z[tok].astype(np.float64)) / u) for v in twins]
        ulps.append(d)
        if c['near']:
            assert int(np.argmax(z)) != pick, (world, case, int(b))
            assert all(x != 0 for x in d)
            if case == 'near_lower':
                assert d[0] < 0 and int(np.argmax(z)) == tok
            else:
                assert 0 < d[0] and all(d[i] < d[i + 1] for i in range(len(d) - 1))
                assert int(np.argmax(z)) == twins[-1]
        else:
            assert all(x == 0 for x in d), (world, case, d)
        # the planted pick is what the reference's decode took
        assert c['seq'][b, 0] == pick
        if case == 'exact_end_token':
            assert (c['seq'][b] == 0).all()
    frag = fragile_rows(c['fr'])
    assert frag.mean() <= FRAGILE_CAP, 'too many fragile rows (%d of %d): change the seed, not the cap' % (
        frag.sum(), frag.size)
    return ulps


# ---------------------------------------------------------------------------------------------- 2. early exits
EXIT_V1 = 68
# raise_: what logit.bias[0] is raised by; pool: the rows decoded once. Chosen by the preconditions; the histograms of
# finishing steps they give are in the docstring of tests/test_wide_edges_host.py.
EXIT_WORLDS = {
    'plain': dict(cell='plain', E=256, R=128, raise_=2.5, pool=600),
    'ln': dict(cell='ln_affine', E=128, R=256, raise_=2.5, pool=600),
}
EXIT_BATCHES = {'late_then_early': 130, 'early_then_late': 130, 'all_early': 257}


def exit_pool(world):
    def make():
        w = EXIT_WORLDS[world]
        dims = make_dims(w['E'], w['R'], EXIT_V1)
        theta = make_theta(w['cell'], dims, 8, 4.0, 0.1)
        theta[dims.offsets()['logit.bias'][0]] += np.float32(w['raise_'])
        fc = make_fc(w['pool'], 55)
        seq, _, fr = decode(w['cell'], dims, theta, fc)
        return _freeze(dict(cell=w['cell'], dims=dims, theta=theta, fc=fc, seq=seq, fin=first_end(seq),
                            ok=~fr.any(1)))
    return once(('exit', world), make)


def exit_rows(world, batch):
    """the pool rows of a batch, in batch order (every row once, none fragile)"""
    p = exit_pool(world)
    fin, ok = p['fin'], p['ok']
    idx = np.arange(len(fin))

    def take(mask, n, used=()):
        got = [int(i) for i in idx[mask & ok] if int(i) not in used][:n]
        assert len(got) == n, (world, batch, 'the pool is too small: %d of %d' % (len(got), n))
        return got
    if batch == 'late_then_early':
        tail = take(fin <= 3, 2)
        full = take(fin == T, 1)
        rest = take(fin >= 0, 127, set(tail + full))
        return np.array(rest[:5] + full + rest[5:] + tail)
    if batch == 'early_then_late':
        slab0 = take(fin <= 4, 128)
        return np.array(slab0 + take(fin == T, 1) + take(fin <= 4, 1, set(slab0)))
    if batch == 'all_early':
        wave = take(fin == 1, 32)
        run = take((fin >= 2) & (fin <= 6), 65)                    # the wave's neighbours and the tail slab's one row
        rest = take(fin <= 6, 160, set(wave + run))
        return np.array(rest[:32] + run[:32] + wave + run[32:64] + rest[32:] + run[64:])
    raise KeyError(batch)


def exit_batch(world, batch):
    """a batch and the reference's decode of it as a whole (its lp rule is the whole batch's)"""
    def make():
        p = exit_pool(world)
        rows = exit_rows(world, batch)
        fc = np.ascontiguousarray(p['fc'][rows])
        seq, lp, fr = decode(p['cell'], p['dims'], p['theta'], fc)
        return _freeze(dict(cell=p['cell'], dims=p['dims'], theta=p['theta'], fc=fc, rows=rows, seq=seq, lp=lp, fr=fr,
                            fin=first_end(seq)))
    return once(('exit', world, batch), make)


def check_exit_batch(world, batch):
    """The CPU preconditions of a batch: the finishing steps that define it, on the whole-batch decode."""
    p, b = exit_pool(world), exit_batch(world, batch)
    fin, B = b['fin'], EXIT_BATCHES[batch]
    assert len(fin) == B and len(set(b['rows'].tolist())) == B
    assert np.array_equal(b['seq'], p['seq'][b['rows']])           # decoding is row-independent
    assert not b['fr'].any()
    if batch == 'late_then_early':
        assert fin[:128].max() == T and fin[128:].max() <= 3
        assert (b['lp'] != 0).all()                                # the batch never finishes: a log-prob at every step
    elif batch == 'early_then_late':
        assert fin[:128].max() <= 4 and fin[128:].max() == T
        assert (b['lp'] != 0).all()
    else:
        assert fin.max() <= 6 and fin.max() < T - 1
        assert (fin[64:96] == 1).all() and fin[32:64].min() >= 2 and fin[96:128].min() >= 2
        assert fin[32:64].max() >= 4 and fin[96:128].max() >= 4   # the neighbours run on
        assert fin[128:256].max() >= 4 and fin[256] >= 2           # three slabs, the tail's one row among them
        assert (b['lp'][:, :fin.max() + 1] != 0).all() and (b['lp'][:, fin.max() + 1:] == 0).all()
    return np.bincount(fin, minlength=T + 1)


# ---------------------------------------------------------------------------------------------- 3. full slabs
FULL_NOISE_LEN = 1 << 23
FULL_WORLDS = {
    'plain_512_512': dict(cell='plain', E=512, R=512, B=257),
    'ln_affine_512_512': dict(cell='ln_affine', E=512, R=512, B=130),
    'ln_256_384': dict(cell='ln', E=256, R=384, B=128),
}


def noise_table(n):
    return once(('table', n), lambda: O.noise_table(n, TABLE_SEED))


def full_world(world):
    """theta itself and member 0 of both signs on a batch that fills every row group of its slabs"""
    def make():
        w = FULL_WORLDS[world]
        dims = make_dims(w['E'], w['R'], 68)
        theta = make_theta(w['cell'], dims, 0, 4.0, 0.1)
        fc = make_fc(w['B'], 300 + w['B'])
        base, blp, bfr = decode(w['cell'], dims, theta, fc)
        idx = O.noise_index(NOISE_SEED, IT, 0, FULL_NOISE_LEN, theta.size)
        outs = [decode(w['cell'], dims, O.perturb(theta, noise_table(FULL_NOISE_LEN), idx, SIGMA, sign), fc)
                for sign in (+1, -1)]
        oseq, olp, ofr = (np.stack([o[i] for o in outs]) for i in range(3))
        return _freeze(dict(cell=w['cell'], dims=dims, theta=theta, fc=fc, base=base, blp=blp, bfr=bfr, idx=idx,
                            oseq=oseq, olp=olp, ofr=ofr))
    return once(('full', world), make)


# ---------------------------------------------------------------------------------------------- 4. vocabulary edges
VOCAB_B = 40
VOCAB_WORLDS = [('plain', 256, 256, V1) for V1 in (32, 64, 96, 100, 128)] + [('ln', 128, 128, V1) for V1 in (32, 96)]
LAST_ID_RAISE = 0.5


def vocab_world(cell, E, R, V1, planted):
    """random theta, or that theta with tok's logit row copied to the last valid id and its bias raised"""
    def make():
        dims = make_dims(E, R, V1)
        theta = make_theta(cell, dims, 0, 4.0, 0.1)
        fc = make_fc(VOCAB_B, 100 + VOCAB_B)
        tok = -1
        if planted:
            tok = int(decode(cell, dims, theta, fc[:1])[0][0, 0])
            assert 0 < tok < V1 - 1, (tok, 'change the seed')
            lw, lb = logit_rows(dims, theta)
            lw[V1 - 1] = lw[tok]
            lb[V1 - 1] = lb[tok] + np.float32(LAST_ID_RAISE)
        seq, lp, fr = decode(cell, dims, theta, fc)
        return _freeze(dict(cell=cell, dims=dims, theta=theta, fc=fc, tok=tok, seq=seq, lp=lp, fr=fr))
    return once(('vocab', cell, E, R, V1, planted), make)


def check_vocab_world(cell, E, R, V1, planted):
    w = vocab_world(cell, E, R, V1, planted)
    frag = fragile_rows(w['fr'])
    assert frag.mean() <= FRAGILE_CAP, 'too many fragile rows (%d of %d): change the seed, not the cap' % (
        frag.sum(), frag.size)
    assert w['seq'].max() <= V1 - 1
    wins = int((w['seq'] == V1 - 1).any(1).sum())
    if planted:
        assert w['seq'][0, 0] == V1 - 1 and not w['fr'][0, 0]      # the last valid id wins where tok did
        assert wins >= 2, 'the last id wins on %d rows: change the seed' % wins
        assert not (w['seq'] == w['tok']).any()                    # and tok, 0.5 below its copy, never again
    return wins
