"""GPU: the step-loop frame of the wide and layer-norm decodes (wide_decode in csrc/decode_wide_kernels.hip, cells
wide_cell and ln_cell) where tests/test_gpu_wide.py and tests/test_gpu_layernorm.py reach it only by accident: its own
copy of the greedy token rule, of the finished mask and the slab exit, and of the row-validity test that drives the lane
scratch. The worlds and their CPU preconditions are tests/wide_edge_worlds.py (the preconditions alone:
tests/test_wide_edges_host.py); every test repeats its preconditions before it touches the GPU. References: oracle.decode
for the plain cell, tests/ln_ref.py for the layer-norm cell. The suite's bars and nothing else: tokens exact up to a
row's first fragile step, log-probs 1e-5 on the live steps of non-fragile rows, fitness 1e-9 against
cider_ref.rollout_fitness, at most 5 % fragile rows per world, identical bits from two runs.

1. Planted ties, no hook set: plain (256, 384) and ln affine (128, 256), V1 = 200 (three full stages, one of 8 ids and an
   empty tile), exact and near twins of row 0's first token in the other lane half, the other tile of a stage, another
   stage, at the end token and at the last valid id; a triple that evicts the pick from the records, which the frame
   must notice by itself (tie_fallbacks rises). A handle with NICNES_FORCE_EXACT=1 gives the same bits.
2. Early exits by construction, plain (256, 128) and ln affine (128, 256): a slab that ends at step 3 beside one that
   runs to T, in both orders (B = 130); a batch that ends at step 6 (B = 257: three slabs, a 1-row tail, a whole 32-row
   group that ends at step 1). Log-probs of every row up to the batch's last finishing step, exact zeros after it, through
   evaluate and through evaluate_theta (B = 257 is odd: sign - has one row fewer).
3. Full slabs at the widest dims: plain (512, 512) B = 257, ln affine (512, 512) B = 130, ln (256, 384) B = 128; theta
   itself and one member of both signs.
4. Vocabulary tile edges: plain (256, 256) at V1 = 32, 64, 96, 100, 128 and ln (128, 128) at V1 = 32, 96, random theta
   and theta whose last valid id wins; the same bits with the exact sweep forced."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from oracle import cider_ref as CR                              # noqa: E402
from tests import wide_edge_worlds as W                         # noqa: E402
from tests.test_gpu_parity import _compare_tokens               # noqa: E402

NOISE_LEN = 1 << 21                                # no member is perturbed (sigma = 0) outside the full-slab worlds
IT = W.IT
COUNTERS = ('tie_fallbacks', 'sample_stage_fallbacks', 'coop_timeouts', 'sample_slot_timeouts', 'screen_candidates',
            'screen_fallback_rows', 'queue_timeouts')
FORCED = (('NICNES_FORCE_EXACT', '1'),)


def _engine(cell, dims, max_batch, env=(), noise_len=NOISE_LEN):
    import nicnes
    mp = pytest.MonkeyPatch()
    for k, v in env:
        mp.setenv(k, v)
    try:
        e = nicnes.Engine(vocab_size=dims.vocab_size, input_encoding_size=dims.E, rnn_size=dims.R, fc_feat_size=dims.F,
                          seq_length=dims.T, max_batch=max_batch, max_members=2, noise_len=noise_len,
                          noise_seed=W.NOISE_SEED, layer_n=cell != 'plain', layer_n_affine=cell == 'ln_affine')
    finally:
        mp.undo()
    e.set_noise_table(W.noise_table(noise_len))
    assert e.D == dims.D + (22 * dims.R if cell == 'ln_affine' else 0)
    assert e.decode_path(max_batch, 1) == ('wide' if cell == 'plain' else 'ln')
    return e


@pytest.fixture(scope='module')
def engines():
    """handles by key, made on first use and closed with the module"""
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    made = {}

    def get(key, cell, dims, max_batch, env=(), noise_len=NOISE_LEN):
        if key not in made:
            made[key] = _engine(cell, dims, max_batch, env, noise_len)
        return made[key]
    yield get
    for e in made.values():
        e.close()


def _refs(key, base, dims):
    return W.once(('refs',) + key, lambda: W.references(base, dims))


def _load(e, theta, fc, refs):
    import nicnes
    gts, df, n, _ = refs
    e.set_theta(theta)
    keys, vals = nicnes.df_table_arrays(df)
    e.set_df_table(keys, vals, np.log(float(n)))
    e.set_batch(fc, gts)


def _np(out):
    return [x.cpu().numpy() for x in out]


def _bits(a):
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _check_rollout(got_seq, got_lp, got_fit, seq, lp, fr, refs, what):
    """one rollout [B, T] under the suite's bars"""
    assert _compare_tokens(got_seq, seq, fr) == 0, what
    keep = ~fr.any(1)
    m = W.live(seq) & keep[:, None]
    err = np.abs(got_lp[m] - lp[m]).max()
    print(what, 'max log-prob error on live steps %.3g' % err)
    assert np.isfinite(got_lp).all() and (got_lp <= 0).all(), what
    assert err <= 1e-5, (what, err)
    f_ref, _ = CR.rollout_fitness(refs[3], got_seq, refs[0])
    assert abs(got_fit - f_ref) <= 1e-9 * max(1.0, abs(f_ref)), (what, got_fit, f_ref)


def _moved(before, after, keys=COUNTERS):
    return {k: after[k] - before[k] for k in keys if after[k] != before[k]}


# ------------------------------------------------------------------------------------------------ 1. planted ties
@pytest.mark.parametrize('case', list(W.TIE_CASES))
@pytest.mark.parametrize('world', list(W.TIE_WORLDS))
def test_planted_ties_follow_the_reference_unforced(engines, world, case):
    W.check_tie_case(world, case)                  # the preconditions (tests/test_wide_edges_host.py)
    c = W.tie_case(world, case)
    dims, rows, pick = c['dims'], c['rows'], c['pick']
    refs = _refs(('tie', world, case), c['seq'], dims)
    e = engines(('tie', world), c['cell'], dims, W.TIE_B)
    forced = engines(('tie', world, 'forced'), c['cell'], dims, W.TIE_B, FORCED)
    _load(e, c['theta'], c['fc'], refs)
    s0 = e.stats()
    fit, seq, lp = _np(e.evaluate(IT, 0, 1, 0.0, return_seq=True, return_lp=True))     # sigma 0: both signs decode theta
    s1 = e.stats()
    assert seq.shape == (1, 2, W.TIE_B, W.T)
    assert (seq[0, 0][rows, 0] == pick).all(), (world, case, seq[0, 0][rows, 0].tolist(), pick)
    _check_rollout(seq[0, 0], lp[0, 0], fit[0, 0], c['seq'], c['lp'], c['fr'], refs, (world, case))
    assert np.array_equal(seq[0, 1], seq[0, 0]) and np.array_equal(_bits(lp[0, 1]), _bits(lp[0, 0]))
    assert _bits(fit)[0, 0] == _bits(fit)[0, 1]
    if case == 'exact_end_token':
        assert (seq[0, 0][rows] == 0).all() and (seq[0, 0] != 0).any()
    if case == 'triple_same_half':
        # three records of one lane half in the window evict tok: only the exact sweep finds it, and nothing asked for it
        assert s1['tie_fallbacks'] > s0['tie_fallbacks'], (s0, s1)
    assert not _moved(s0, s1, [k for k in COUNTERS if k != 'tie_fallbacks']), (s0, s1)
    # the greedy-only decode, and a second run of each: the same bits
    fit_n, seq_n = _np(e.evaluate(IT, 0, 1, 0.0, return_seq=True))
    fit_2, seq_2, lp_2 = _np(e.evaluate(IT, 0, 1, 0.0, return_seq=True, return_lp=True))
    assert np.array_equal(seq_n, seq) and np.array_equal(_bits(fit_n), _bits(fit))
    assert np.array_equal(seq_2, seq) and np.array_equal(_bits(fit_2), _bits(fit)) and np.array_equal(_bits(lp_2), _bits(lp))
    # the exact sweep on every step
    _load(forced, c['theta'], c['fc'], refs)
    f0 = forced.stats()
    fit_f, seq_f, lp_f = _np(forced.evaluate(IT, 0, 1, 0.0, return_seq=True, return_lp=True))
    assert forced.stats()['tie_fallbacks'] > f0['tie_fallbacks']
    assert np.array_equal(seq_f, seq) and np.array_equal(_bits(fit_f), _bits(fit)) and np.array_equal(_bits(lp_f), _bits(lp))


# ------------------------------------------------------------------------------------------------ 2. early exits
def _check_batch_lp(got_lp, b, what):
    """log-probs of every row, finished or not, up to the batch's last finishing step; exact zeros after it"""
    last = int(b['fin'].max())                     # the index of that step; T when a caption has full length
    err = np.abs(got_lp[:, :last + 1] - b['lp'][:, :last + 1]).max()
    print(what, 'last finishing step', last, 'max log-prob error %.3g' % err)
    assert err <= 1e-5, (what, err)
    assert (got_lp[:, :last + 1] <= 0).all(), what
    assert (got_lp[:, last + 1:] == 0).all() and (b['lp'][:, last + 1:] == 0).all(), what


@pytest.mark.parametrize('batch', list(W.EXIT_BATCHES))
@pytest.mark.parametrize('world', list(W.EXIT_WORLDS))
def test_early_exits_match_the_reference(engines, world, batch):
    W.check_exit_batch(world, batch)               # the finishing steps that define the batch
    b = W.exit_batch(world, batch)
    dims, B, fin = b['dims'], W.EXIT_BATCHES[batch], b['fin']
    if batch == 'all_early':
        assert fin.max() < W.T - 1                 # so the zeros behind the last finishing step are there to check
    refs = _refs(('exit', world, batch), b['seq'], dims)
    e = engines(('exit', world, B), b['cell'], dims, B)
    _load(e, b['theta'], b['fc'], refs)
    assert e.decode_shape(B, 1) == (4, (B + 127) // 128, 1)
    s0 = e.stats()
    fit_n, seq_n = _np(e.evaluate(IT, 0, 1, 0.0, return_seq=True))
    fit, seq, lp = _np(e.evaluate(IT, 0, 1, 0.0, return_seq=True, return_lp=True))
    assert np.array_equal(seq_n, seq) and np.array_equal(_bits(fit_n), _bits(fit))     # running on to T changes no token
    f_ref, _ = CR.rollout_fitness(refs[3], b['seq'], refs[0])
    for s in range(2):
        assert np.array_equal(seq[0, s], b['seq']), (world, batch, s)                  # no row of the batch is fragile
        _check_batch_lp(lp[0, s], b, (world, batch, 'sign', s))
        assert abs(fit[0, s] - f_ref) <= 1e-9 * max(1.0, abs(f_ref)), (s, fit[0, s], f_ref)
    # theta itself: sign + decodes the first ceil(B / 2) rows, sign - the rest; the two halves are one rollout
    f1_n, seq1_n = _np(e.evaluate_theta(0, return_seq=True))
    f1, seq1, lp1 = _np(e.evaluate_theta(0, return_seq=True, return_lp=True))
    assert seq1.shape == (B, W.T)
    assert np.array_equal(seq1, b['seq']) and np.array_equal(seq1_n, b['seq'])
    _check_batch_lp(lp1, b, (world, batch, 'theta'))
    for f in (f1[0], f1_n[0]):
        assert abs(f - f_ref) <= 1e-9 * max(1.0, abs(f_ref)), (f, f_ref)
    assert not _moved(s0, e.stats()), (s0, e.stats())


# ------------------------------------------------------------------------------------------------ 3. full slabs
@pytest.mark.parametrize('world', list(W.FULL_WORLDS))
def test_full_slabs_at_the_widest_dims(engines, world):
    w = W.full_world(world)
    dims, B = w['dims'], W.FULL_WORLDS[world]['B']
    frag = W.fragile_rows(w['bfr'], w['ofr'])
    assert frag.mean() <= W.FRAGILE_CAP, 'too many fragile rows (%d of %d): change the seed, not the cap' % (
        frag.sum(), frag.size)
    refs = _refs(('full', world), w['base'], dims)
    e = engines(('full', world), w['cell'], dims, B, noise_len=W.FULL_NOISE_LEN)
    _load(e, w['theta'], w['fc'], refs)
    assert e.decode_shape(B, 1) == (4, (B + 127) // 128, 1)
    assert int(e.noise_indices(IT, 0, 1).cpu().numpy()[0]) == w['idx']
    s0 = e.stats()
    f0, seq0, lp0 = _np(e.evaluate_theta(0, return_seq=True, return_lp=True))
    _check_rollout(seq0, lp0, f0[0], w['base'], w['blp'], w['bfr'], refs, (world, 'theta'))
    fit, seq, lp = _np(e.evaluate(IT, 0, 1, W.SIGMA, return_seq=True, return_lp=True))
    for s in range(2):
        _check_rollout(seq[0, s], lp[0, s], fit[0, s], w['oseq'][s], w['olp'][s], w['ofr'][s], refs, (world, 'sign', s))
    assert fit.max() > 0.0
    fit_n, seq_n = _np(e.evaluate(IT, 0, 1, W.SIGMA, return_seq=True))
    assert np.array_equal(seq_n, seq) and np.array_equal(_bits(fit_n), _bits(fit))
    # identical bits from a second run of each
    f0_2, seq0_2, lp0_2 = _np(e.evaluate_theta(0, return_seq=True, return_lp=True))
    fit_2, seq_2, lp_2 = _np(e.evaluate(IT, 0, 1, W.SIGMA, return_seq=True, return_lp=True))
    assert np.array_equal(seq0_2, seq0) and np.array_equal(_bits(lp0_2), _bits(lp0)) and np.array_equal(_bits(f0_2), _bits(f0))
    assert np.array_equal(seq_2, seq) and np.array_equal(_bits(lp_2), _bits(lp)) and np.array_equal(_bits(fit_2), _bits(fit))
    assert not _moved(s0, e.stats()), (s0, e.stats())
    assert not e.last_decode_bounded()


# ------------------------------------------------------------------------------------------------ 4. vocabulary edges
@pytest.mark.parametrize('planted', [False, True], ids=['random', 'last_id'])
@pytest.mark.parametrize('cell,E,R,V1', W.VOCAB_WORLDS, ids=['%s_V%d' % (c[0], c[3]) for c in W.VOCAB_WORLDS])
def test_vocabulary_tile_edges(engines, cell, E, R, V1, planted):
    W.check_vocab_world(cell, E, R, V1, planted)   # the fragile cap, and the last id's win where it is planted
    w = W.vocab_world(cell, E, R, V1, planted)
    dims, B = w['dims'], W.VOCAB_B
    refs = _refs(('vocab', cell, V1, planted), w['seq'], dims)
    e = engines(('vocab', cell, V1), cell, dims, B)
    forced = engines(('vocab', cell, V1, 'forced'), cell, dims, B, FORCED)
    _load(e, w['theta'], w['fc'], refs)
    s0 = e.stats()
    fit, seq, lp = _np(e.evaluate(IT, 0, 1, 0.0, return_seq=True, return_lp=True))
    assert seq.max() <= V1 - 1 and seq.min() >= 0
    _check_rollout(seq[0, 0], lp[0, 0], fit[0, 0], w['seq'], w['lp'], w['fr'], refs, (cell, V1, planted))
    assert np.array_equal(seq[0, 1], seq[0, 0]) and np.array_equal(_bits(lp[0, 1]), _bits(lp[0, 0]))
    if planted:
        assert seq[0, 0][0, 0] == V1 - 1
    assert not _moved(s0, e.stats()), (s0, e.stats())
    fit_n, seq_n = _np(e.evaluate(IT, 0, 1, 0.0, return_seq=True))
    assert np.array_equal(seq_n, seq) and np.array_equal(_bits(fit_n), _bits(fit))
    _load(forced, w['theta'], w['fc'], refs)
    f0 = forced.stats()
    fit_f, seq_f, lp_f = _np(forced.evaluate(IT, 0, 1, 0.0, return_seq=True, return_lp=True))
    assert forced.stats()['tie_fallbacks'] > f0['tie_fallbacks']
    assert np.array_equal(seq_f, seq) and np.array_equal(_bits(fit_f), _bits(fit)) and np.array_equal(_bits(lp_f), _bits(lp))
