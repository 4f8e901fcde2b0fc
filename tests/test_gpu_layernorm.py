"""GPU: the layer-norm greedy decode (csrc/decode_ln_kernels.hip), layer_n models at every supported width, behind the
C ABI. The reference on this side is tests/ln_ref.py, the numpy restatement that tests/test_layernorm_host.py pins to
the C oracle (normalisation off: bit for bit) and to the imported reference (tests/golden/decode_layernorm.npz).

1. One LN cell through nicnes_test_ln_cell (the decode's own device function), bitwise against ln_ref, rows = 1, 33, 128,
   (E, R) = (128, 128) and (256, 384), affine off and on: random rows, and planted ones (all-equal pre-activations from
   zero weights and a constant bias, so var = 0; a bias offset of 1e4 on one chain; gamma = 0 on one gate block; a row
   whose c' is constant).
2. Decode parity against ln_ref: theta itself and two members of both signs per case; tokens exact up to the first step
   ln_ref marks fragile, at most 5 % of the rows fragile, log-probs to 1e-5 (the bar of tests/test_gpu_wide.py), fitness
   1e-9; identical bits from two runs; no counter of stats() raised.
     case  E    R    V1    F     T   B    affine
     a     128  128  68    128   16  40   off
     b     128  256  8     128   3   40   on
     c     384  128  68    256   16  8    on
     d     512  512  68    128   16  8    off
     e     128  128  9488  2048  16  130  on        (two slabs, a 2-row tail)
3. NICNES_FORCE_EXACT=1 gives the unforced bits (case a); a neutral tail (gamma = 1, beta = 0) gives the bits of a
   handle without affine (an internal consistency check only); the tail is perturbed (an SM-VECTOR evaluate that blows
   the tail's noise up a thousandfold changes tokens, as ln_ref on theta +- delta' says: a kernel that read gamma and
   beta from theta alone would fail it).
4. The remaining paths at (128, 256) affine: evaluate_theta, Split.decode / evaluate, per-member batches, the four
   greedy_* criteria, SM-PROPORTIONAL (the tail's beta = 0 entries take the mean), grad_partial / Adam / SGD at the affine
   D, two EngineMaster.run iterations with a Validator that move the tail and reload their snapshot, every refusal with
   the handle usable afterwards, decode_path() == 'ln'.
5. The entries on a layer_n_affine experiment: a `python -m nicnes.worker` process serving two dispatched iterations, and
   python -m nicnes.evaluate's main on a .pth that carries the six tail tensors."""
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from oracle import oracle as O                                  # noqa: E402
from oracle import cider_ref as CR                              # noqa: E402
from tests import ln_ref as L                                   # noqa: E402
from tests.test_gpu_parity import _compare_tokens               # noqa: E402

NOISE_LEN = 1 << 23
SEED = 7
SIGMA = 0.01
IT = 3
P = 2
FRAGILE_CAP = 0.05

CASES = {
    'a': dict(E=128, R=128, vocab=67, F=128, T=16, B=40, affine=False),
    'b': dict(E=128, R=256, vocab=7, F=128, T=3, B=40, affine=True),
    'c': dict(E=384, R=128, vocab=67, F=256, T=16, B=8, affine=True),
    'd': dict(E=512, R=512, vocab=67, F=128, T=16, B=8, affine=False),
    'e': dict(E=128, R=128, vocab=9487, F=2048, T=16, B=130, affine=True),
}
FEATURE_CASE = 'f'                                 # the engine's other paths: two k windows in the h2h / logit products
CASES[FEATURE_CASE] = dict(E=128, R=256, vocab=67, F=128, T=16, B=40, affine=True)

_cache = {}


def _dims(c):
    return O.Dims(vocab_size=c['vocab'], E=c['E'], R=c['R'], F=c['F'], T=c.get('T', 16))


def _table(n=NOISE_LEN):
    if ('table', n) not in _cache:
        _cache['table', n] = O.noise_table(n, 123)
    return _cache['table', n]


def _idx(D, member, iteration=IT, n=NOISE_LEN):
    return O.noise_index(SEED, iteration, member, n, D)


def _theta(dims, affine, seed=0, tail_seed=1500):
    th = O.make_theta(dims, seed, 4.0, 0.1)
    return np.concatenate([th, L.make_tail(dims.R, tail_seed, 0.1)]) if affine else th


def _decode(dims, theta, fc):
    return L.Model(dims, theta).decode(fc)


def _world(case):
    """ln_ref's side of a case, computed once and never modified."""
    if ('world', case) not in _cache:
        import nicnes.synthetic as S
        c, dims, table = CASES[case], _dims(CASES[case]), _table()
        theta = _theta(dims, c['affine'])
        fc = np.random.Generator(np.random.PCG64(300 + c['B'])).standard_normal((c['B'], c['F'])).astype(np.float32)
        base, blp, bfr = _decode(dims, theta, fc)
        gts, df, n = S.build_references(base, dims.vocab_size, seed=11, df_sets=64, T=dims.T)
        B = c['B']
        oseq = np.zeros((P, 2, B, dims.T), np.int32)
        olp = np.zeros((P, 2, B, dims.T), np.float32)
        ofr = np.zeros((P, 2, B, dims.T), np.uint8)
        for k in range(P):
            for s, sign in enumerate((+1, -1)):
                oseq[k, s], olp[k, s], ofr[k, s] = _decode(dims, O.perturb(theta, table, _idx(theta.size, k), SIGMA, sign), fc)
        for a in (base, blp, bfr, oseq, olp, ofr, theta, fc):
            a.setflags(write=False)
        _cache['world', case] = dict(dims=dims, theta=theta, fc=fc, base=base, blp=blp, bfr=bfr, gts=gts, df=df, n=n,
                                     oseq=oseq, olp=olp, ofr=ofr, scorer=CR.CiderDOracle(df, n), affine=c['affine'])
    return _cache['world', case]


def _engine(dims, max_batch, affine, env=(), noise_len=NOISE_LEN, max_members=4, layer_n=True):
    import nicnes
    mp = pytest.MonkeyPatch()
    for k, v in env:
        mp.setenv(k, v)
    try:
        e = nicnes.Engine(vocab_size=dims.vocab_size, input_encoding_size=dims.E, rnn_size=dims.R, fc_feat_size=dims.F,
                          seq_length=dims.T, max_batch=max_batch, max_members=max_members, noise_len=noise_len,
                          noise_seed=SEED, layer_n=layer_n, layer_n_affine=affine)
    finally:
        mp.undo()
    e.set_noise_table(_table(noise_len))
    assert e.D == dims.D + (22 * dims.R if affine and layer_n else 0)
    return e


@pytest.fixture(scope='module')
def engines():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    made = {}

    def get(case):
        if case not in made:
            c = CASES[case]
            made[case] = _engine(_dims(c), c['B'], c['affine'])
        return made[case]
    yield get
    for e in made.values():
        e.close()


def _load(e, w):
    import nicnes
    e.set_theta(w['theta'])
    keys, vals = nicnes.df_table_arrays(w['df'])
    e.set_df_table(keys, vals, np.log(float(w['n'])))
    e.set_batch(w['fc'], w['gts'])


def _close(got, want, rel=1e-9):
    return abs(got - want) <= rel * max(1.0, abs(want))


def _live(seq):
    return np.concatenate([np.ones((len(seq), 1), bool), seq[:, :-1] > 0], 1)


COUNTERS = ('tie_fallbacks', 'sample_stage_fallbacks', 'coop_timeouts', 'sample_slot_timeouts', 'screen_candidates',
            'screen_fallback_rows', 'queue_timeouts')


# ------------------------------------------------------------------------------------------------ 1. the cell
CELL_DIMS = [(128, 128), (256, 384)]


@pytest.fixture(scope='module')
def cell_engines():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    made = {}

    def get(E, R, affine):
        if (E, R, affine) not in made:
            made[E, R, affine] = _engine(O.Dims(vocab_size=7, E=E, R=R, F=128), 8, affine, noise_len=1 << 21,
                                         max_members=1)
        return made[E, R, affine]
    yield get
    for e in made.values():
        e.close()


def _cell_check(e, dims, theta, x, h, c, what):
    e.set_theta(theta)
    hg, cg = e.test_ln_cell(x, h, c)
    hr, cr = L.Model(dims, theta).cell(x, h, c)
    assert np.array_equal(cg.view(np.uint32), cr.view(np.uint32)), (what, np.abs(cg - cr).max())
    assert np.array_equal(hg.view(np.uint32), hr.view(np.uint32)), (what, np.abs(hg - hr).max())
    return hg, cg


@pytest.mark.parametrize('affine', [False, True], ids=['plain', 'affine'])
@pytest.mark.parametrize('E,R', CELL_DIMS)
def test_ln_cell_bitwise_on_random_rows(cell_engines, E, R, affine):
    dims = O.Dims(vocab_size=7, E=E, R=R, F=128)
    e = cell_engines(E, R, affine)
    theta = _theta(dims, affine, seed=4, tail_seed=1600)
    rng = np.random.Generator(np.random.PCG64(E + R))
    for rows in (1, 33, 128):
        x = rng.standard_normal((rows, E)).astype(np.float32)
        h = np.tanh(rng.standard_normal((rows, R))).astype(np.float32)
        c = rng.standard_normal((rows, R)).astype(np.float32)
        hg, cg = _cell_check(e, dims, theta, x, h, c, rows)
        assert np.isfinite(hg).all() and np.unique(hg).size > rows * R // 2


@pytest.mark.parametrize('affine', [False, True], ids=['plain', 'affine'])
@pytest.mark.parametrize('E,R', CELL_DIMS)
def test_ln_cell_bitwise_on_planted_rows(cell_engines, E, R, affine):
    dims = O.Dims(vocab_size=7, E=E, R=R, F=128)
    e = cell_engines(E, R, affine)
    off = dims.offsets()
    rng = np.random.Generator(np.random.PCG64(7 * E + R))
    rows = 33
    x = rng.standard_normal((rows, E)).astype(np.float32)
    h = np.tanh(rng.standard_normal((rows, R))).astype(np.float32)
    c = rng.standard_normal((rows, R)).astype(np.float32)

    def span(name):
        o, shp = off[name]
        return slice(o, o + int(np.prod(shp)))
    tail = L.tail_offsets(dims)
    # (1) zero weights and a constant bias: every pre-activation of a chain equal, var = 0, y = 0 (then beta)
    th = _theta(dims, affine, seed=4, tail_seed=1600).copy()
    th[span('core.i2h.weight')] = 0
    th[span('core.h2h.weight')] = 0
    th[span('core.i2h.bias')] = 0.375
    th[span('core.h2h.bias')] = -1.25
    hg, cg = _cell_check(e, dims, th, x, h, c, 'constant')
    if not affine:                                 # s = 0: g = 0, c' = sigmoid(0) * c
        assert np.array_equal(cg, (O.vec_math('sigmoid', np.zeros(1, np.float32))[0] * c).astype(np.float32))
    # (4) with that theta and a constant c, c' is constant over the row when the gates are (no affine, or a constant
    # beta): LN_c sees var = 0 and h' = o * tanh(0 or beta_c)
    if affine:
        for i in (1, 3):
            th[tail[i]:tail[i + 1]] = 0.25         # beta of both chains constant: s constant over a gate's units
    cc = np.repeat(rng.standard_normal((rows, 1)).astype(np.float32), R, 1)
    hg, cg = _cell_check(e, dims, th, x, h, cc, 'constant c')
    assert (cg == cg[:, :1]).all()
    if not affine:
        # a lane's sequential sum of R / 2 copies of v is R / 2 * v only to R / 2 roundings of 2^-24 relative each, so
        # d = v - mean is at most that much of |v| and y = d / sqrt(0 + 1e-5); h' = o * tanh(y) is no larger
        bound = (R / 2) * 2.0 ** -24 * np.abs(cg).max() / np.sqrt(1e-5)
        assert np.abs(hg).max() <= bound
    # (2) a bias offset of 1e4 on one chain: the two-pass variance keeps the spread
    th = _theta(dims, affine, seed=4, tail_seed=1600).copy()
    th[span('core.i2h.bias')] += np.float32(1e4)
    hg, _ = _cell_check(e, dims, th, x, h, c, 'offset 1e4')
    assert np.isfinite(hg).all() and np.unique(hg).size > rows * R // 2
    # (3) gamma = 0 on one gate block (the f gate's first 32 units, both chains): that block's s is beta_i + beta_h
    if affine:
        th = _theta(dims, affine, seed=4, tail_seed=1600).copy()
        th[tail[0] + R:tail[0] + R + 32] = 0
        th[tail[2] + R:tail[2] + R + 32] = 0
        _cell_check(e, dims, th, x, h, c, 'gamma 0')


# ------------------------------------------------------------------------------------------------ 2. parity
@pytest.mark.parametrize('case', ['a', 'b', 'c', 'd', 'e'])
def test_ln_parity_against_ln_ref(engines, case):
    w = _world(case)
    c = CASES[case]
    dims, B, T = w['dims'], c['B'], c['T']
    oseq, olp, ofr = w['oseq'], w['olp'], w['ofr']
    frag_rows = np.concatenate([ofr.any(-1).ravel(), w['bfr'].any(-1)])
    assert frag_rows.mean() <= FRAGILE_CAP, 'too many fragile rows (%d of %d): change the fc seed, not the cap' % (
        frag_rows.sum(), frag_rows.size)
    assert np.unique(oseq).size >= min(c['vocab'], 12)
    e = engines(case)
    _load(e, w)
    assert e.decode_path(B, P) == 'ln' and e.decode_shape(B, P) == (4, (B + 127) // 128, 1)
    assert [int(i) for i in e.noise_indices(IT, 0, P).cpu().numpy()] == [_idx(e.D, k) for k in range(P)]
    before = e.stats()
    # theta itself
    f0, seq0, lp0 = [x.cpu().numpy() for x in e.evaluate_theta(0, return_seq=True, return_lp=True)]
    assert _compare_tokens(seq0, w['base'], w['bfr']) == 0
    keep = ~w['bfr'].any(1)
    m = _live(w['base']) & keep[:, None]
    assert np.abs(lp0[m] - w['blp'][m]).max() <= 1e-5
    # two members, both signs
    fit, seq = e.evaluate(IT, 0, P, SIGMA, return_seq=True)
    assert seq.shape == (P, 2, B, T)
    fit, seq = fit.cpu().numpy(), seq.cpu().numpy()
    for k in range(P):
        for s in range(2):
            assert _compare_tokens(seq[k, s], oseq[k, s], ofr[k, s]) == 0, (k, s)
            f_ref, _ = CR.rollout_fitness(w['scorer'], seq[k, s], w['gts'])
            assert _close(fit[k, s], f_ref), (k, s, fit[k, s], f_ref)
    assert fit.max() > 0.0
    fit_l, seq_l, lp = [x.cpu().numpy() for x in e.evaluate(IT, 0, P, SIGMA, return_seq=True, return_lp=True)]
    assert np.array_equal(seq_l, seq) and np.array_equal(fit_l.view(np.uint64), fit.view(np.uint64))
    assert np.isfinite(lp).all() and (lp <= 0).all()
    for k in range(P):
        for s in range(2):
            keep = ~ofr[k, s].any(1)
            m = _live(oseq[k, s]) & keep[:, None]
            assert np.abs(lp[k, s][m] - olp[k, s][m]).max() <= 1e-5, (k, s)
    # identical bits from a second run of each
    fit2, seq2 = e.evaluate(IT, 0, P, SIGMA, return_seq=True)
    _, seq3, lp3 = e.evaluate(IT, 0, P, SIGMA, return_seq=True, return_lp=True)
    assert np.array_equal(seq2.cpu().numpy(), seq) and np.array_equal(fit2.cpu().numpy().view(np.uint64), fit.view(np.uint64))
    assert np.array_equal(seq3.cpu().numpy(), seq) and np.array_equal(lp3.cpu().numpy().view(np.uint32), lp.view(np.uint32))
    after = e.stats()
    assert all(after[k] == before[k] for k in COUNTERS), (before, after)
    assert not e.last_decode_bounded()


# ------------------------------------------------------------------------------------------------ 3. further checks
def test_ln_forced_exact_sweep_gives_the_unforced_bits(engines):
    w = _world('a')
    B = CASES['a']['B']
    plain = engines('a')
    _load(plain, w)
    fit_p, seq_p, lp_p = [x.cpu().numpy() for x in plain.evaluate(IT, 0, P, SIGMA, return_seq=True, return_lp=True)]
    e = _engine(w['dims'], B, False, (('NICNES_FORCE_EXACT', '1'),))
    try:
        _load(e, w)
        s0 = e.stats()
        fit, seq, lp = [x.cpu().numpy() for x in e.evaluate(IT, 0, P, SIGMA, return_seq=True, return_lp=True)]
        s1 = e.stats()
        assert np.array_equal(seq, seq_p) and np.array_equal(fit.view(np.uint64), fit_p.view(np.uint64))
        assert np.array_equal(lp.view(np.uint32), lp_p.view(np.uint32))
        assert s1['tie_fallbacks'] > s0['tie_fallbacks']
    finally:
        e.close()


def test_ln_neutral_tail_equals_the_handle_without_affine(engines):
    """gamma = 1, beta = 0: y * 1 + 0 is y. An internal consistency check only (both sides are this kernel)."""
    w = _world('a')
    dims, B = w['dims'], CASES['a']['B']
    plain = engines('a')
    _load(plain, w)
    want = [x.cpu().numpy() for x in plain.evaluate_theta(0, return_seq=True, return_lp=True)]
    e = _engine(dims, B, True)
    try:
        e.set_theta(np.concatenate([w['theta'], L.make_tail(dims.R)]))
        e.set_df_table(*_df(w))
        e.set_batch(w['fc'], w['gts'])
        got = [x.cpu().numpy() for x in e.evaluate_theta(0, return_seq=True, return_lp=True)]
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64))
        assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
    finally:
        e.close()


def _df(w):
    import nicnes
    keys, vals = nicnes.df_table_arrays(w['df'])
    return keys, vals, np.log(float(w['n']))


def test_ln_the_tail_is_perturbed(engines):
    """SM-VECTOR with sensitivity 1 everywhere except 1e-3 on the tail: the tail's noise a thousand times the rest's. The
    tokens are ln_ref's on theta +- delta' and not the plain members': the kernel forms gamma, beta as W0 +- delta."""
    w = _world(FEATURE_CASE)
    dims, e, table = w['dims'], engines(FEATURE_CASE), _table()
    theta = w['theta']
    _load(e, w)
    vec = np.ones(theta.size, np.float32)
    vec[dims.D:] = np.float32(1e-3)
    try:
        e.set_mutation('divide', vec)
        _, seq = e.evaluate(IT, 0, P, SIGMA, return_seq=True)
        seq = seq.cpu().numpy()
        nv = e.noise_vectors(IT, 0, P, SIGMA).cpu().numpy()
        differs = 0
        for k in range(P):
            delta = O.member_delta(table, _idx(theta.size, k), SIGMA, theta.size, ('divide', vec))
            assert np.array_equal(nv[k], delta), k
            assert np.abs(delta[dims.D:]).mean() > 100 * np.abs(delta[:dims.D]).mean()
            for s, sign in enumerate((+1, -1)):
                oseq, _, fr = _decode(dims, O.perturb(theta, table, _idx(theta.size, k), SIGMA, sign, ('divide', vec)),
                                      w['fc'])
                assert fr.any(1).mean() <= FRAGILE_CAP
                assert _compare_tokens(seq[k, s], oseq, fr) == 0, (k, s)
                differs += int((seq[k, s] != w['oseq'][k, s]).any(1).sum())
        assert differs >= 1
    finally:
        e.set_mutation('plain')


# ------------------------------------------------------------------------------------------------ 4. the other paths
def test_ln_evaluate_theta_and_the_sigma0_member(engines):
    w = _world(FEATURE_CASE)
    e = engines(FEATURE_CASE)
    _load(e, w)
    assert e.decode_path() == 'ln'
    f2, seq2, lp2 = e.evaluate(0, 0, 1, 0.0, return_seq=True, return_lp=True)
    f1, seq1, lp1 = e.evaluate_theta(0, return_seq=True, return_lp=True)
    f2, f1 = f2.cpu().numpy(), f1.cpu().numpy()
    assert np.array_equal(seq1.cpu().numpy(), seq2[0, 0].cpu().numpy())
    assert _compare_tokens(seq1.cpu().numpy(), w['base'], w['bfr']) == 0
    np.testing.assert_allclose(lp1.cpu().numpy(), lp2[0, 0].cpu().numpy(), rtol=2.5e-7, atol=0)
    assert f2[0, 0] == f2[0, 1] and f1[0] == f2[0, 0]
    f_ref, _ = CR.rollout_fitness(w['scorer'], seq1.cpu().numpy(), w['gts'])
    assert _close(f1[0], f_ref)


def test_ln_split_decode_and_evaluate(engines):
    w = _world(FEATURE_CASE)
    dims, e = w['dims'], engines(FEATURE_CASE)
    _load(e, w)
    _, seq_t = e.evaluate_theta(0, return_seq=True)
    split = e.make_split(w['fc'], w['gts'])
    try:
        assert torch.equal(split.decode(), seq_t)
        res, seq_e = split.evaluate(return_seq=True)
        assert torch.equal(seq_e, seq_t) and res == split.score(seq_t)
        assert np.isfinite(res['CIDEr']) and res['CIDEr'] > 0
    finally:
        split.close()
    fc = np.random.Generator(np.random.PCG64(5)).standard_normal((300, dims.F)).astype(np.float32)   # two pseudo-members
    oseq, _, fr = _decode(dims, w['theta'], fc)
    split = e.make_split(fc)
    try:
        got = split.decode().cpu().numpy()
        assert _compare_tokens(got, oseq, fr) == 0
        assert np.array_equal(split.decode(259, 30).cpu().numpy(), got[259:289])
    finally:
        split.close()


def test_ln_per_member_batches(engines):
    import nicnes.synthetic as S
    w = _world(FEATURE_CASE)
    dims, e, theta = w['dims'], engines(FEATURE_CASE), w['theta']
    batches = []
    for j in range(2):
        fc = np.random.Generator(np.random.PCG64(50 + j)).standard_normal((9, dims.F)).astype(np.float32)
        base, _, _ = _decode(dims, theta, fc)
        gts, _, _ = S.build_references(base, dims.vocab_size, seed=20 + j, df_sets=64)
        batches.append((fc, gts))
    _load(e, w)
    e.set_batches(batches)
    mb = [1, 0]
    fit, seq = e.evaluate(IT, 0, 2, SIGMA, return_seq=True, member_batch=mb)
    fit, seq = fit.cpu().numpy(), seq.cpu().numpy()
    for k in range(2):
        fc, gts = batches[mb[k]]
        for s, sign in enumerate((+1, -1)):
            oseq, _, fr = _decode(dims, O.perturb(theta, _table(), _idx(theta.size, k), SIGMA, sign), fc)
            assert _compare_tokens(seq[k, s], oseq, fr) == 0, (k, s)
            f_ref, _ = CR.rollout_fitness(w['scorer'], seq[k, s], gts)
            assert _close(fit[k, s], f_ref), (k, s)


@pytest.mark.parametrize('mode', ['greedy_logprob', 'greedy_expprob', 'greedy_linprob', 'greedy_avgprob'])
def test_ln_fitness_criteria_match_the_oracle_scorer(engines, mode):
    w = _world(FEATURE_CASE)
    e = engines(FEATURE_CASE)
    _load(e, w)
    e.set_fitness_mode(mode)
    try:
        fit, seq, lp = e.evaluate(IT, 0, 2, SIGMA, return_seq=True, return_lp=True)
        fit_nolp = e.evaluate(IT, 0, 2, SIGMA).cpu().numpy()
    finally:
        e.set_fitness_mode('greedy')
    fit, seq, lp = fit.cpu().numpy(), seq.cpu().numpy(), lp.cpu().numpy()
    assert np.array_equal(fit, fit_nolp)
    for k in range(2):
        for s in range(2):
            assert _compare_tokens(seq[k, s], w['oseq'][k, s], w['ofr'][k, s]) == 0
            _, scores = CR.rollout_fitness(w['scorer'], seq[k, s], w['gts'])
            f_own = CR.criterion_fitness(mode, lp[k, s], seq[k, s], scores)
            assert abs(fit[k, s] - f_own) <= 1e-6 * max(1.0, abs(f_own)), (k, s, fit[k, s], f_own)
            if not w['ofr'][k, s].any():
                f_ref = CR.criterion_fitness(mode, w['olp'][k, s], w['oseq'][k, s], scores)
                assert abs(fit[k, s] - f_ref) <= 1e-5 * max(1.0, abs(f_ref)), (k, s, fit[k, s], f_ref)


def test_ln_proportional_mutation_covers_the_tail(engines):
    """SM-PROPORTIONAL on a fresh tail (gamma = 1, beta = 0): the beta entries, exact zeros, take the mean of |theta| as
    PolicyNet.evolve gives them (nets.py:108-112), so they are perturbed too."""
    w = _world(FEATURE_CASE)
    dims, e, table = w['dims'], engines(FEATURE_CASE), _table()
    theta = np.concatenate([w['theta'][:dims.D], L.make_tail(dims.R)])
    _load(e, w)
    e.set_theta(theta)
    try:
        mean_abs = float(np.abs(theta).mean(dtype=np.float32))
        vec = np.where(theta == 0, np.float32(mean_abs), np.abs(theta)).astype(np.float32)
        tail = L.tail_offsets(dims)
        assert (theta[tail[1]:tail[2]] == 0).all() and (vec[tail[1]:tail[2]] == np.float32(mean_abs)).all()
        e.set_mutation_proportional(mean_abs)
        _, seq = e.evaluate(IT, 0, P, SIGMA, return_seq=True)
        seq = seq.cpu().numpy()
        nv = e.noise_vectors(IT, 0, P, SIGMA).cpu().numpy()
        for k in range(P):
            assert np.array_equal(nv[k], O.member_delta(table, _idx(theta.size, k), SIGMA, theta.size, ('scale', vec))), k
            assert (nv[k][tail[1]:tail[2]] != 0).all()
            for s, sign in enumerate((+1, -1)):
                oseq, _, fr = _decode(dims, O.perturb(theta, table, _idx(theta.size, k), SIGMA, sign, ('scale', vec)), w['fc'])
                assert _compare_tokens(seq[k, s], oseq, fr) == 0, (k, s)
    finally:
        e.set_mutation('plain')
        e.set_theta(w['theta'])


def test_ln_grad_partial_and_optimizers_bit_exact(engines, golden_dir):
    """rank_weights, grad_partial, Adam and SGD at the affine D: the goldens sit at the END of theta, on the tail."""
    w = _world(FEATURE_CASE)
    e, table = engines(FEATURE_CASE), _table()
    D = w['theta'].size
    assert e.D == D == w['dims'].D + 22 * w['dims'].R
    e.set_mutation('plain')
    rng = np.random.default_rng(1)
    fit = rng.random((3, 2))
    w_ref, cr_ref = O.weights_from_fitness(fit)
    cr, wt = e.rank_weights(torch.from_numpy(fit).to(e.device))
    assert np.array_equal(cr.cpu().numpy(), cr_ref) and np.array_equal(wt.cpu().numpy(), w_ref)
    g = e.grad_partial(9, 0, 3, wt, SIGMA).cpu().numpy()
    acc = np.zeros(D, np.float64)
    for i in range(3):
        acc += np.float64(w_ref[i]) * O.member_delta(table, _idx(D, i, 9), SIGMA, D).astype(np.float64)
    assert np.array_equal(g, acc.astype(np.float32)) and (g[w['dims'].D:] != 0).any()

    def embed(arr, dtype):
        out = np.zeros(D, dtype)
        out[D - arr.size:] = arr
        return out
    try:
        z = np.load(os.path.join(golden_dir, 'adam.npz'))
        n = z['theta0'].size
        e.set_theta(embed(z['theta0'], np.float32))
        e.set_adam_state(np.zeros(D), np.zeros(D), 0)
        for k in range(3):
            ratio = e.adam_step(torch.from_numpy(embed(z['grads'][k] * np.float32(2.0), np.float32)).to(e.device), 1,
                                float(z['l2coeff']), float(z['stepsize']))
            assert np.array_equal(e.theta()[0].cpu().numpy()[-n:], z['thetas'][k]), k
            m, v, t = e.adam_state()
            assert np.array_equal(m.cpu().numpy()[-n:], z['ms'][k]) and np.array_equal(v.cpu().numpy()[-n:], z['vs'][k])
            assert t == k + 1 and ratio > 0
        z = np.load(os.path.join(golden_dir, 'sgd.npz'))
        n = z['theta0'].size
        e.set_theta(embed(z['theta0'], np.float32))
        e.set_adam_state(np.zeros(D), np.zeros(D), 0)
        for k in range(3):
            ratio = e.sgd_step(torch.from_numpy(embed(z['grads'][k] * np.float32(2.0), np.float32)).to(e.device), 1,
                               float(z['l2coeff']), float(z['stepsize']), float(z['momentum']))
            t64, t32 = e.theta()
            assert np.array_equal(t64.cpu().numpy()[-n:], z['thetas'][k]), k
            assert np.array_equal(t32.cpu().numpy()[-n:], z['thetas'][k].astype(np.float32))
            assert ratio > 0
    finally:
        e.set_theta(w['theta'])
        e.set_adam_state(np.zeros(D), np.zeros(D), 0)


def test_ln_master_two_iterations_with_a_validator_and_a_snapshot(tmp_path):
    """EngineMaster.run on a layer_n_affine experiment with a Validator: two iterations complete, the tail moves, the
    best elite and the snapshot carry the six tensors under the reference's names, and the snapshot loads back."""
    import nicnes
    import nicnes.synthetic as S
    from nicnes import config as C, master as M
    from nicnes.validation import Validator
    from tests.test_gpu_wide import _Loader
    dims = O.Dims(vocab_size=67, E=128, R=128, F=128)
    sd = S.Dims(67, 128, 128, 128, layer_n=True, layer_n_affine=True)
    theta = S.init_theta(sd, 0, 4.0, 0.1)                       # a fresh theta: weight 1, bias 0 in the tail
    assert np.array_equal(theta[dims.D:], L.make_tail(128))
    fc = np.random.Generator(np.random.PCG64(1234)).standard_normal((27, dims.F)).astype(np.float32)
    base, _, _ = _decode(dims, theta, fc)
    gts, df, n = S.build_references(base, dims.vocab_size, seed=9, n_refs=5, df_sets=128)
    Pm = 4

    def spec():
        return C.ExperimentSpec({
            'algorithm': 'nic_nes', 'nb_offspring': Pm,
            'config': {'noise_stdev': 0.01, 'batch_size': 8, 'l2coeff': 1e-3, 'snapshot_freq': 2, 'single_batch': True,
                       'patience': 5, 'num_val_items': 9},
            'policy_options': {'net': 'fc_caption', 'fitness': 'greedy',
                               'model_options': {'fc_feat_size': 128, 'layer_n': True, 'layer_n_affine': True}},
            'optimizer_options': {'type': 'adam', 'args': {'stepsize': 1e-2}}}, vocab_size=67)
    e = nicnes.Engine(**spec().engine_kwargs(max_members=Pm, noise_len=1 << 21, noise_seed=0, max_batch=8))
    try:
        assert e.D == theta.size and e.decode_path(8, Pm) == 'ln'
        e.set_noise_table(_table(1 << 21))
        keys, vals = nicnes.df_table_arrays(df)
        e.set_df_table(keys, vals, np.log(float(n)))
        la = _Loader(fc, gts, 11, 67)
        m = M.EngineMaster(spec(), e, log_dir=str(tmp_path / 'gpu'), theta=theta, validator=Validator(e, la, 'val', 9))
        m.run(la, max_iterations=2)
        assert len(m.stats) == 2
        for a in m.stats:
            assert np.isfinite(a['score_mean']) and np.isfinite(a['val_score']) and a['val_score'] > 0
        t64 = e.theta()[0].cpu().numpy()
        assert (t64[dims.D:] != theta[dims.D:]).all()           # Adam moved every entry of the tail
        mm, vv, t = e.adam_state()
        assert t == 2
        best = torch.load(m.best_model_path(), weights_only=True)
        assert list(best)[9:] == L.LN_NAMES
        snap = [f for f in os.listdir(str(tmp_path / 'gpu' / 'snapshot')) if f.startswith('z_info')]
        assert len(snap) == 1
        e.set_theta(theta)
        e.set_adam_state(np.zeros(e.D), np.zeros(e.D), 0)
        m2 = M.EngineMaster(spec(), e, log_dir=str(tmp_path / 'gpu2'))
        m2.load_snapshot(str(tmp_path / 'gpu' / 'snapshot' / snap[0]))
        assert np.array_equal(e.theta()[0].cpu().numpy(), t64)
        m2b, v2b, t2 = e.adam_state()
        assert t2 == 2 and torch.equal(m2b, mm) and torch.equal(v2b, vv)
    finally:
        e.close()


def test_ln_refusals_leave_the_handle_usable(engines):
    import nicnes
    w = _world(FEATURE_CASE)
    dims, e = w['dims'], engines(FEATURE_CASE)
    _load(e, w)
    want = e.evaluate(IT, 0, 2, SIGMA).cpu().numpy()
    split = e.make_split(w['fc'], w['gts'])
    refused = [
        lambda: e.set_fitness_mode('sample'),
        lambda: e.set_fitness_mode('self_critical'),
        lambda: e.set_fitness_mode('sc_loss'),
        lambda: e.sum_sensitivity(8, 0.01),
        lambda: e.es_create(4, 1),
        lambda: split.decode_beam(beam_size=3),
        lambda: split.evaluate(beam_size=2),
        lambda: e.test_logit_chain(IT, 0, SIGMA, 0, np.zeros((32, dims.R), np.float32)),
        lambda: e.test_certify_items(IT, 0, SIGMA, 0, np.zeros((128, dims.R), np.float32), np.array([[0, 1]], np.int32)),
        lambda: e.set_decode_split(4, 4),
        lambda: e.set_decode_split(2, 4),
        lambda: e.set_decode_split(1, 2),
        lambda: e.set_decode_streams(2),
    ]
    try:
        for i, call in enumerate(refused):
            with pytest.raises(nicnes.NicnesError, match='not supported.*layer_n'):
                call()
            assert e.decode_path(40, 2) == 'ln', i
            assert np.array_equal(e.evaluate(IT, 0, 2, SIGMA).cpu().numpy(), want), i
        e.set_decode_split(0, 0)
        e.set_decode_split(1, 4)
        e.set_decode_streams(1)
        e.set_decode_streams(0)
        e.set_decode_coop(0)
        e.set_decode_coop(1)
        e.set_decode_screen(1)                     # ignored, as on a wide handle
        assert e.decode_path(40, 512) == 'ln'
        assert np.array_equal(e.evaluate(IT, 0, 2, SIGMA).cpu().numpy(), want)
    finally:
        split.close()
        e.set_decode_split(0, 0)
        e.set_fitness_mode('greedy')


def test_ln_cell_entry_is_refused_without_layer_n():
    import nicnes
    dims = O.Dims(vocab_size=7, E=128, R=128, F=128)
    e = _engine(dims, 8, False, noise_len=1 << 21, max_members=1, layer_n=False)
    try:
        assert e.decode_path(8, 1) != 'ln'
        e.set_theta(O.make_theta(dims, 0))
        z = np.zeros((4, 128), np.float32)
        with pytest.raises(nicnes.NicnesError, match='layer_n'):
            e.test_ln_cell(z, z, z)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 5. the entries
LN_MODEL_OPTIONS = {'fc_feat_size': 128, 'layer_n': True, 'layer_n_affine': True}


def test_ln_worker_process_serves_engine_master(tmp_path):
    """`python -m nicnes.worker` on a layer_n_affine experiment (the default engine factory builds its Engine from the
    experiment's model_options, the .pth it loads carries the six tail tensors): two dispatched iterations give the
    theta of the local loop on the same inputs, as at the default model (tests/test_gpu_worker.py)."""
    import signal
    import socket
    import subprocess
    import sys
    import nicnes
    import nicnes.synthetic as S
    from nicnes import config as C, data, master as M, transport as T
    from nicnes.worker import STOP_KEY
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dims = O.Dims(vocab_size=67, E=128, R=128, F=128)
    theta = _theta(dims, True, seed=2, tail_seed=1700)
    Pm, B, n_len = 8, 12, 1 << 21
    fc = np.random.Generator(np.random.PCG64(77)).standard_normal((B, dims.F)).astype(np.float32)
    base, _, _ = _decode(dims, theta, fc)
    gts, df, n = S.build_references(base, dims.vocab_size, seed=5, n_refs=5, df_sets=128)
    batch = {'fc_feats': fc, 'gts': gts}

    def spec():
        return C.ExperimentSpec({
            'algorithm': 'nic_nes', 'nb_offspring': Pm,
            'config': {'noise_stdev': 0.01, 'batch_size': B, 'l2coeff': 1e-7, 'snapshot_freq': 0},
            'policy_options': {'net': 'fc_caption', 'fitness': 'greedy', 'model_options': dict(LN_MODEL_OPTIONS)},
            'optimizer_options': {'type': 'adam', 'args': {'stepsize': 1e-3}}}, vocab_size=67)
    e = nicnes.Engine(**spec().engine_kwargs(max_members=Pm, noise_len=n_len, noise_seed=0, max_batch=B))
    try:
        e.set_noise_table(_table(n_len))
        keys, vals = nicnes.df_table_arrays(df)
        e.set_df_table(keys, vals, np.log(float(n)))
        assert e.decode_path(B, Pm) == 'ln' and e.D == theta.size
        local = M.EngineMaster(spec(), e, log_dir=str(tmp_path / 'a'), theta=theta)
        local.run([batch] * 2, max_iterations=2)
        want = e.theta()[0].cpu().numpy()
        assert not np.array_equal(want.astype(np.float32)[dims.D:], theta[dims.D:])
        df_path = str(tmp_path / 'df.json')
        data.save_df_table(df_path, df, n)
        s = socket.socket()
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
        s.close()
        store = T.TCPStoreRedis('127.0.0.1', port, is_master=True)
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([repo, os.path.join(repo, 'nes-img-captioning_amd')]))
        cmd = [sys.executable, '-m', 'nicnes.worker', '--store', 'tcp://127.0.0.1:%d' % port, '--num_workers', '1',
               '--wire', 'engine', '--chunk', '4', '--noise_len', str(n_len), '--noise_seed', '0', '--vocab_size', '67',
               '--df_path', df_path, '--check_interval', '0.5']
        pool = subprocess.Popen(cmd, env=env, cwd=repo, start_new_session=True, stdout=subprocess.DEVNULL,
                                stderr=open(str(tmp_path / 'pool.log'), 'w'))
        try:
            e.set_theta(theta)
            e.set_adam_state(np.zeros(e.D), np.zeros(e.D), 0)
            master = M.EngineMaster(spec(), e, log_dir=str(tmp_path / 'b'))
            master.run_dispatched(T.MasterClient(store), [batch] * 2, max_iterations=2, result_timeout=240)
            assert np.array_equal(e.theta()[0].cpu().numpy(), want)
            store.set(STOP_KEY, b'1')
            assert pool.wait(timeout=120) == 0
        finally:
            if pool.poll() is None:
                os.killpg(pool.pid, signal.SIGKILL)
    finally:
        e.close()


def test_ln_evaluate_entry_scores_a_split(tmp_path):
    """python -m nicnes.evaluate (its main, in this process) on a layer_n_affine experiment and a .pth with the six tail
    tensors: the captions are ln_ref's on the split's images."""
    import json
    from nicnes import data as Dt, evaluate as EV, nes as N
    from nicnes.validation import decode_sequence
    from types import SimpleNamespace
    dims = O.Dims(vocab_size=67, E=128, R=128, F=128)
    theta = _theta(dims, True, seed=2, tail_seed=1700)
    rng = np.random.default_rng(3)
    n_img = 9
    images = [{'id': 700 + i, 'split': 'val' if i >= 4 else 'train', 'file_path': 'i%d.jpg' % i} for i in range(n_img)]
    ix_to_word = {str(i): 'w%d' % i for i in range(1, dims.vocab_size + 1)}
    with open(tmp_path / 'cocotalk.json', 'w') as f:
        json.dump({'ix_to_word': ix_to_word, 'images': images}, f)
    os.makedirs(tmp_path / 'fc')
    fc = rng.standard_normal((n_img, dims.F)).astype(np.float32)
    for im, row in zip(images, fc):
        np.save(tmp_path / 'fc' / ('%d.npy' % im['id']), row)
    ncap = rng.integers(5, 8, n_img)
    start = np.cumsum(np.concatenate([[0], ncap[:-1]])) + 1
    labels = rng.integers(1, dims.vocab_size + 1, (int(ncap.sum()), 16))
    labels[:, 9:] = 0
    Dt.LabelStore(labels, start, start + ncap - 1).save_npz(str(tmp_path / 'labels.npz'))
    exp = {'algorithm': 'nic_nes', 'dataset': 'mscoco', 'nb_offspring': 4,
           'config': {'noise_stdev': 0.01, 'batch_size': 3},
           'policy_options': {'net': 'fc_caption', 'fitness': 'greedy', 'model_options': dict(LN_MODEL_OPTIONS)},
           'caption_options': {'input_json': 'cocotalk.json', 'input_fc_dir': 'fc', 'input_label_h5': 'labels.npz'}}
    with open(tmp_path / 'exp.json', 'w') as f:
        json.dump(exp, f)
    cfg = SimpleNamespace(vocab_size=67, input_encoding_size=128, rnn_size=128, fc_feat_size=128, layer_n=1,
                          layer_n_affine=1)
    model = str(tmp_path / 'theta.pth')
    torch.save(N.state_dict_from_vector(torch.from_numpy(theta), N.param_shapes(SimpleNamespace(cfg=cfg))), model)
    out = str(tmp_path / 'eval.json')
    assert EV.main(['--exp', str(tmp_path / 'exp.json'), '--model', model, '--data_root', str(tmp_path), '--out', out,
                    '--split', 'val', '--num', '-1']) == 0
    res = json.load(open(out))
    assert [p['image_id'] for p in res['predictions']] == [704, 705, 706, 707, 708]
    assert np.isfinite(res['stats']['CIDEr'])
    seq, _, fr = _decode(dims, theta, fc[4:])
    assert not fr.any()
    assert [p['caption'] for p in res['predictions']] == decode_sequence(ix_to_word, seq)
