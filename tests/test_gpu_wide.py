"""GPU: the wide greedy decode (csrc/decode_wide_kernels.hip), models with rnn_size / input_encoding_size in
128, 256, 384, 512, behind the C ABI.

1. Parity against the CPU oracle (itself pinned to the reference at these widths by tests/test_wide_host.py): three
   members, both signs; width pairs that give 1, 2, 3 and 4 k windows per product with E != R in both directions; V1 = 8
   (one stage, 8 columns), 68 (two stages, the second 4 wide) and 9488; F = 128 and 384; T = 1, 3, 16; B = 40 and 130
   (two slabs, a 2-row tail). The suite's bars: tokens bit-exact up to the first step the oracle marks fragile, fitness
   1e-9 relative, log-probs 1e-5; two runs give the same bits; no fallback or fault counter moves. Cases a and e again
   with the kernel's exact tie sweep forced on every step (NICNES_FORCE_EXACT=1): the same tokens and bits.
     case  E    R    V1    F    T   B
     a     256  256  68    128  16  40
     b     128  256  8     128  3   40
     c     256  128  68    384  16  130
     d     384  128  8     384  1   40
     e     512  512  68    128  16  40
     f     256  256  9488  128  3   130
2. The wide kernel at the default widths (the test hook NICNES_DECODE_WIDE=1) against the fused fp32 kernel
   (NICNES_SCREEN=0 for both): tokens, fitness and log-probs bit for bit, and the reference's tokens of
   decode_full_{wc,xavier}.npz end to end.
3. tests/golden/decode_wide.npz (the imported reference at three width pairs) end to end on the rows its margins do not
   mark as near-ties.
4. The engine's features at (256, 256): evaluate_theta, the resident split, per-member batches, the greedy_* criteria,
   the materialised mutations, grad_partial / Adam / SGD at the wide D, two EngineMaster.run iterations with a validator,
   and a `python -m nicnes.worker` process serving two dispatched iterations.
5. What is refused at wide dims says "not supported" and leaves the handle usable; widths 64, 192, 640 are refused at
   create."""
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from oracle import oracle as O                                  # noqa: E402
from oracle import cider_ref as CR                              # noqa: E402
from tests.test_gpu_parity import _compare_tokens               # noqa: E402
from tests.test_wide_host import wide_cases, MARGIN, FRAGILE_CAP    # noqa: E402

NOISE_LEN = 1 << 23
SEED = 7
SIGMA = 0.01
IT = 3
P = 3

CASES = {
    'a': dict(E=256, R=256, vocab=67, F=128, T=16, B=40),
    'b': dict(E=128, R=256, vocab=7, F=128, T=3, B=40),
    'c': dict(E=256, R=128, vocab=67, F=384, T=16, B=130),
    'd': dict(E=384, R=128, vocab=7, F=384, T=1, B=40, fc_seed=240),
    'e': dict(E=512, R=512, vocab=67, F=128, T=16, B=40),
    'f': dict(E=256, R=256, vocab=9487, F=128, T=3, B=130),
}

_cache = {}


def _dims(case):
    c = CASES[case]
    return O.Dims(vocab_size=c['vocab'], E=c['E'], R=c['R'], F=c['F'], T=c['T'])


def _table(n=NOISE_LEN):
    if ('table', n) not in _cache:
        _cache['table', n] = O.noise_table(n, 123)
    return _cache['table', n]


def _idx(dims, member, iteration=IT, n=NOISE_LEN):
    return O.noise_index(SEED, iteration, member, n, dims.D)


def _world(case):
    """The oracle's side of a case, computed once and never modified."""
    if ('world', case) not in _cache:
        import nicnes.synthetic as S
        c, dims, table = CASES[case], _dims(case), _table()
        theta = O.make_theta(dims, 0, 4.0, 0.1)
        fc = np.random.Generator(np.random.PCG64(c.get('fc_seed', 100 + c['B']))).standard_normal(
            (c['B'], c['F'])).astype(np.float32)
        base, _, _ = O.decode(dims, theta, fc)
        gts, df, n = S.build_references(base, dims.vocab_size, seed=11, df_sets=64, T=dims.T)
        B = c['B']
        oseq = np.zeros((P, 2, B, dims.T), np.int32)
        olp = np.zeros((P, 2, B, dims.T), np.float32)
        ofr = np.zeros((P, 2, B, dims.T), np.uint8)
        for k in range(P):
            for s, sign in enumerate((+1, -1)):
                oseq[k, s], olp[k, s], ofr[k, s] = O.decode(dims, O.perturb(theta, table, _idx(dims, k), SIGMA, sign), fc)
        for a in (base, oseq, olp, ofr, theta, fc):
            a.setflags(write=False)
        _cache['world', case] = dict(dims=dims, theta=theta, fc=fc, base=base, gts=gts, df=df, n=n, oseq=oseq, olp=olp,
                                     ofr=ofr, scorer=CR.CiderDOracle(df, n))
    return _cache['world', case]


def _engine(dims, max_batch, env=(), noise_len=NOISE_LEN, max_members=4):
    import nicnes
    mp = pytest.MonkeyPatch()
    for k, v in env:
        mp.setenv(k, v)
    try:
        e = nicnes.Engine(vocab_size=dims.vocab_size, input_encoding_size=dims.E, rnn_size=dims.R, fc_feat_size=dims.F,
                          seq_length=dims.T, max_batch=max_batch, max_members=max_members, noise_len=noise_len,
                          noise_seed=SEED)
    finally:
        mp.undo()
    e.set_noise_table(_table(noise_len))
    assert e.D == dims.D
    return e


@pytest.fixture(scope='module')
def engines():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    made = {}

    def get(case):
        if case not in made:
            made[case] = _engine(_dims(case), CASES[case]['B'])
        return made[case]
    yield get
    for e in made.values():
        e.close()


def _load(e, theta, fc, gts, df, n):
    import nicnes
    e.set_theta(theta)
    keys, vals = nicnes.df_table_arrays(df)
    e.set_df_table(keys, vals, np.log(float(n)))
    e.set_batch(fc, gts)


def _close(got, want, rel=1e-9):
    return abs(got - want) <= rel * max(1.0, abs(want))


COUNTERS = ('tie_fallbacks', 'sample_stage_fallbacks', 'coop_timeouts', 'sample_slot_timeouts', 'screen_candidates',
            'screen_fallback_rows', 'queue_timeouts')


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize('case', list(CASES))
def test_wide_parity_against_the_oracle(engines, case):
    w = _world(case)
    dims, B, T = w['dims'], CASES[case]['B'], CASES[case]['T']
    oseq, olp, ofr = w['oseq'], w['olp'], w['ofr']
    frag_rows = ofr.any(-1)
    assert frag_rows.mean() <= FRAGILE_CAP, 'too many fragile rows (%d of %d): change the fc seed, not the cap' % (
        frag_rows.sum(), frag_rows.size)
    assert np.unique(oseq).size >= min(CASES[case]['vocab'], 12)
    e = engines(case)
    _load(e, w['theta'], w['fc'], w['gts'], w['df'], w['n'])
    assert e.decode_path(B, P) == 'wide' and e.decode_shape(B, P) == (4, (B + 127) // 128, 1)
    assert [int(i) for i in e.noise_indices(IT, 0, P).cpu().numpy()] == [_idx(dims, k) for k in range(P)]
    before = e.stats()
    fit, seq = e.evaluate(IT, 0, P, SIGMA, return_seq=True)
    assert seq.shape == (P, 2, B, T)
    fit, seq = fit.cpu().numpy(), seq.cpu().numpy()
    for k in range(P):
        for s in range(2):
            assert _compare_tokens(seq[k, s], oseq[k, s], ofr[k, s]) == 0, (k, s)
            f_ref, _ = CR.rollout_fitness(w['scorer'], seq[k, s], w['gts'])
            assert _close(fit[k, s], f_ref), (k, s, fit[k, s], f_ref)
    assert fit.max() > 0.0
    # the log-prob pass, and the same bits from a second run of each
    fit_l, seq_l, lp = e.evaluate(IT, 0, P, SIGMA, return_seq=True, return_lp=True)
    fit_l, seq_l, lp = fit_l.cpu().numpy(), seq_l.cpu().numpy(), lp.cpu().numpy()
    assert np.array_equal(seq_l, seq) and np.array_equal(fit_l.view(np.uint64), fit.view(np.uint64))
    assert np.isfinite(lp).all() and (lp <= 0).all()
    for k in range(P):
        for s in range(2):
            keep = ~frag_rows[k, s]
            m = np.concatenate([np.ones((B, 1), bool), oseq[k, s][:, :-1] > 0], 1) & keep[:, None]
            assert np.abs(lp[k, s][m] - olp[k, s][m]).max() <= 1e-5, (k, s)
            if keep.all():                                 # steps after the batch's last finishing one stay 0
                ends = np.where((oseq[k, s] == 0).any(1), (oseq[k, s] == 0).argmax(1) + 1, T)
                assert (lp[k, s][:, ends.max():] == 0).all(), (k, s)
    fit2, seq2 = e.evaluate(IT, 0, P, SIGMA, return_seq=True)
    _, seq3, lp3 = e.evaluate(IT, 0, P, SIGMA, return_seq=True, return_lp=True)
    assert np.array_equal(seq2.cpu().numpy(), seq) and np.array_equal(fit2.cpu().numpy().view(np.uint64), fit.view(np.uint64))
    assert np.array_equal(seq3.cpu().numpy(), seq) and np.array_equal(lp3.cpu().numpy().view(np.uint32), lp.view(np.uint32))
    after = e.stats()
    assert all(after[k] == before[k] for k in COUNTERS), (before, after)
    assert not e.last_decode_bounded()


@pytest.mark.parametrize('case', ['a', 'e'])
def test_wide_exact_tie_sweep_matches_the_oracle(engines, case):
    """The wide kernel's own exact tie sweep (the second pass over ceil(V1 / 32) x R / 128 tiles, normally taken only
    when more records than tracked fall in the tie window) forced on every step (NICNES_FORCE_EXACT=1), with 2 and 4 k
    windows per logit product: the oracle's tokens, the tokens, fitness and log-prob bits of the unforced run, and
    one fallback counted per workgroup and decode step run."""
    w = _world(case)
    B, T = CASES[case]['B'], CASES[case]['T']
    oseq, ofr = w['oseq'], w['ofr']
    plain = engines(case)
    _load(plain, w['theta'], w['fc'], w['gts'], w['df'], w['n'])
    fit_p, seq_p, lp_p = [x.cpu().numpy() for x in plain.evaluate(IT, 0, P, SIGMA, return_seq=True, return_lp=True)]
    e = _engine(w['dims'], B, (('NICNES_FORCE_EXACT', '1'),))
    try:
        _load(e, w['theta'], w['fc'], w['gts'], w['df'], w['n'])
        assert e.decode_path(B, P) == 'wide'
        s0 = e.stats()
        fit, seq = e.evaluate(IT, 0, P, SIGMA, return_seq=True)
        fit, seq = fit.cpu().numpy(), seq.cpu().numpy()
        s1 = e.stats()
        for k in range(P):
            for s in range(2):
                assert _compare_tokens(seq[k, s], oseq[k, s], ofr[k, s]) == 0, (k, s)
        assert np.array_equal(seq, seq_p) and np.array_equal(fit.view(np.uint64), fit_p.view(np.uint64))
        # a greedy-only decode leaves a workgroup (a member: one slab) after the step that ends its last caption
        ends = np.where((seq == 0).any(-1), (seq == 0).argmax(-1) + 1, T)           # [P, 2, B]
        steps = int(ends.reshape(P, -1).max(1).sum())
        assert s1['tie_fallbacks'] - s0['tie_fallbacks'] == steps, (s0, s1, steps)
        assert steps >= T * P                      # every member has a caption of full length: T sweeps per workgroup
        # the log-prob decode (one slab: the same exit): as many sweeps again, and the same lse bits
        fit_l, seq_l, lp = [x.cpu().numpy() for x in e.evaluate(IT, 0, P, SIGMA, return_seq=True, return_lp=True)]
        s2 = e.stats()
        assert s2['tie_fallbacks'] - s1['tie_fallbacks'] == steps, (s1, s2)
        assert np.array_equal(seq_l, seq_p) and np.array_equal(fit_l.view(np.uint64), fit_p.view(np.uint64))
        assert np.array_equal(lp.view(np.uint32), lp_p.view(np.uint32))
        assert all(s2[k] == s0[k] for k in COUNTERS if k != 'tie_fallbacks'), (s0, s2)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 2. default widths
@pytest.mark.parametrize('vocab,F,B', [(67, 384, 130), (9487, 256, 40)], ids=['V68', 'V9488'])
def test_wide_kernel_equals_the_fused_kernel_at_the_default_widths(vocab, F, B):
    import nicnes.synthetic as S
    dims = O.Dims(vocab_size=vocab, F=F)
    theta = O.make_theta(dims, 0, 4.0, 0.1)
    fc = np.random.Generator(np.random.PCG64(100 + B)).standard_normal((B, F)).astype(np.float32)
    base, _, _ = O.decode(dims, theta, fc)
    gts, df, n = S.build_references(base, dims.vocab_size, seed=11, df_sets=64)
    out = {}
    for name, env in (('wide', (('NICNES_DECODE_WIDE', '1'), ('NICNES_SCREEN', '0'))), ('fused', (('NICNES_SCREEN', '0'),))):
        e = _engine(dims, B, env)
        try:
            _load(e, theta, fc, gts, df, n)
            if name == 'fused':
                e.set_decode_split(1, 4)           # the fused kernel whatever the automatic shape of (B, P) is
            assert e.decode_path(B, P) == ('wide' if name == 'wide' else 'fused')
            fit, seq = e.evaluate(IT, 0, P, SIGMA, return_seq=True)
            fit_l, seq_l, lp = e.evaluate(IT, 0, P, SIGMA, return_seq=True, return_lp=True)
            out[name] = [x.cpu().numpy() for x in (fit, seq, fit_l, seq_l, lp)]
            st = e.stats()
            assert st['coop_timeouts'] == 0 and st['sample_slot_timeouts'] == 0 and st['screen_candidates'] == 0, st
        finally:
            e.close()
    a, b = out['wide'], out['fused']
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3]) and np.array_equal(a[1], a[3])
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))
    assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))
    assert np.array_equal(a[4].view(np.uint32), b[4].view(np.uint32))
    assert np.unique(a[1]).size >= 12 and a[0].max() > 0


@pytest.mark.parametrize('kind', ['wc', 'xavier'])
def test_wide_kernel_reproduces_the_reference_goldens_at_the_default_dims(kind, golden_dir):
    z = np.load(os.path.join(golden_dir, 'decode_full_%s.npz' % kind))
    V, E, R, F, T = [int(x) for x in z['dims']]
    dims = O.Dims(vocab_size=V, E=E, R=R, F=F, T=T)
    assert (E, R) == (128, 128) and int(z['noise_len']) == NOISE_LEN and int(z['noise_seed']) == SEED
    theta = O.make_theta(dims, int(z['theta_seed']), float(z['gain']), float(z['bias_std']))
    B = int(z['B'])
    fc = np.random.Generator(np.random.PCG64(int(z['fc_seed']))).standard_normal((B, F)).astype(np.float32)
    gts = [np.ones((1, T), np.int32)] * B
    e = _engine(dims, B, (('NICNES_DECODE_WIDE', '1'),))
    try:
        _load(e, theta, fc, gts, {}, 4096)
        assert e.decode_path(B, 2) == 'wide'
        _, seq0 = e.evaluate_theta(0, return_seq=True)
        _, seq = e.evaluate(int(z['iteration']), 0, 2, float(z['sigma']), return_seq=True)
        seq0, seq = seq0.cpu().numpy(), seq.cpu().numpy().reshape(4, B, T)
        # every row up to its first near-tie step; a handful of rows of each rollout end to end (xavier: 7 of theta's 16)
        assert _compare_tokens(seq0, z['seq'], z['margins'] < MARGIN) == 0
        ok = (z['margins'] >= MARGIN).all(1)
        assert ok.sum() >= 5 and np.array_equal(seq0[ok], z['seq'][ok])
        for i in range(4):
            assert _compare_tokens(seq[i], z['member_seq'][i], z['member_margins'][i] < MARGIN) == 0, i
            ok = (z['member_margins'][i] >= MARGIN).all(1)
            assert ok.sum() >= 5 and np.array_equal(seq[i][ok], z['member_seq'][i][ok]), i
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 3. the fixture
def test_wide_reference_fixture_end_to_end():
    n_len = 1 << 21
    for name, d, theta, fc, rolls in wide_cases():
        B = fc.shape[0]
        e = _engine(d, B, noise_len=n_len)
        try:
            _load(e, theta, fc, [np.ones((1, d.T), np.int32)] * B, {}, 4096)
            assert e.decode_path(B, 2) == 'wide'
            _, seq0 = e.evaluate_theta(0, return_seq=True)
            _, seq = e.evaluate(IT, 0, 2, SIGMA, return_seq=True)
            got = [seq0.cpu().numpy()] + list(seq.cpu().numpy().reshape(4, B, d.T))
            for i, (_, rseq, mar, _) in enumerate(rolls):
                ok = (mar >= MARGIN).all(1)
                assert ok.mean() >= 1 - FRAGILE_CAP and np.array_equal(got[i][ok], rseq[ok]), (name, i)
        finally:
            e.close()


# ------------------------------------------------------------------------------------------------ 4. features
def test_wide_evaluate_theta_equals_the_sigma0_member(engines):
    w = _world('a')
    e = engines('a')
    _load(e, w['theta'], w['fc'], w['gts'], w['df'], w['n'])
    try:
        for mode in ('greedy', 'greedy_linprob'):
            e.set_fitness_mode(mode)
            f2, seq2, lp2 = e.evaluate(0, 0, 1, 0.0, return_seq=True, return_lp=True)
            f1, seq1, lp1 = e.evaluate_theta(0, return_seq=True, return_lp=True)
            f2, f1 = f2.cpu().numpy(), f1.cpu().numpy()
            assert np.array_equal(seq1.cpu().numpy(), seq2[0, 0].cpu().numpy()), mode
            assert np.array_equal(seq1.cpu().numpy(), w['base'])
            np.testing.assert_allclose(lp1.cpu().numpy(), lp2[0, 0].cpu().numpy(), rtol=2.5e-7, atol=0)
            assert f2[0, 0] == f2[0, 1]
            if mode == 'greedy':
                assert f1[0] == f2[0, 0], (f1, f2)
                f_ref, _ = CR.rollout_fitness(w['scorer'], w['base'], w['gts'])
                assert _close(f1[0], f_ref)
            else:
                assert abs(f1[0] - f2[0, 0]) <= 1e-6 * abs(f2[0, 0]), (f1, f2)
    finally:
        e.set_fitness_mode('greedy')


def test_wide_split_decode_and_evaluate(engines):
    """Split.decode / Split.evaluate against evaluate_theta on the same images, and over three pseudo-members."""
    w = _world('a')
    dims, e = w['dims'], engines('a')
    _load(e, w['theta'], w['fc'], w['gts'], w['df'], w['n'])
    _, seq_t, lp_t = e.evaluate_theta(0, return_seq=True, return_lp=True)
    split = e.make_split(w['fc'], w['gts'])
    try:
        seq, lp = split.decode(return_lp=True)
        assert torch.equal(seq, seq_t)
        ended = (np.cumsum(seq.cpu().numpy() == 0, 1) - (seq.cpu().numpy() == 0)) > 0      # past the row's end token
        np.testing.assert_allclose(lp.cpu().numpy()[~ended], lp_t.cpu().numpy()[~ended], rtol=2.5e-7, atol=0)
        res, seq_e = split.evaluate(return_seq=True)
        assert torch.equal(seq_e, seq_t) and res == split.score(seq_t)
        assert np.isfinite(res['CIDEr']) and res['CIDEr'] > 0
    finally:
        split.close()
    fc = np.random.Generator(np.random.PCG64(5)).standard_normal((600, dims.F)).astype(np.float32)
    oseq, _, fr = O.decode(dims, w['theta'], fc)
    split = e.make_split(fc)
    try:
        got = split.decode().cpu().numpy()
        assert _compare_tokens(got, oseq, fr) == 0
        assert np.array_equal(split.decode(259, 300).cpu().numpy(), got[259:559])
    finally:
        split.close()


def test_wide_per_member_batches(engines):
    import nicnes.synthetic as S
    w = _world('a')
    dims, e = w['dims'], engines('a')
    batches = []
    for j in range(3):
        fc = np.random.Generator(np.random.PCG64(50 + j)).standard_normal((33, dims.F)).astype(np.float32)
        base, _, _ = O.decode(dims, w['theta'], fc)
        gts, _, _ = S.build_references(base, dims.vocab_size, seed=20 + j, df_sets=64)
        batches.append((fc, gts))
    _load(e, w['theta'], w['fc'], w['gts'], w['df'], w['n'])
    e.set_batches(batches)
    mb = [2, 0, 1]
    fit, seq = e.evaluate(IT, 0, 3, SIGMA, return_seq=True, member_batch=mb)
    fit, seq = fit.cpu().numpy(), seq.cpu().numpy()
    for k in range(3):
        fc, gts = batches[mb[k]]
        for s, sign in enumerate((+1, -1)):
            oseq, _, fr = O.decode(dims, O.perturb(w['theta'], _table(), _idx(dims, k), SIGMA, sign), fc)
            assert _compare_tokens(seq[k, s], oseq, fr) == 0, (k, s)
            f_ref, _ = CR.rollout_fitness(w['scorer'], seq[k, s], gts)
            assert _close(fit[k, s], f_ref), (k, s)
        e.set_batch(fc, gts)
        alone = e.evaluate(IT, k, 1, SIGMA).cpu().numpy()
        assert np.array_equal(alone[0], fit[k]), k
        e.set_batches(batches)


@pytest.mark.parametrize('mode', ['greedy_logprob', 'greedy_expprob', 'greedy_linprob', 'greedy_avgprob'])
def test_wide_fitness_criteria_match_the_oracle(engines, mode):
    w = _world('a')
    e = engines('a')
    _load(e, w['theta'], w['fc'], w['gts'], w['df'], w['n'])
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
            assert not w['ofr'][k, s].any() and np.array_equal(seq[k, s], w['oseq'][k, s])
            _, scores = CR.rollout_fitness(w['scorer'], seq[k, s], w['gts'])
            f_own = CR.criterion_fitness(mode, lp[k, s], seq[k, s], scores)
            assert abs(fit[k, s] - f_own) <= 1e-6 * max(1.0, abs(f_own)), (k, s, fit[k, s], f_own)
            f_ora = CR.criterion_fitness(mode, w['olp'][k, s], w['oseq'][k, s], scores)
            assert abs(fit[k, s] - f_ora) <= 1e-5 * max(1.0, abs(f_ora)), (k, s, fit[k, s], f_ora)


@pytest.mark.parametrize('mode', ['scale', 'divide'], ids=['SM-PROPORTIONAL', 'SM-VECTOR'])
def test_wide_mutated_members_match_the_oracle(engines, mode):
    """The members' delta' rows are materialised whole (the NICNES_MUT_FULL arrangement): tokens, fitness and the
    noise vectors against the oracle's member_delta."""
    w = _world('a')
    dims, e, table = w['dims'], engines('a'), _table()
    theta = w['theta']
    _load(e, theta, w['fc'], w['gts'], w['df'], w['n'])
    try:
        if mode == 'scale':
            mean_abs = float(np.abs(theta).mean(dtype=np.float32))
            vec = np.where(theta == 0, np.float32(mean_abs), np.abs(theta)).astype(np.float32)
            e.set_mutation_proportional(mean_abs)
        else:
            vec = (0.5 + np.random.Generator(np.random.PCG64(3)).random(theta.size)).astype(np.float32)
            e.set_mutation('divide', vec)
        fit, seq = e.evaluate(IT, 0, 2, SIGMA, return_seq=True)
        fit, seq = fit.cpu().numpy(), seq.cpu().numpy()
        nv = e.noise_vectors(IT, 0, 2, SIGMA).cpu().numpy()
        differs = 0
        for k in range(2):
            assert np.array_equal(nv[k], O.member_delta(table, _idx(dims, k), SIGMA, dims.D, (mode, vec))), k
            for s, sign in enumerate((+1, -1)):
                oseq, _, fr = O.decode(dims, O.perturb(theta, table, _idx(dims, k), SIGMA, sign, (mode, vec)), w['fc'])
                assert _compare_tokens(seq[k, s], oseq, fr) == 0, (k, s)
                f_ref, _ = CR.rollout_fitness(w['scorer'], seq[k, s], w['gts'])
                assert _close(fit[k, s], f_ref), (k, s)
                differs += int(not np.array_equal(oseq, w['oseq'][k, s]))
        assert differs > 0                         # the mutation changes captions: not the plain members again
    finally:
        e.set_mutation('plain')


def test_wide_grad_partial_and_optimizers_bit_exact(engines, golden_dir):
    """rank_weights, grad_partial, Adam and SGD are D-generic: at D = 725,828 as at the default D
    (tests/test_gpu_parity.py)."""
    w = _world('a')
    dims, e, table = w['dims'], engines('a'), _table()
    e.set_mutation('plain')
    rng = np.random.default_rng(1)
    fit = rng.random((P, 2))
    w_ref, cr_ref = O.weights_from_fitness(fit)
    cr, wt = e.rank_weights(torch.from_numpy(fit).to(e.device))
    assert np.array_equal(cr.cpu().numpy(), cr_ref) and np.array_equal(wt.cpu().numpy(), w_ref)
    g = e.grad_partial(9, 0, P, wt, SIGMA).cpu().numpy()
    acc = np.zeros(dims.D, np.float64)
    for i in range(P):
        acc += np.float64(w_ref[i]) * O.member_delta(table, _idx(dims, i, 9), SIGMA, dims.D).astype(np.float64)
    assert np.array_equal(g, acc.astype(np.float32))

    def embed(arr, dtype):
        out = np.zeros(e.D, dtype)
        out[e.D - arr.size:] = arr                 # at the END of theta: past every default-D offset
        return out
    try:
        z = np.load(os.path.join(golden_dir, 'adam.npz'))
        n = z['theta0'].size
        e.set_theta(embed(z['theta0'], np.float32))
        e.set_adam_state(np.zeros(e.D), np.zeros(e.D), 0)
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
        e.set_adam_state(np.zeros(e.D), np.zeros(e.D), 0)
        for k in range(3):
            ratio = e.sgd_step(torch.from_numpy(embed(z['grads'][k] * np.float32(2.0), np.float32)).to(e.device), 1,
                               float(z['l2coeff']), float(z['stepsize']), float(z['momentum']))
            t64, t32 = e.theta()
            assert np.array_equal(t64.cpu().numpy()[-n:], z['thetas'][k]), k
            assert np.array_equal(t32.cpu().numpy()[-n:], z['thetas'][k].astype(np.float32))
            assert ratio > 0
    finally:
        e.set_theta(w['theta'])
        e.set_adam_state(np.zeros(e.D), np.zeros(e.D), 0)


class _Labels:
    def __init__(self, gts):
        self.labels = np.concatenate(gts, 0)
        n = np.array([g.shape[0] for g in gts])
        self.label_start_ix = np.cumsum(np.concatenate([[0], n[:-1]])) + 1      # 1-based, inclusive
        self.label_end_ix = self.label_start_ix + n - 1


class _Loader:
    """the surface of nicnes.data.CocoFcDataLoader a Validator and the master read (tests/test_gpu_validation_master.py)"""

    def __init__(self, fc, gts, n_val, vocab):
        self.fc, self.gts, self.pos, self.seq_length = fc, gts, 0, 16
        self.labels = _Labels(gts)
        n = len(gts)
        self.info = {'images': [{'id': 1000 + i} for i in range(n)]}
        self.ix_to_word = {str(i): 'w%d' % i for i in range(1, vocab + 1)}
        self.split_ix = {'val': list(range(n - n_val, n)), 'train': list(range(n - n_val))}

    def fc_feature(self, ix):
        return self.fc[ix]

    def get_batch(self, split, batch_size=None):
        tr = self.split_ix['train']
        ix = [tr[(self.pos + k) % len(tr)] for k in range(batch_size)]
        self.pos += batch_size
        return {'fc_feats': np.repeat(self.fc[ix], 5, axis=0), 'gts': [self.gts[i] for i in ix]}


def test_wide_master_two_iterations_with_a_validator(tmp_path):
    """EngineMaster.run at E = R = 256 with a Validator on the engine against the same run on the oracle engine
    (tests/cpu_engine.py; validation reads theta and touches nothing the evaluates use): fitness 1e-9, theta / m / v 1e-6."""
    import nicnes
    import nicnes.synthetic as S
    from nicnes import config as C, master as M
    from nicnes.validation import Validator
    from tests.cpu_engine import OracleEngine
    dims = O.Dims(vocab_size=67, E=256, R=256, F=128)
    theta = O.make_theta(dims, 0, 4.0, 0.1)
    fc = np.random.Generator(np.random.PCG64(1234)).standard_normal((27, dims.F)).astype(np.float32)
    base, _, _ = O.decode(dims, theta, fc)
    gts, df, n = S.build_references(base, dims.vocab_size, seed=9, n_refs=5, df_sets=128)
    table = _table(1 << 21)
    Pm = 4

    def spec():
        return C.ExperimentSpec({
            'algorithm': 'nic_nes', 'nb_offspring': Pm,
            'config': {'noise_stdev': 0.01, 'batch_size': 8, 'l2coeff': 1e-3, 'snapshot_freq': 0, 'single_batch': True,
                       'patience': 5, 'num_val_items': 9},
            'policy_options': {'net': 'fc_caption', 'fitness': 'greedy',
                               'model_options': {'rnn_size': 256, 'input_encoding_size': 256, 'fc_feat_size': 128}},
            'optimizer_options': {'type': 'adam', 'args': {'stepsize': 1e-2}}}, vocab_size=67)
    kw = spec().engine_kwargs(max_members=Pm, noise_len=1 << 21, noise_seed=0, max_batch=8)
    e = nicnes.Engine(**kw)
    try:
        assert e.D == dims.D and e.decode_path(8, Pm) == 'wide'
        e.set_noise_table(table)
        keys, vals = nicnes.df_table_arrays(df)
        e.set_df_table(keys, vals, np.log(float(n)))
        la, lb = _Loader(fc, gts, 11, 67), _Loader(fc, gts, 11, 67)
        v = Validator(e, la, 'val', 9)
        gpu = M.EngineMaster(spec(), e, log_dir=str(tmp_path / 'gpu'), theta=theta, validator=v)
        ora_e = OracleEngine(dims, theta, fc, gts, df, n, table, noise_seed=0)
        ora = M.EngineMaster(spec(), ora_e, log_dir=str(tmp_path / 'ora'), theta=theta)
        gpu.run(la, max_iterations=2)
        ora.run(lb, max_iterations=2)
        assert len(gpu.stats) == len(ora.stats) == 2
        for a, b in zip(gpu.stats, ora.stats):
            for k in ('score_mean', 'score_max', 'score_min'):
                assert abs(a[k] - b[k]) <= 1e-9 * max(1.0, abs(b[k])), (k, a[k], b[k])
            assert np.isfinite(a['val_score']) and a['val_score'] > 0
        assert np.allclose(e.theta()[0].cpu().numpy(), ora_e.adam.theta, rtol=1e-6, atol=1e-12)
        m, vv, t = e.adam_state()
        assert t == 2 and np.allclose(m.cpu().numpy(), ora_e.adam.m, rtol=1e-6, atol=1e-15)
        assert np.allclose(vv.cpu().numpy(), ora_e.adam.v, rtol=1e-6, atol=1e-20)
    finally:
        e.close()


def test_wide_worker_process_serves_engine_master(tmp_path):
    """`python -m nicnes.worker` at E = R = 256 (the default engine factory builds its Engine from the experiment's
    model_options): two dispatched iterations give the theta of the local loop on the same inputs, as at the default
    widths (tests/test_gpu_worker.py)."""
    import signal
    import socket
    import subprocess
    import sys
    import nicnes
    import nicnes.synthetic as S
    from nicnes import config as C, data, master as M, transport as T
    from nicnes.worker import STOP_KEY
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dims = O.Dims(vocab_size=67, E=256, R=256, F=128)
    theta = O.make_theta(dims, 2, 4.0, 0.1)
    Pm, B, n_len = 8, 12, 1 << 21
    fc = np.random.Generator(np.random.PCG64(77)).standard_normal((B, dims.F)).astype(np.float32)
    base, _, _ = O.decode(dims, theta, fc)
    gts, df, n = S.build_references(base, dims.vocab_size, seed=5, n_refs=5, df_sets=128)
    batch = {'fc_feats': fc, 'gts': gts}

    def spec():
        return C.ExperimentSpec({
            'algorithm': 'nic_nes', 'nb_offspring': Pm,
            'config': {'noise_stdev': 0.01, 'batch_size': B, 'l2coeff': 1e-7, 'snapshot_freq': 0},
            'policy_options': {'net': 'fc_caption', 'fitness': 'greedy',
                               'model_options': {'rnn_size': 256, 'input_encoding_size': 256, 'fc_feat_size': 128}},
            'optimizer_options': {'type': 'adam', 'args': {'stepsize': 1e-3}}}, vocab_size=67)
    e = nicnes.Engine(**spec().engine_kwargs(max_members=Pm, noise_len=n_len, noise_seed=0, max_batch=B))
    try:
        e.set_noise_table(_table(n_len))
        keys, vals = nicnes.df_table_arrays(df)
        e.set_df_table(keys, vals, np.log(float(n)))
        assert e.decode_path(B, Pm) == 'wide'
        local = M.EngineMaster(spec(), e, log_dir=str(tmp_path / 'a'), theta=theta)
        local.run([batch] * 2, max_iterations=2)
        want = e.theta()[0].cpu().numpy()
        assert not np.array_equal(want.astype(np.float32), theta)
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


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_wide_refusals_leave_the_handle_usable(engines):
    import nicnes
    w = _world('a')
    dims, e = w['dims'], engines('a')
    _load(e, w['theta'], w['fc'], w['gts'], w['df'], w['n'])
    want = e.evaluate(IT, 0, 2, SIGMA).cpu().numpy()
    split = e.make_split(w['fc'], w['gts'])
    h_rows = np.zeros((32, dims.R), np.float32)
    refused = [
        lambda: e.set_fitness_mode('sample'),
        lambda: e.set_fitness_mode('self_critical'),
        lambda: e.set_fitness_mode('sc_loss'),
        lambda: e.sum_sensitivity(8, 0.01),
        lambda: e.es_create(4, 1),
        lambda: split.decode_beam(beam_size=3),
        lambda: split.evaluate(beam_size=2),
        lambda: e.test_logit_chain(IT, 0, SIGMA, 0, h_rows),
        lambda: e.test_certify_items(IT, 0, SIGMA, 0, np.zeros((128, dims.R), np.float32), np.array([[0, 1]], np.int32)),
        lambda: e.set_decode_split(4, 4),
        lambda: e.set_decode_split(2, 4),
        lambda: e.set_decode_split(1, 2),
        lambda: e.set_decode_streams(2),
    ]
    try:
        for i, call in enumerate(refused):
            with pytest.raises(nicnes.NicnesError, match='not supported'):
                call()
            assert e.decode_path(40, 2) == 'wide', i
            assert np.array_equal(e.evaluate(IT, 0, 2, SIGMA).cpu().numpy(), want), i
        # what stays allowed: the automatic shape, the fused shape it is, one stream, the coop switch (never taken)
        e.set_decode_split(0, 0)
        e.set_decode_split(1, 4)
        e.set_decode_streams(1)
        e.set_decode_streams(0)
        e.set_decode_coop(0)
        e.set_decode_coop(1)
        assert torch.equal(split.decode(), e.evaluate_theta(0, return_seq=True)[1])
        assert np.array_equal(e.evaluate(IT, 0, 2, SIGMA).cpu().numpy(), want)
    finally:
        split.close()
        e.set_decode_split(0, 0)
        e.set_fitness_mode('greedy')


@pytest.mark.parametrize('E,R', [(64, 128), (128, 64), (192, 128), (128, 192), (640, 128), (128, 640), (256, 200)])
def test_create_refuses_other_widths(E, R):
    import nicnes
    with pytest.raises(nicnes.NicnesError, match='not supported'):
        nicnes.Engine(vocab_size=67, input_encoding_size=E, rnn_size=R, fc_feat_size=128, max_batch=8, max_members=2,
                      noise_len=1 << 21)
