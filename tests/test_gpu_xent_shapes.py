"""GPU: the teacher-forced forward (csrc/xent_kernels.hip) on the paths tests/test_gpu_xent.py's shapes leave out, against
tests/xent_ref.py. The worlds and what each reaches are in tests/xent_worlds.py; tests/test_xent_worlds_host.py holds
them to their preconditions on the CPU.

  image projection at F = 256, 384, 2048 (nK = 2, 3, 16)           M1, M4, M2, S2
  more than 256 rows per candidate (the reduce loop's later passes)  M1 (300), M3 (513), S1, H1
  three and five slabs, a batch that skips whole slabs, nslabs below what the stride implies   M1, M3
  flat ranges of 2..5 pseudo-members, row0 > 0 off a slab edge, one-row halves    S1, S2, H1
  a pseudo-member of 256 different images; an image over a pseudo-member boundary   S1
  evaluate_theta(k) / test_xent_steps(theta_batch=k) for k > 0       H1
  member windows (member_begin > 0, count = max_members)             M1
  batches drawn on the GPU, a draw that outgrows max_refs             D
  one handle's buffers growing and shrinking                          G, S1
  label rows with a 0 inside                                          M4

Bars (the project's own): per-step log-prob 1e-5 absolute; n_tok exact; lp_sum the fp64 re-sum of the returned steps bit
for bit, and (T + 1) x 1e-5 where only sums come back; fitness and loss 1e-5 absolute; fitness and loss against the host
emulation of the device's reduce order (xent_worlds.reduce_order) bit for bit."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from tests import xent_ref as X                                 # noqa: E402
from tests import xent_worlds as W                              # noqa: E402

IT, P, SIGMA, LP_BAR = W.IT, W.P, W.SIGMA, W.LP_BAR


def _df(e, batches):
    """any df table: the engine wants one before a batch (the CIDEr-D side of the batch is cooked whatever the mode)"""
    from nicnes.validation import corpus_df
    rows = [g for _, gts in batches for g in gts]
    keys, vals = corpus_df(rows, e.cfg.seq_length)
    e.set_df_table(keys, vals, float(np.log(float(len(rows)))))


def _engine(dims, theta, max_batch=64, max_refs=256):
    import nicnes
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    e = nicnes.Engine(vocab_size=dims.vocab_size, fc_feat_size=dims.F, seq_length=dims.T, max_batch=max_batch,
                      max_refs=max_refs, max_members=4, noise_len=W.NOISE_LEN, noise_seed=W.SEED)
    e.set_noise_table(W.table())
    e.set_theta(theta)
    return e


def _batch_engine(dims, theta, batches, **kw):
    e = _engine(dims, theta, **kw)
    _df(e, batches)
    e.set_batches(batches)
    e.set_fitness_mode('xent')
    return e


def _np(*ts):
    out = tuple(t.cpu().numpy() for t in ts)
    return out if len(out) > 1 else out[0]


def _resum(steps, mask):
    """the fp64 sum of the counted steps in step order"""
    acc = np.zeros(steps.shape[0], np.float64)
    for t in range(steps.shape[1]):
        acc = np.where(mask[:, t], acc + steps[:, t].astype(np.float64), acc)
    return acc


def _check_candidate(r, steps, lp_sum, n_tok, fit, what):
    """one candidate against its restatement r: the assertions of test_gpu_xent's first test, and the reduce order.
    steps [stride, T + 1] as the test entry returned them. Returns the largest |lp - restatement|."""
    n = r['lp'].shape[0]
    got = steps[:n]
    assert np.array_equal(got != 0, r['mask'] & (got != 0)), ('a step that does not count was written', what)
    assert np.array_equal(got != 0, r['mask']), ('a step that counts was not written', what)
    err = np.abs(got.astype(np.float64) - r['lp'])[r['mask']].max()
    assert err <= LP_BAR, (what, err)
    assert (steps[n:] == 0).all(), ('rows past the batch were written', what)
    assert np.array_equal(n_tok, r['n_tok']), what
    assert np.array_equal(lp_sum, _resum(got, r['mask'])), ('lp_sum is not the fp64 sum of the steps in step order', what)
    assert abs(fit - r['fit']) <= 1e-5, (what, fit, r['fit'])
    assert fit == W.reduce_fitness(lp_sum, n_tok), ('fitness is not the reduce order over the device rows', what)
    return err


# ---- 1, 2, 8: members --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def member_engines():
    made = {}

    def get(name):
        if name not in made:
            w = W.member_inputs(name)
            made[name] = _batch_engine(w['dims'], w['theta'], w['batches'])
        return made[name]
    yield get
    for e in made.values():
        e.close()


def _member_run(e, mb, count=P, begin=0):
    """evaluate, every candidate's rows, the evaluate again"""
    fit = e.evaluate(IT, begin, count, SIGMA, member_batch=mb)
    rows = {(k, s): _np(*e.xent_rows(2 * k + s, mb[k] if mb else 0)) for k in range(count) for s in (0, 1)}
    again = e.evaluate(IT, begin, count, SIGMA, member_batch=mb)
    assert torch.equal(fit, again), 'two runs differ'
    return _np(fit), rows


@pytest.mark.parametrize('name', sorted(W.MEMBER_WORLDS))
def test_members_against_the_restatement(member_engines, name):
    w, e = W.member_world(name), member_engines(name)
    mb = w['mb']
    fit_s, lp = _np(*e.test_xent_steps(IT, 0, P, SIGMA, member_batch=mb))
    fit, rows = _member_run(e, mb)
    assert np.array_equal(fit, fit_s), 'the test entry and evaluate differ'
    worst = 0.0
    for k in range(P):
        for s in (0, 1):
            lp_sum, n_tok = rows[k, s]
            worst = max(worst, _check_candidate(w['ref'][k, s], lp[k, s], lp_sum, n_tok, fit[k, s], (name, k, s)))
    print('world %s: largest |lp - restatement| %.3g' % (name, worst))
    if name == 'M3':
        # every member on the 257-row batch: three slabs under the stride of 513
        one = [1] * P
        fit1, rows1 = _member_run(e, one)
        _, lp1 = _np(*e.test_xent_steps(IT, 0, P, SIGMA, member_batch=one))
        for k in (1, 3):
            assert np.array_equal(fit1[k], fit[k]), 'a member on batch 1 depends on the other members\' batches'
            for s in (0, 1):
                assert np.array_equal(rows1[k, s][0], rows[k, s][0]) and np.array_equal(rows1[k, s][1], rows[k, s][1])
                assert np.array_equal(lp1[k, s], lp[k, s])
        for k in (0, 2):                         # and the others, now on batch 1, against their own rows' reduce order
            for s in (0, 1):
                assert rows1[k, s][0].shape == (257,)
                assert fit1[k, s] == W.reduce_fitness(*rows1[k, s])
                assert np.array_equal(rows1[k, s][1], w['ref'][1, 0]['n_tok'])


def test_member_windows(member_engines):
    from nicnes._lib import NicnesError
    e = member_engines('M1')
    assert e.cfg.max_members == P
    full, rows_full = _member_run(e, None)                    # count = max_members
    assert np.isfinite(full).all()
    part, rows_part = _member_run(e, None, count=2, begin=2)
    assert np.array_equal(part, full[2:4]), 'a member depends on the window it is evaluated in'
    for k in (0, 1):
        for s in (0, 1):
            for a, b in zip(rows_part[k, s], rows_full[k + 2, s]):
                assert np.array_equal(a, b)
    one, _ = _member_run(e, None, count=1, begin=3)
    assert np.array_equal(one[0], full[3])
    with pytest.raises(NicnesError, match='max_members'):
        e.evaluate(IT, 0, P + 1, SIGMA)
    again, _ = _member_run(e, None)
    assert np.array_equal(again, full), 'the handle after a refused count'


@pytest.mark.parametrize('kind', [k for k in W.M4_KINDS if k != 'plain'])
def test_rows_with_zeros_inside_count_their_steps(member_engines, kind):
    """each row kind of M4 by name: the steps the device wrote and its n_tok are the kind's, for every candidate"""
    w, e = W.member_inputs('M4'), member_engines('M4')
    T = w['dims'].T
    want = W.m4_counted(kind, T)
    at = [r for r, k in W.M4_AT.items() if k == kind]
    assert len(at) == 3
    _, lp = _np(*e.test_xent_steps(IT, 0, P, SIGMA))
    e.evaluate(IT, 0, P, SIGMA)
    for k in range(P):
        for s in (0, 1):
            _, n_tok = _np(*e.xent_rows(2 * k + s))
            for r in at:
                assert np.flatnonzero(lp[k, s, r]).tolist() == want, (kind, r, k, s)
                assert n_tok[r] == len(want), (kind, r, k, s)


# ---- 3, 4: flat ranges ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def flat():
    made = {}

    def get(name):
        if name not in made:
            w = W.flat_inputs(name)
            e = _engine(w['dims'], w['theta'])
            made[name] = (e, e.make_split(w['fc'], w['gts']))
        return made[name]
    yield get
    for e, sp in made.values():
        sp.close()
        e.close()


FLAT_RANGES = [('S1', n) for n in sorted(W.S1_RANGES)] + [('S2', 'whole')]


@pytest.mark.parametrize('name,rng', FLAT_RANGES)
def test_flat_range_against_the_restatement(flat, name, rng):
    w = W.flat_world(name)
    _, sp = flat(name)
    first, count = w['ranges'][rng]
    r0, r1 = int(w['starts'][first]), int(w['starts'][first + count])
    ref_lp, ref_nt = w['ref']['lp_sum'][r0:r1], w['ref']['n_tok'][r0:r1]
    x = sp.xent(first, count)
    x2 = sp.xent(first, count)
    lp_sum, n_tok = _np(x['lp_sum'], x['n_tok'])
    assert lp_sum.shape == (r1 - r0,)
    assert np.array_equal(n_tok, ref_nt)
    err = np.abs(lp_sum - ref_lp).max()
    print('%s %s: largest |lp_sum - restatement| %.3g over %d rows' % (name, rng, err, r1 - r0))
    assert err <= (w['dims'].T + 1) * LP_BAR
    assert x['tokens'] == int(ref_nt.sum())
    assert abs(x['loss'] - X.loss_of(ref_lp, ref_nt)) <= 1e-5
    assert x['perplexity'] == pytest.approx(np.exp(x['loss']), rel=1e-12)
    assert x['loss'] == -W.reduce_fitness(lp_sum, n_tok), 'loss is not the reduce order over the returned rows'
    assert x2['loss'] == x['loss'] and x2['perplexity'] == x['perplexity'] and x2['tokens'] == x['tokens']
    assert torch.equal(x2['lp_sum'], x['lp_sum']) and torch.equal(x2['n_tok'], x['n_tok'])


def test_a_row_does_not_depend_on_where_it_lands():
    """small ranges, the whole split, the small ranges again, on a fresh split (its work buffers grow in between): a
    row's lp_sum and n_tok are the same bits in whichever pseudo-member, sign half, wave and image window it runs"""
    w = W.flat_inputs('S1')
    e = _engine(w['dims'], w['theta'])
    sp = e.make_split(w['fc'], w['gts'])
    try:
        names = [n for n in sorted(W.S1_RANGES) if n != 'whole']

        def run(n):
            x = sp.xent(*w['ranges'][n])
            return x['loss'], x['tokens'], _np(x['lp_sum']), _np(x['n_tok'])
        before = {n: run(n) for n in names}
        whole = run('whole')
        after = {n: run(n) for n in reversed(names)}
        for n in names:
            first, count = w['ranges'][n]
            r0, r1 = int(w['starts'][first]), int(w['starts'][first + count])
            for got in (before[n], after[n]):
                assert np.array_equal(got[2], whole[2][r0:r1]), n
                assert np.array_equal(got[3], whole[3][r0:r1]), n
            assert before[n][0] == after[n][0] and before[n][1] == after[n][1], n
        assert whole[2].shape == (int(w['starts'][-1]),)
    finally:
        sp.close()
        e.close()


# ---- 5: the handle's own flat path -----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def h1_engine():
    w = W.h1_inputs()
    e = _batch_engine(w['dims'], w['theta'], w['batches'])
    yield e
    e.close()


@pytest.mark.parametrize('k', [0, 1, 2])
def test_theta_on_batch_k_of_the_handle(h1_engine, k):
    w, e = W.h1_world(), h1_engine
    r = w['ref'][k]
    fc, gts = w['batches'][k]
    fit_s, steps = _np(*e.test_xent_steps(theta_batch=k))
    assert steps.shape == r['lp'].shape
    assert np.array_equal(steps != 0, r['mask']), 'written only where counted, and everywhere counted'
    err = np.abs(steps.astype(np.float64) - r['lp'])[r['mask']].max()
    print('H1 batch %d: largest |lp - restatement| %.3g' % (k, err))
    assert err <= LP_BAR
    lp_s, nt_s = e.xent_rows(0, k)
    ft = e.evaluate_theta(k)
    lp_t, nt_t = e.xent_rows(0, k)
    f0 = e.evaluate(IT, 0, 1, 0.0, member_batch=[k])
    lp_0, nt_0 = e.xent_rows(0, k)
    lp_1, nt_1 = e.xent_rows(1, k)
    sp = e.make_split(fc, gts)
    try:
        x = sp.xent()
    finally:
        sp.close()
    assert float(ft[0]) == float(fit_s[0]) == float(f0[0, 0]) == float(f0[0, 1]) == -x['loss']
    for lp_, nt_ in ((lp_s, nt_s), (lp_0, nt_0), (lp_1, nt_1), (x['lp_sum'], x['n_tok'])):
        assert torch.equal(lp_t, lp_) and torch.equal(nt_t, nt_)
    lp_t, nt_t = _np(lp_t, nt_t)
    assert np.array_equal(nt_t, r['n_tok']) and x['tokens'] == int(r['n_tok'].sum())
    assert np.array_equal(lp_t, _resum(steps, r['mask']))
    assert abs(float(ft[0]) - r['fit']) <= 1e-5
    assert float(ft[0]) == W.reduce_fitness(lp_t, nt_t)


# ---- 6: drawn batches ------------------------------------------------------------------------------------------------------
def test_drawn_batches_against_set_batches_and_the_restatement():
    w = W.drawn_world()
    M = W.D['members']
    mb = list(range(M))
    n_first = sum(W.draw_rows('first'))
    assert sum(W.draw_rows('large')) > n_first + 8
    drawn = _engine(w['dims'], w['theta'], max_refs=n_first + 8)       # the second draw outgrows it
    given = _engine(w['dims'], w['theta'], max_refs=1024)
    ts = None
    try:
        for e in (drawn, given):
            _df(e, [(w['fc'], w['gts'])])
            e.set_fitness_mode('xent')
        ts = drawn.make_trainset(w['fc'], w['gts'])

        def run(e):
            fit_s, lp = _np(*e.test_xent_steps(IT, 0, M, SIGMA, member_batch=mb))
            fit = _np(e.evaluate(IT, 0, M, SIGMA, member_batch=mb))
            rows = {(k, s): _np(*e.xent_rows(2 * k + s, k)) for k in range(M) for s in (0, 1)}
            assert np.array_equal(fit, fit_s)
            return fit, lp, rows

        def same(a, b, what):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what
            for key in a[2]:
                assert np.array_equal(a[2][key][0], b[2][key][0]) and np.array_equal(a[2][key][1], b[2][key][1]), what

        got = {}
        for name in ('first', 'large', 'first'):
            drawn.draw_batches(ts, np.array(W.DRAWS[name], np.int32))
            assert [drawn.xent_batch_rows(b) for b in range(2)] == W.draw_rows(name)
            a = run(drawn)
            given.set_batches(w['host'][name])
            b = run(given)
            same(a, b, 'draw %s: drawn and given batches differ' % name)
            fit, lp, rows = a
            worst = max(_check_candidate(w['ref'][name][k, s], lp[k, s], rows[k, s][0], rows[k, s][1], fit[k, s],
                                         (name, k, s)) for k in range(M) for s in (0, 1))
            print('draw %s: largest |lp - restatement| %.3g' % (name, worst))
            if name in got:
                same(a, got[name], 'the first draw again')
            got[name] = a
    finally:
        if ts is not None:
            ts.close()
        drawn.close()
        given.close()


# ---- 7: one handle, growing and shrinking -----------------------------------------------------------------------------------
def test_one_handle_growing_and_shrinking():
    w = W.grow_inputs()

    def run(e, rows):
        fit = e.evaluate(IT, 0, 2, SIGMA)
        cand = [_np(*e.xent_rows(c)) for c in range(4)]
        ft = e.evaluate_theta(0)
        th = _np(*e.xent_rows(0))
        assert all(a.shape == (rows,) and b.shape == (rows,) for a, b in cand + [th])
        return _np(fit), cand, float(ft[0]), th

    one = _engine(w['dims'], w['theta'])
    try:
        _df(one, w['batches'])
        one.set_fitness_mode('xent')
        for batch, rows in zip(w['batches'], W.G_ROWS):
            one.set_batches([batch])
            assert one.xent_batch_rows(0) == rows
            got = run(one, rows)
            fresh = _batch_engine(w['dims'], w['theta'], [batch])
            try:
                want = run(fresh, rows)
            finally:
                fresh.close()
            assert np.array_equal(got[0], want[0]) and got[2] == want[2], rows
            for (a, b), (c, d) in zip(got[1] + [got[3]], want[1] + [want[3]]):
                assert np.array_equal(a, c) and np.array_equal(b, d), rows
            _, lab, _ = X.rows_of(*batch)
            assert np.array_equal(got[3][1], X.counted(lab).sum(1)), 'n_tok of theta on this batch'
            assert got[2] == W.reduce_fitness(*got[3])
            for c in range(4):
                assert got[0][c >> 1, c & 1] == W.reduce_fitness(*got[1][c])
        # after the 5-row batch nothing of the 513-row one can be read
        from nicnes._lib import NicnesError, check
        from nicnes.engine import _ptr
        lp = torch.empty(6, dtype=torch.float64, device=one.device)
        nt = torch.empty(6, dtype=torch.int32, device=one.device)
        with pytest.raises(NicnesError, match='outside the last xent evaluate'):
            check(one.L.nicnes_xent_rows(one.h, 0, 6, _ptr(lp), _ptr(nt), one._stream()), one.h, 'xent_rows')
    finally:
        one.close()
