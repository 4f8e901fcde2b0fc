"""GPU: the teacher-forced forward (csrc/xent_kernels.hip) behind the C ABI: NICNES_FITNESS_XENT on nicnes_evaluate*,
nicnes_evaluate_theta, nicnes_split_xent, the per-row read-back and the per-step test entry, against tests/xent_ref.py
(the host restatement tests/test_xent_host.py pins to the imported reference and to the oracle's decode).

Bars: per-step log-probs 1e-5 absolute, the project's log-prob bar (tests/test_gpu_parity.py); n_tok exact; lp_sum the
fp64 re-sum of the returned steps bit for bit; fitness 1e-5 absolute (a mean of log-probs each within 1e-5); two runs the
same bits; theta three ways (Split.xent, evaluate_theta, the sigma = 0 member) the same bits.

Cases (F = 128, three members, sigma 0.01; images of 1..7 label rows throughout):
  a  V1 8     T 16  130 rows  two slabs with a 2-row tail; the first slab's 128 rows are one word long (they all end at
                              step 1) beside a second slab whose two rows run all T + 1 steps
  b  V1 68    T 16  128 rows  the last logit stage 4 ids wide; rows of 0, 1, 5 and 16 words; two batches, per member
  c  V1 200   T 3   33 rows   four stages, the last 8 wide
  d  V1 9488  T 3   33 rows   the workload's vocabulary
  e  V1 68    T 1   1 row     one image, one row, one word
Targets are planted at ids 0, 3, 4, 31, 32, 63, 64 and V1 - 1 (those below V1), so every lane half ((id >> 2) & 1), both
32-id tiles of a stage, the first and the last stage and the partial one own a target.
Other F, more rows, slabs, pseudo-members, windows, draws and zeros inside labels: tests/test_gpu_xent_shapes.py."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from oracle import oracle as O                                  # noqa: E402
from tests import xent_ref as X                                 # noqa: E402
from tests.cpu_engine import OracleEngine                       # noqa: E402

NOISE_LEN = 1 << 23
SEED = 7
SIGMA = 0.01
IT = 3
P = 3
LP_BAR = 1e-5

CASES = {
    'a': dict(vocab=7, T=16, rows=130),
    'b': dict(vocab=67, T=16, rows=128, batches=2),
    'c': dict(vocab=199, T=3, rows=33),
    'd': dict(vocab=9487, T=3, rows=33),
    'e': dict(vocab=67, T=1, rows=1),
}
PLANT = (3, 4, 31, 32, 63, 64)

_cache = {}


def _dims(case):
    c = CASES[case]
    return O.Dims(vocab_size=c['vocab'], F=128, T=c['T'])


def _table():
    if 'table' not in _cache:
        _cache['table'] = O.noise_table(NOISE_LEN, 123)
    return _cache['table']


def _labels(case, n_rows, rng):
    """label rows [n_rows, T]: lengths cycling through 0, 1, 5, T (cut to T), words random with the planted ids"""
    c = CASES[case]
    V, T = c['vocab'], c['T']
    plant = [v for v in PLANT if v <= V] + [V]
    lab = np.zeros((n_rows, T), np.int32)
    for r in range(n_rows):
        n = min((0, 1, 5, T)[r % 4], T)
        if case == 'a':
            n = 1 if r < 128 else T
        if case == 'e':
            n = 1
        w = rng.integers(1, V + 1, n)
        for j in range(n):                       # every third word a planted id, walking through them
            if (r + j) % 3 == 0:
                w[j] = plant[(r + j) // 3 % len(plant)]
        lab[r, :n] = w
    return lab


def _batch(case, seed):
    """(fc [B, F], gts): images of 1..7 label rows until the case's row count is reached"""
    c = CASES[case]
    rng = np.random.Generator(np.random.PCG64(seed))
    lab = _labels(case, c['rows'], rng)
    gts, at, k = [], 0, 0
    while at < c['rows']:
        n = min(1 + k % 7, c['rows'] - at)
        gts.append(lab[at:at + n])
        at += n
        k += 1
    fc = rng.standard_normal((len(gts), 128)).astype(np.float32)
    return fc, gts


def _world(case):
    """The host's side, computed once and never modified: theta, the batches, and for every member and sign the
    restatement's per-step log-probs, lp_sum, n_tok and fitness on the member's batch."""
    if case not in _cache:
        c, dims = CASES[case], _dims(case)
        theta = O.make_theta(dims, 0, 4.0, 0.1)
        batches = [_batch(case, 500 + 10 * i) for i in range(c.get('batches', 1))]
        if len(batches) == 2:                    # the second batch one row shorter: the stride is the larger one's
            fc, gts = batches[1]
            j = max(i for i, g in enumerate(gts) if g.shape[0] > 1)
            batches[1] = (fc, gts[:j] + [gts[j][:-1]] + gts[j + 1:])
        mb = [k % len(batches) for k in range(P)]
        ref = {}
        for k in range(P):
            idx = O.noise_index(SEED, IT, k, NOISE_LEN, dims.D)
            fr, lab, _ = X.rows_of(*batches[mb[k]])
            for s, sign in enumerate((+1, -1)):
                lp, lp_sum, n_tok = X.forced(dims, O.perturb(theta, _table(), idx, SIGMA, sign), fr, lab)
                ref[k, s] = dict(lp=lp, lp_sum=lp_sum, n_tok=n_tok, fit=-X.loss_of(lp_sum, n_tok), mask=X.counted(lab))
        fr, lab, _ = X.rows_of(*batches[0])
        lp, lp_sum, n_tok = X.forced(dims, theta, fr, lab)
        ref['theta'] = dict(lp=lp, lp_sum=lp_sum, n_tok=n_tok, fit=-X.loss_of(lp_sum, n_tok), mask=X.counted(lab))
        for r in ref.values():
            for a in r.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _cache[case] = dict(dims=dims, theta=theta, batches=batches, mb=mb, ref=ref)
    return _cache[case]


def _df(e, batches):
    """any df table: the engine wants one before a batch (the CIDEr-D side of the batch is cooked whatever the mode)"""
    from nicnes.validation import corpus_df
    rows = [g for _, gts in batches for g in gts]
    keys, vals = corpus_df(rows, e.cfg.seq_length)
    e.set_df_table(keys, vals, float(np.log(float(len(rows)))))


def _engine(case, **kw):
    import nicnes
    c = CASES[case]
    e = nicnes.Engine(vocab_size=c['vocab'], fc_feat_size=128, seq_length=c['T'], max_batch=64, max_refs=256,
                      max_members=4, noise_len=NOISE_LEN, noise_seed=SEED, **kw)
    e.set_noise_table(_table())
    return e


@pytest.fixture(scope='module')
def engines():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    made = {}

    def get(case):
        if case not in made:
            w = _world(case)
            e = _engine(case)
            e.set_theta(w['theta'])
            _df(e, w['batches'])
            e.set_batches(w['batches'])
            e.set_fitness_mode('xent')
            made[case] = e
        return made[case]
    yield get
    for e in made.values():
        e.close()


@pytest.mark.parametrize('case', sorted(CASES))
def test_steps_rows_and_fitness_against_the_restatement(engines, case):
    w, e = _world(case), engines(case)
    mb = w['mb'] if len(w['batches']) > 1 else None
    fit, lp = e.test_xent_steps(IT, 0, P, SIGMA, member_batch=mb)
    fit, lp = fit.cpu().numpy(), lp.cpu().numpy()
    fit2 = e.evaluate(IT, 0, P, SIGMA, member_batch=mb)
    rows_dev = {(k, s): [a.cpu().numpy() for a in e.xent_rows(2 * k + s, w['mb'][k])] for k in range(P) for s in (0, 1)}
    fit3 = e.evaluate(IT, 0, P, SIGMA, member_batch=mb)
    assert torch.equal(fit2, fit3) and np.array_equal(fit2.cpu().numpy(), fit), 'two runs differ'
    worst = 0.0
    for k in range(P):
        for s in (0, 1):
            r = w['ref'][k, s]
            n = r['lp'].shape[0]
            got = lp[k, s, :n]
            assert np.array_equal(got != 0, r['mask'] & (got != 0)), 'a step that does not count was written'
            err = np.abs(got.astype(np.float64) - r['lp'])[r['mask']].max()
            worst = max(worst, err)
            assert err <= LP_BAR, (case, k, s, err)
            assert (lp[k, s, n:] == 0).all()
            lp_sum, n_tok = rows_dev[k, s]
            assert np.array_equal(n_tok, r['n_tok'])
            resum = np.zeros(n, np.float64)
            for t in range(got.shape[1]):            # step order
                resum = np.where(r['mask'][:, t], resum + got[:, t].astype(np.float64), resum)
            assert np.array_equal(lp_sum, resum), 'lp_sum is not the fp64 sum of the steps in step order'
            assert abs(fit[k, s] - r['fit']) <= 1e-5, (case, k, s, fit[k, s], r['fit'])
            assert fit[k, s] == lp_sum.sum() / n_tok.sum() or abs(fit[k, s] - lp_sum.sum() / n_tok.sum()) < 1e-12
    print('case %s: largest |lp - restatement| %.3g' % (case, worst))


@pytest.mark.parametrize('case', ['a', 'b', 'e'])
def test_theta_three_ways_bit_for_bit(engines, case):
    w, e = _world(case), engines(case)
    fc, gts = w['batches'][0]
    ft = e.evaluate_theta(0)
    lp_t, nt_t = e.xent_rows(0, 0)
    f0 = e.evaluate(IT, 0, 1, 0.0, member_batch=[0] if len(w['batches']) > 1 else None)
    lp_0, nt_0 = e.xent_rows(0, 0)
    sp = e.make_split(fc, gts)
    try:
        x = sp.xent()
        x2 = sp.xent()
    finally:
        pass
    r = w['ref']['theta']
    assert float(ft[0]) == float(f0[0, 0]) == float(f0[0, 1]) == -x['loss'] == -x2['loss']
    assert torch.equal(lp_t, lp_0) and torch.equal(lp_t, x['lp_sum']) and torch.equal(x['lp_sum'], x2['lp_sum'])
    assert torch.equal(nt_t, nt_0) and torch.equal(nt_t, x['n_tok'])
    assert x['tokens'] == int(r['n_tok'].sum()) and np.array_equal(nt_t.cpu().numpy(), r['n_tok'])
    assert x['perplexity'] == pytest.approx(np.exp(x['loss']), rel=1e-12)
    assert abs(-x['loss'] - r['fit']) <= 1e-5
    assert np.abs(lp_t.cpu().numpy() - r['lp_sum']).max() <= 17 * LP_BAR
    _, steps = e.test_xent_steps(theta_batch=0)
    assert np.abs(steps.cpu().numpy().astype(np.float64) - r['lp'])[r['mask']].max() <= LP_BAR
    # a sub-range of the split: the rows of images 1.. only
    if len(gts) > 1:
        y = sp.xent(first=1)
        n0 = gts[0].shape[0]
        assert torch.equal(y['lp_sum'], x['lp_sum'][n0:]) and torch.equal(y['n_tok'], x['n_tok'][n0:])
    sp.close()


def test_split_xent_leaves_the_handle_as_it_was(engines):
    """fitness mode, df table and batches after Split.xent: a greedy evaluate before and after gives the same bits, and
    so does an xent one"""
    w, e = _world('b'), engines('b')
    fc, gts = w['batches'][1]
    try:
        e.set_fitness_mode('greedy')
        g0, s0 = e.evaluate(IT, 0, P, SIGMA, member_batch=w['mb'], return_seq=True)
        sp = e.make_split(fc, gts)
        sp.xent()
        g1, s1 = e.evaluate(IT, 0, P, SIGMA, member_batch=w['mb'], return_seq=True)
        assert torch.equal(g0, g1) and torch.equal(s0, s1) and e.fitness_mode == 0
        e.set_fitness_mode('xent')
        x0 = e.evaluate(IT, 0, P, SIGMA, member_batch=w['mb'])
        sp.xent()
        x1 = e.evaluate(IT, 0, P, SIGMA, member_batch=w['mb'])
        assert torch.equal(x0, x1)
        sp.close()
    finally:
        e.set_fitness_mode('xent')


def test_a_greedy_decodes_tokens_as_labels_reproduce_its_log_probs(engines):
    """evaluate_lp's log-probs of member 0, sign +, are the forced log-probs of its own tokens, step by step"""
    w = _world('b')
    fc = w['batches'][0][0]
    e = _engine('b')
    try:
        e.set_theta(w['theta'])
        _df(e, w['batches'])
        e.set_batch(*w['batches'][0])
        _, seq, lp = e.evaluate(IT, 0, 1, SIGMA, return_seq=True, return_lp=True)
        seq, lp = seq.cpu().numpy()[0, 0], lp.cpu().numpy()[0, 0]
        assert (seq > 0).any()
        e.set_batch(fc, [r[None] for r in seq])
        e.set_fitness_mode('xent')
        _, steps = e.test_xent_steps(IT, 0, 1, SIGMA)
        steps = steps.cpu().numpy()[0, 0]
        mask = X.counted(seq)[:, :seq.shape[1]]
        assert np.abs(steps[:, :seq.shape[1]].astype(np.float64) - lp)[mask].max() <= LP_BAR
    finally:
        e.close()


class _XentOracleEngine(OracleEngine):
    """the oracle engine with the restatement's xent fitness"""

    def set_fitness_mode(self, fitness):
        assert fitness == 'xent'
        self.fitness_mode = 8

    def evaluate(self, iteration, member_begin, count, sigma, fitness_out=None, member_batch=None):
        out = fitness_out if fitness_out is not None else torch.empty((count, 2), dtype=torch.float64)
        for k in range(count):
            idx = self._idx(iteration, member_begin + k)
            fc, gts = (self.fc, self.gts) if member_batch is None else self.batches[member_batch[k]]
            for s, sign in enumerate((+1, -1)):
                out[k, s] = X.fitness(self.dims, O.perturb(self.theta32, self.table, idx, sigma, sign), fc, gts)
        return out


def test_master_two_iterations_with_a_validator_against_the_host_trajectory(tmp_path):
    import nicnes
    import nicnes.synthetic as S
    from nicnes import config as C, master as M
    from nicnes.validation import Validator
    from tests.test_gpu_wide import _Loader
    dims = O.Dims(vocab_size=67, F=128)
    theta = O.make_theta(dims, 0, 4.0, 0.1)
    fc = np.random.Generator(np.random.PCG64(1234)).standard_normal((19, dims.F)).astype(np.float32)
    base, _, _ = O.decode(dims, theta, fc)
    gts, df, n = S.build_references(base, dims.vocab_size, seed=9, n_refs=5, df_sets=128)
    table = O.noise_table(1 << 21, 123)
    Pm = 4

    def spec():
        return C.ExperimentSpec({
            'algorithm': 'nic_nes', 'nb_offspring': Pm,
            'config': {'noise_stdev': 0.01, 'batch_size': 8, 'l2coeff': 1e-3, 'snapshot_freq': 0, 'single_batch': True,
                       'num_val_items': 3},
            'policy_options': {'net': 'fc_caption', 'fitness': 'xent', 'model_options': {'fc_feat_size': 128}},
            'optimizer_options': {'type': 'adam', 'args': {'stepsize': 1e-2}}}, vocab_size=67)
    e = nicnes.Engine(**spec().engine_kwargs(max_members=Pm, noise_len=1 << 21, noise_seed=0, max_batch=8))
    try:
        e.set_noise_table(table)
        keys, vals = nicnes.df_table_arrays(df)
        e.set_df_table(keys, vals, np.log(float(n)))
        la, lb = _Loader(fc, gts, 3, 67), _Loader(fc, gts, 3, 67)
        gpu = M.EngineMaster(spec(), e, log_dir=str(tmp_path / 'gpu'), theta=theta,
                             validator=Validator(e, la, 'val', 3, xent=True))
        ora_e = _XentOracleEngine(dims, theta, fc, gts, df, n, table, noise_seed=0)
        ora = M.EngineMaster(spec(), ora_e, log_dir=str(tmp_path / 'cpu'), theta=theta)
        val_fc, val_gts = fc[-3:], gts[-3:]
        want_val = []
        gpu.run(la, max_iterations=2)
        for _ in range(2):                       # the host's val_loss of the theta each iteration evaluates
            want_val.append(-X.fitness(dims, ora_e.theta32, val_fc, val_gts))
            ora.run(lb, max_iterations=ora.sched.iteration + 1)
        assert len(gpu.stats) == len(ora.stats) == 2
        for a, b, v in zip(gpu.stats, ora.stats, want_val):
            for k in ('score_mean', 'score_max', 'score_min'):
                assert abs(a[k] - b[k]) <= 1e-5, (k, a[k], b[k])
            assert abs(a['val_loss'] - v) <= 1e-5 and np.isfinite(a['val_score'])
        t64 = e.theta()[0].cpu().numpy()
        assert np.allclose(t64, ora_e.adam.theta, rtol=1e-6, atol=1e-12)
        m, v, t = e.adam_state()
        assert t == 2 and np.allclose(m.cpu().numpy(), ora_e.adam.m, rtol=1e-6, atol=1e-15)
        assert np.allclose(v.cpu().numpy(), ora_e.adam.v, rtol=1e-6, atol=1e-20)
    finally:
        e.close()


def test_the_mode_is_chosen_by_name(engines):
    """Engine.set_fitness_mode takes integer codes of the reference's Fitness enum only; the extension goes by name"""
    e = engines('e')
    try:
        with pytest.raises(ValueError, match='xent'):
            e.set_fitness_mode(8)
        assert e.fitness_mode == 8                   # unchanged by the refused call
        e.set_fitness_mode(0)
        assert e.fitness_mode == 0
    finally:
        e.set_fitness_mode('xent')
    assert e.fitness_mode == e.XENT_MODE == 8


def _refused(fn, word):
    from nicnes._lib import NicnesError
    with pytest.raises(NicnesError, match='not supported') as ei:
        fn()
    assert word in str(ei.value), str(ei.value)


def test_refusals_leave_the_handle_usable(engines):
    import nicnes
    w, e = _world('b'), engines('b')
    before = e.evaluate(IT, 0, P, SIGMA, member_batch=w['mb'])
    # a mutation together with xent
    e.set_mutation('divide', np.ones(e.D, np.float32))
    try:
        _refused(lambda: e.evaluate(IT, 0, P, SIGMA, member_batch=w['mb']), 'mutations')
        _refused(lambda: e.evaluate_theta(0), 'mutations')
    finally:
        e.set_mutation('plain')
    # nic_es in xent mode
    e.es_create(2, 1)
    try:
        e.es_set_parent(0, w['theta'])
        e.es_set_parent_count(1)
        _refused(lambda: e.es_evaluate(0, 0, 1, SIGMA, [0], member_batch=[0]), 'nic_es')
    finally:
        e.es_free()
    # a split without references
    sp = e.make_split(w['batches'][0][0])
    _refused(lambda: sp.xent(), 'decode-only')
    assert sp.decode().shape[0] == sp.N
    sp.close()
    after = e.evaluate(IT, 0, P, SIGMA, member_batch=w['mb'])
    assert torch.equal(before, after)
    # wide and layer_n handles
    for kw in (dict(rnn_size=256), dict(layer_n=True)):
        h = nicnes.Engine(vocab_size=67, fc_feat_size=128, max_batch=8, max_members=2, noise_len=NOISE_LEN, noise_seed=SEED,
                          **kw)
        try:
            _refused(lambda: h.set_fitness_mode('xent'), 'xent')
            assert h.fitness_mode == 0
            fc, gts = w['batches'][0][0][:4], w['batches'][0][1][:4]
            sd = O.Dims(vocab_size=67, F=128, R=kw.get('rnn_size', 128))
            h.set_noise_table(_table())
            h.set_theta(O.make_theta(sd, 0, 4.0, 0.1))
            sp = h.make_split(fc, gts)
            _refused(lambda: sp.xent(), 'xent')
            assert sp.decode().shape == (4, 16)
            sp.close()
        finally:
            h.close()
