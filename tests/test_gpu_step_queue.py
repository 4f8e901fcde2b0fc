"""GPU: the screened decode from the step queue (nicnes_decode_steps_screen_queue_kernel) against the same handle with
the queue off (nicnes_decode_steps_screen_kernel): every token, the fitness bits, the screen_* counters and
tie_fallbacks. Screening is forced on; the worker count is forced small so that a member's steps migrate between
workers (two workers: each re-reads scratch lines the other has just rewritten, the case that shows a load served from a
stale L1 line; one worker: every hand-off goes through one warm L1).

Worlds (small, as tests/test_gpu_dims.py's): vocabulary 255 (V1 256, 4 logit stages), T 4, B 32 and 136 (two slabs), and
vocabulary 999 (V1 1000, 16 stages, the last 40 columns wide), T 16, B 128; F 128. theta is the trained-like one of
tests/test_gpu_dims.py (gain 4, bias std 0.1) with the end token's logit bias raised by END_BIAS, so that rows end at
different steps; members decode per-member batches, one of which repeats a single image, so every row of such a member
ends at the same step and its `alive` goes to 0 before T (asserted on the queue-off run's tokens).

After every case: queue_timeouts has not moved, queue_steps has moved by the tasks the queue-off tokens imply (a member
slab runs t = -1, 0, then one task per token position until every row of the slab has ended or T is reached), the ring
is empty and the finished count equals the member slabs."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

NOISE_LEN = 1 << 22
SEED = 7
SIGMA = 0.01
IT = 3
END_BIAS = 2.0
MAX_MEMBERS = 13
WORLDS = {
    'v255': dict(vocab=255, T=4, B=32),
    'v255_two_slabs': dict(vocab=255, T=4, B=136),
    'v999': dict(vocab=999, T=16, B=128),
}
N_BATCHES = 3                      # batch 1 repeats one image

_cache = {}


def _table():
    import nicnes.synthetic as S
    if 'table' not in _cache:
        _cache['table'] = S.noise_table(NOISE_LEN, 123)
    return _cache['table']


def _make(world, env=None, edit=None):
    """An engine of the world, loaded: theta (edit(theta, offsets) may change it), three batches and references made from
    the engine's own decode of theta (the comparison is queue on against queue off, so the references only have to give
    a non-trivial fitness). env: test hooks read at create."""
    import nicnes
    import nicnes.synthetic as S
    w = WORLDS[world]
    mp = pytest.MonkeyPatch()
    mp.setenv('NICNES_BOUNDED_LSE', '1')       # greedy-only decodes always run the PAIRS instantiations (screening)
    for k, v in (env or {}).items():
        mp.setenv(k, v)
    try:
        e = nicnes.Engine(vocab_size=w['vocab'], fc_feat_size=128, seq_length=w['T'], max_batch=w['B'],
                          max_members=MAX_MEMBERS, noise_len=NOISE_LEN, noise_seed=SEED)
    finally:
        mp.undo()
    try:
        theta = S.init_theta(S.Dims(w['vocab'], 128, 128, 128, w['T']), 0, 4.0, 0.1)
        assert theta.size == e.D
        theta[e.offsets[4]] += np.float32(END_BIAS)          # logit.bias[0]: the end token
        if edit:
            edit(theta, e.offsets)
        e.set_noise_table(_table())
        e.set_theta(theta)
        rng = np.random.Generator(np.random.PCG64(100 + w['B']))
        fcs = [rng.standard_normal((w['B'], 128)).astype(np.float32) for _ in range(N_BATCHES)]
        fcs[1] = np.repeat(fcs[1][:1], w['B'], axis=0)
        zero = [np.zeros((1, w['T']), np.int32)] * w['B']
        e.set_df_table(np.zeros(0, np.uint64), np.zeros(0), np.log(64.0))
        base_all = []
        for fc in fcs:                              # theta's own captions of each batch -> its references
            e.set_batch(fc, zero)
            base_all.append(e.evaluate_theta(0, return_seq=True)[1].cpu().numpy())
        _, df, n = S.build_references(np.concatenate(base_all), w['vocab'], seed=11, df_sets=64, T=w['T'])
        gts_all = [S.build_references(base, w['vocab'], seed=20 + i, df_sets=0, T=w['T'])[0]
                   for i, base in enumerate(base_all)]
        keys, vals = nicnes.df_table_arrays(df)
        e.set_df_table(keys, vals, np.log(float(n)))
        e.set_batches(list(zip(fcs, gts_all)))
        e.set_decode_split(1, 4)                    # the fused path (128-row slabs, one workgroup per member slab),
        e.set_decode_screen(True)                   # screened, whatever the member count
    except BaseException:
        e.close()
        raise
    return e


@pytest.fixture(scope='module')
def engines():
    """One engine per world, made at its first use and kept for the module."""
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    made = {}

    def get(world):
        if world not in made:
            made[world] = _make(world)
        return made[world]
    yield get
    for e in made.values():
        e.close()


def _tasks(seq, T):
    """Tasks of a launch from the queue-off tokens seq [members, 2, B, T]: per member slab (128 rows of both signs)
    2 + the steps until every row has emitted its end token, at most T."""
    total, early = 0, 0
    P, _, B, _ = seq.shape
    for k in range(P):
        for r0 in range(0, B, 128):
            rows = seq[k, :, r0:r0 + 128].reshape(-1, T)
            ended = (rows == 0).any(1)
            last = int(np.where(ended, (rows == 0).argmax(1), T).max()) + 1     # steps until the last row has ended
            n = min(T, last)
            early += n < T
            total += 2 + n
    return total, early


_COUNTERS = ['tie_fallbacks', 'screen_candidates', 'screen_fallback_rows', 'screen_rows_over_cap', 'screen_rows_undecided',
             'screen_rows_evicted', 'screen_rows_nonfinite', 'screen_rows_settled_later', 'screen_resweep_rows',
             'screen_resweep_steps', 'screen_resweep_waves']


def _run(e, members, mb, sigma):
    before = e.stats()
    fit, seq = e.evaluate(IT, 0, members, sigma, return_seq=True, member_batch=mb)
    fit, seq = fit.cpu().numpy(), seq.cpu().numpy()
    after = e.stats()
    return fit, seq, {k: after[k] - before[k] for k in _COUNTERS + ['queue_steps', 'queue_timeouts']}, after


def _check(e, world, members, workers, mode=True, expect_queue=True, need_early=False, sigma=SIGMA):
    w = WORLDS[world]
    mb = [k % N_BATCHES for k in range(members)]
    slabs = (w['B'] + 127) // 128
    e.set_decode_queue(False)
    fit0, seq0, d0, _ = _run(e, members, mb, sigma)
    # (the screened kernel ran: it counts candidates, or, under force_exact, which lists none, the rows it left bad)
    assert d0['queue_steps'] == 0 and d0['screen_candidates'] + d0['screen_fallback_rows'] > 0, d0
    assert fit0.max() > 0.0
    if sigma:
        assert len(np.unique(seq0)) >= 20
    tasks, early = _tasks(seq0, w['T'])
    if need_early:
        assert early >= 1, 'no member slab ends before T: raise END_BIAS'
        assert early < members * slabs, 'every member slab ends before T: lower END_BIAS'
    e.set_decode_queue(mode, workers)
    try:
        runs = [_run(e, members, mb, sigma) for _ in range(2)]       # twice: the queue words are set again each launch
    finally:
        e.set_decode_queue('auto', 0)
    for fit1, seq1, d1, after in runs:
        assert np.array_equal(seq1, seq0)
        assert np.array_equal(fit1.view(np.uint64), fit0.view(np.uint64))
        assert {k: d1[k] for k in _COUNTERS} == {k: d0[k] for k in _COUNTERS}
        assert d1['queue_timeouts'] == 0 and after['coop_timeouts'] == 0
        if expect_queue:
            assert d1['queue_steps'] == tasks, (d1['queue_steps'], tasks)
            assert after['queue_pending'] == 0 and after['queue_finished'] == members * slabs, after
        else:
            assert d1['queue_steps'] == 0
    return d0


@pytest.mark.parametrize('world,members,workers', [('v255', 13, 5), ('v999', 7, 2), ('v255', 3, 2), ('v999', 6, 1),
                                                   ('v255_two_slabs', 5, 3), ('v255', 1, 1)],
                         ids=['13_over_5', '7_over_2', '3_over_2', '6_over_1', '5x2_slabs_over_3', '1_over_1'])
def test_steps_migrate_between_workers(engines, world, members, workers):
    """More member slabs than workers (and one on one): tokens, fitness and counters are those of the one-launch kernel.
    The per-member batches end rows at different steps, and the members on the repeated image leave before T."""
    _check(engines(world), world, members, workers, need_early=world == 'v999')


@pytest.mark.parametrize('members,workers', [(4, 4), (3, 8)], ids=['equal', 'below'])
def test_at_or_below_the_worker_count(engines, members, workers):
    """Members equal to the workers, and fewer: auto keeps the one-launch kernel; forced on, the queue is still correct."""
    e = engines('v255')
    _check(e, 'v255', members, workers, mode='auto', expect_queue=False)
    _check(e, 'v255', members, workers, mode=True, expect_queue=True)


def test_auto_takes_the_queue_above_the_worker_count(engines):
    _check(engines('v255'), 'v255', 5, 4, mode='auto', expect_queue=True)


def _tie_nine(theta, off):
    """Nine ids, one per logit stage 1..9 and all of lane half 0, share one logit row; biases 30 - j 2^-12 (the 'tied K'
    input of tests/test_gpu_screen_rounds.py): at sigma = 0 every one is a candidate of its row's lane, nine hit weights
    against a list of eight, so every step takes a second certify round; id 64 wins."""
    W = theta[off[3]:off[3] + 1000 * 128].reshape(1000, 128)
    b = theta[off[4]:off[4] + 1000]
    for j, v in enumerate([64 * s for s in range(1, 10)]):
        W[v] = W[64]
        b[v] = np.float32(30.0) - np.float32(j * 2.0 ** -12)


@pytest.mark.parametrize('env,edit,sigma,key', [(None, _tie_nine, 0.0, 'screen_rows_settled_later'),
                                                 ({'NICNES_FORCE_EXACT': '1'}, None, SIGMA, 'screen_resweep_steps')],
                         ids=['certify_rounds', 'fp32_fallback'])
def test_certify_rounds_and_fp32_fallback_migrate(env, edit, sigma, key):
    """A decode whose every step takes a second certify round, and one whose every step takes the gated fp32 fallback
    (force_exact), each with four members over two workers."""
    e = _make('v999', env, edit)
    try:
        d0 = _check(e, 'v999', 4, 2, sigma=sigma)
        assert d0[key] > 0, (key, d0)
    finally:
        e.close()
