"""GPU: the sampled pick (sample_pick, csrc/decode_kernel.hip) with draws that are aimed instead of random.

The pick scans stored per-lane fp64 block and stage sums, each relative to the lane's own integer reference r, then
walks one stage's 64 logits spread over the two lanes of a row, and has three "the sums stop short" fallbacks. Uniform
draws leave what it picks to chance; here every draw is planted by the CPU oracle (oracle.decode_sample_planted, the
worlds of tests/sample_worlds.py) at the midpoint of a chosen id's cdf interval, at least 1e-5 from both ends (ten
times U_MARGIN: no summation order moves a boundary that far), so the engine's token has to be the target at every
position:

(a) planted picks: every in-stage slot of the stages either side of the block boundaries (7|8, 15|16, 63|64), of the
    level-1 round boundary (blocks 19|20, stages 159|160; V1 16384) and of the 4-, 8-, 16-, 40- and 60-column tail
    stages; the 'stairs' worlds raise r in mid-block, at a block start and at the last stage, and in one lane half;
(b) rows that end: a target of 0 ends its row; the oracle then feeds 0 back and goes on drawing (it = tok * unfinished,
    the draw's log-prob is still recorded), and once every row of a (member, sign) has ended the remaining log-probs
    are the global early exit's zeros;
(c) edge draws u = 0.0 and u = nextafter(1, 0);
(d) the fallback branches, run deterministically with u = 2.0: thr = 2 T is never crossed;
(e) the engine's own draw stream against oracle.sample_draws fed through the hook, bit for bit.

Every case runs on both instantiations of the pick: the stage scan and the full walk (NICNES_FORCE_EXACT=1)."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from oracle import oracle as O          # noqa: E402
from tests import sample_worlds as W    # noqa: E402
from tests.test_gpu_sample import _write_coverage   # noqa: E402

LP_TOL = 1e-5                           # the suite's log-prob bar (tests/test_gpu_parity.py)
PICKS = ['scan', 'walk']
EDGE_WORLDS = ['flat', 'stairs', 'stairs1000', 'v68', 'v60', 'v255']
ONE_MINUS = np.nextafter(1.0, 0.0)

_REPORT = {}


def _write_report(name, key, value):
    """Into the run's output directory, next to tests/test_gpu_sample.py's coverage file and by its writer."""
    _REPORT.setdefault(name, {})[key] = value
    _write_coverage(name + '.json', _REPORT[name])


def _make(vocab, T, B, members, exact):
    import nicnes
    mp = pytest.MonkeyPatch()
    if exact:
        mp.setenv('NICNES_FORCE_EXACT', '1')
    else:
        mp.delenv('NICNES_FORCE_EXACT', raising=False)
    try:
        e = nicnes.Engine(vocab_size=vocab, fc_feat_size=W.F, seq_length=T, max_batch=B, max_members=members,
                          noise_len=W.NOISE_LEN, noise_seed=W.NOISE_SEED)
    finally:
        mp.undo()
    try:
        e.set_noise_table(W.table())
        e.set_df_table(np.zeros(0, np.uint64), np.zeros(0), np.log(64.0))     # fitness is not the subject here
    except BaseException:
        e.close()
        raise
    return e


@pytest.fixture(scope='module')
def engines():
    """One engine per (shape, pick), made at its first use and kept for the module; worlds of one shape share it."""
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    made = {}

    def get(world, pick, B=None):
        w = W.WORLDS[world]
        B = B or w['B']
        key = (w['vocab'], w['T'], B, w['members'], pick)
        if key not in made:
            made[key] = _make(*key[:4], exact=pick == 'walk')
        e = made[key]
        assert e.D == W.dims(world).D
        e.set_theta(W.theta(world))
        return e
    yield get
    for e in made.values():
        e.close()


def _load(e, fc, T):
    e.set_batch(fc, [np.zeros((1, T), np.int32)] * fc.shape[0])


def _launch(e, world, u, count=None):
    """One sampled evaluate of the world's members with the draws u: (seq, lp, the counters' movement)."""
    w = W.WORLDS[world]
    count = count or w['members']
    _load(e, W.fc(world), w['T'])
    idx, _ = W.member_thetas(world)
    assert e.noise_indices(W.IT, 0, count).cpu().numpy().tolist() == idx[:count]
    e.set_fitness_mode('sample')
    try:
        e.set_sample_draws(u)
        before = e.stats()
        _, seq, lp = e.evaluate(W.IT, 0, count, W.SIGMA, return_seq=True, return_lp=True)
        seq, lp = seq.cpu().numpy(), lp.cpu().numpy()
        after = e.stats()
    finally:
        e.set_fitness_mode('greedy')
        e.set_sample_draws(None)
    return seq, lp, {k: after[k] - before[k] for k in ('sample_stage_fallbacks', 'sample_slot_timeouts')}


def _lp_close(lp, want):
    err = np.abs(lp.astype(np.float64) - want.astype(np.float64))
    assert err.max() <= LP_TOL, (err.max(), np.argwhere(err > LP_TOL)[:5])
    return float(err.max())


def _mismatch(seq, want):
    bad = np.argwhere(seq != want)
    return '%d of %d differ; first (member, sign, row, step) got / want: %s' % (
        len(bad), want.size, [(tuple(i), int(seq[tuple(i)]), int(want[tuple(i)])) for i in bad[:8]])


# ---- (a) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pick', PICKS)
@pytest.mark.parametrize('world', W.PLANTED_WORLDS)
def test_planted_picks(engines, world, pick):
    """Every candidate id of the world is drawn at least once, by a draw at the middle of its interval: tokens are the
    targets at 100 % of the positions, log-probs the oracle's to 1e-5, and neither the stage fallback nor the slot
    timeout counter moves."""
    tg = W.targets(world)
    u, hw, oseq, olp = W.planted(world)
    assert hw.min() >= W.MIN_HALF_WIDTH and np.array_equal(oseq, tg)
    seq, lp, moved = _launch(engines(world, pick), world, u)
    print('%s/%s: %d positions, %d ids, min half-width %.3g, counters %s' % (world, pick, tg.size, len(np.unique(tg)),
                                                                            hw.min(), moved))
    assert np.array_equal(seq, tg), _mismatch(seq, tg)
    err = _lp_close(lp, olp)
    assert moved == {'sample_stage_fallbacks': 0, 'sample_slot_timeouts': 0}, moved
    _write_report('sample_pick_planted', '%s/%s' % (world, pick),
                  {'positions_compared': int(tg.size), 'positions': int(seq.size), 'distinct_ids': int(len(np.unique(tg))),
                   'candidates': int(len(W.candidates(world))), 'min_half_width': float(hw.min()),
                   'max_logprob_error': err})


# ---- (b) ---------------------------------------------------------------------------------------------------------
def _ending_targets(world):
    """The world's targets with ends planted: scattered rows draw 0 at a step before T (the first step, a middle one,
    the one before last), and every row of the last (member, sign) draws 0 at step 4."""
    w = W.WORLDS[world]
    tg = W.targets(world).copy()
    T, B = w['T'], w['B']
    for i, b in enumerate(range(1, B, 7)):
        tg[0, 0, b, (0, T // 2, T - 2)[i % 3]] = 0
    tg[0, 0, B - 1, 2] = 0                               # (in the second slab where B > 128)
    tg[-1, 1, :, 3] = 0
    return tg


@pytest.mark.parametrize('pick', PICKS)
@pytest.mark.parametrize('world', ['flat', 'stairs1000'])
def test_rows_that_end(engines, world, pick):
    """Rows that draw the end token. The oracle (decode_core) keeps drawing for a finished row: it feeds it = tok *
    unfinished = 0 back, picks with the row's next draw and records that pick's log-prob while the token written is 0;
    after the step at which the last row of a (member, sign) ended its log-probs stay 0 (the reference's global early
    exit). The engine must give the same: tokens 0 after the end, log-probs the oracle's, zeros included."""
    def make():
        tg = _ending_targets(world)
        return (tg,) + W.plant(world, tg)
    tg, u, hw, oseq, olp = W._once(('ending', world), make)
    assert hw.min() >= W.MIN_HALF_WIDTH
    ended = np.cumsum(tg == 0, axis=-1) > 0
    assert np.array_equal(oseq, np.where(ended, 0, tg))
    assert ended[-1, 1].all(axis=0)[3:].all() and (olp[-1, 1, :, 4:] == 0).all() and (olp[-1, 1, :, :4] != 0).all()
    assert (olp[0, 0] != 0).all()                        # scattered ends: no global exit, every draw's log-prob is kept
    seq, lp, moved = _launch(engines(world, pick), world, u)
    assert np.array_equal(seq, oseq), _mismatch(seq, oseq)
    _lp_close(lp, olp)
    assert np.array_equal(lp == 0, olp == 0)
    assert moved == {'sample_stage_fallbacks': 0, 'sample_slot_timeouts': 0}, moved


# ---- (c) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pick', PICKS)
@pytest.mark.parametrize('world', EDGE_WORLDS)
def test_edge_draws(engines, world, pick):
    """Even rows draw u = 0.0 at every step, odd rows u = nextafter(1, 0), in one launch. u = 0.0 takes id 0 at step 1
    and the row stays ended; u = 1 - 2^-53 takes V1 - 1 at every step (V1 - 1 lies in lane half 1 of chain a in the
    16-column tail, in half 1 of chain b in the 40- and 64-column ones, in half 0 of chain a in the 4-column one and in
    half 0 of chain b in the 60-column one). The oracle flags every one of these draws fragile, being within 1e-6 of a cdf boundary (0 and 1) by
    construction; the answer is unambiguous all the same: every prefix sum that leaves the last id out is at least
    p(V1 - 1) (about 1e-4 in the flat worlds) short of the total, far more than any rounding of u * T, and p(0) > 0
    exceeds a threshold of exactly 0. The fallback count of this launch is recorded, not asserted: whether the sums
    reach (1 - 2^-53) T is a matter of rounding."""
    w = W.WORLDS[world]
    V1 = w['vocab'] + 1
    u = np.empty((w['members'], 2, w['B'], w['T']))
    u[:, :, 0::2] = 0.0
    u[:, :, 1::2] = ONE_MINUS
    oseq, olp, ofr = W._once(('edge', world), lambda: W.decode_with(world, u))
    want = np.zeros_like(oseq)
    want[:, :, 1::2] = V1 - 1
    assert np.array_equal(oseq, want) and ofr.all()
    p_last = np.exp(olp[:, :, 1::2].astype(np.float64)).min()
    assert p_last > 1e-5 and np.exp(olp[:, :, 0::2, 0].astype(np.float64)).min() > 1e-6
    seq, lp, moved = _launch(engines(world, pick), world, u)
    print('%s/%s: edge-draw launch moved %s, min p(V1 - 1) %.3g' % (world, pick, moved, p_last))
    _write_report('sample_pick_fallbacks', 'edge/%s/%s' % (world, pick),
                  dict(moved, rows_at_one_minus=int(u[:, :, 1::2, 0].size), steps=w['T']))
    assert np.array_equal(seq, want), _mismatch(seq, want)
    _lp_close(lp, olp)
    assert moved['sample_slot_timeouts'] == 0


# ---- (d) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pick', PICKS)
@pytest.mark.parametrize('world', EDGE_WORLDS)
def test_fallbacks_with_a_draw_past_one(engines, world, pick):
    """u = 2.0 on every row and step (the hook takes any fp64; no draw of the engine's own stream reaches 1): thr = 2 T
    is never crossed, so the block scan, the stage scan and the stage walk each take their "stops short" branch (the
    full walk: its no-crossing tail). By the code every pick is min(64 sf + 63, V1 - 1) with sf the last stage, that
    is V1 - 1, inside the vocabulary, its log-prob read from the registers of the lane half that holds that column;
    the oracle's default is V1 - 1 as well. The counter moves by exactly members x 2 x B x T: one per valid row and
    step, added by lane half 0, and no row ever ends."""
    w = W.WORLDS[world]
    V1 = w['vocab'] + 1
    u = np.full((w['members'], 2, w['B'], w['T']), 2.0)
    oseq, olp, _ = W._once(('past_one', world), lambda: W.decode_with(world, u))
    assert (oseq == V1 - 1).all()
    seq, lp, moved = _launch(engines(world, pick), world, u)
    print('%s/%s: u = 2.0 launch moved %s of %d picks' % (world, pick, moved, u.size))
    _write_report('sample_pick_fallbacks', 'past_one/%s/%s' % (world, pick), dict(moved, picks=int(u.size)))
    assert (seq == V1 - 1).all(), _mismatch(seq, oseq)
    _lp_close(lp, olp)
    assert moved == {'sample_stage_fallbacks': u.size, 'sample_slot_timeouts': 0}, (moved, u.size)


# ---- (e) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pick', PICKS)
@pytest.mark.parametrize('B', [40, 130])
def test_engine_stream_is_the_oracles(engines, B, pick):
    """The engine's own draws (nicnes_sample_draws_kernel: values, the [count, 2, rows, T] layout, the member offset):
    an evaluate without the hook returns tokens and log-probs equal bit for bit to the same call with
    oracle.sample_draws fed through the hook. Members from 0, one member from 2, five rows per image (rows = 5 B), and
    evaluate_theta, whose stream is member 0xffffffff's over the half batch each sign decodes."""
    world, T = 'flat', W.WORLDS['flat']['T']
    e = engines(world, pick, B=B)
    fc = np.random.Generator(np.random.PCG64(100 + B)).standard_normal((B, W.F)).astype(np.float32)
    _load(e, fc, T)

    def both(run, draws):
        e.set_sample_draws(None)
        own = [x.cpu().numpy() for x in run()[1:]]
        e.set_sample_draws(draws)
        fed = [x.cpu().numpy() for x in run()[1:]]
        e.set_sample_draws(None)
        assert np.array_equal(own[0], fed[0]), _mismatch(own[0], fed[0])
        assert np.array_equal(own[1].view(np.int32), fed[1].view(np.int32))
        assert len(np.unique(own[0])) > 100               # flat logits: the draws spread over the vocabulary
        return own[0]

    e.set_fitness_mode('sample')
    try:
        it = 5
        a = both(lambda: e.evaluate(it, 0, 2, W.SIGMA, return_seq=True, return_lp=True),
                 O.sample_draws(W.NOISE_SEED, it, 0, 2, B, T))
        assert a.shape == (2, 2, B, T)
        c = both(lambda: e.evaluate(it, 2, 1, W.SIGMA, return_seq=True, return_lp=True),
                 O.sample_draws(W.NOISE_SEED, it, 2, 1, B, T))
        assert not np.array_equal(c[0], a[0])
        e.set_rows_per_image(5)
        r = both(lambda: e.evaluate(it + 1, 0, 2, W.SIGMA, return_seq=True, return_lp=True),
                 O.sample_draws(W.NOISE_SEED, it + 1, 0, 2, 5 * B, T))
        assert r.shape == (2, 2, 5 * B, T)
        e.set_rows_per_image(1)
        t = both(lambda: e.evaluate_theta(0, return_seq=True, return_lp=True, iteration=it),
                 O.sample_draws(W.NOISE_SEED, it, 0xffffffff, 1, (B + 1) // 2, T))
        assert t.shape == (B, T)
    finally:
        e.set_sample_draws(None)
        e.set_rows_per_image(1)
        e.set_fitness_mode('greedy')
