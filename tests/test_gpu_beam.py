"""GPU: the beam-search decode of a resident split (nicnes_split_decode_beam / _evaluate_beam, Split.decode_beam,
Split.evaluate(beam_size=)) against the host restatement of its definition, tests/beam_ref.py.

Selection: the kernel's own top-K and selection code on planted log-prob rows (nicnes_test_beam_select) must give the
restatement's selector's (b, v) list exactly, ties included. Tokens and scores: on every image the restatement does
not mark fragile (tests/beam_ref.py; tests/test_beam_ref.py checks on the CPU that at most FRAGILE_CAP of every case's
images are, and that the workloads are not vacuous) the tokens are equal and the fp64 scores agree within 16 x 1e-5,
the project's per-step log-prob bar over at most 16 steps. K = 1 is Split.decode on the rows the oracle does not mark
fragile, and its score the sum of Split.decode's log-probs. Runs repeat bit for bit, a range decoded in halves equals the whole, evaluate(beam_size=K) is
score(decode_beam(K)) bit for bit and beam_size=None is today's evaluate, the training batches and fitness mode are
untouched, and K outside 1..8 is refused."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from oracle import oracle as O          # noqa: E402
from tests import beam_ref as BR        # noqa: E402

NOISE_LEN = 1 << 23


def _engine(dims, max_batch=16):
    import nicnes
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return nicnes.Engine(max_batch=max_batch, max_members=2, noise_len=max(NOISE_LEN, dims.D), noise_seed=7,
                         vocab_size=dims.vocab_size, fc_feat_size=dims.F, seq_length=dims.T)


@pytest.fixture(scope='module')
def small():
    """an engine for the entries that need no particular model"""
    dims = O.Dims(vocab_size=127, F=128, T=16)
    e = _engine(dims)
    yield e
    e.close()


# ------------------------------------------------------------------ selection on planted rows -----------------------
def _select_ref(lp, score, live, K):
    out = np.full((lp.shape[0], K, 2), -1, np.int32)
    for i in range(lp.shape[0]):
        for k, (_, b, v) in enumerate(BR.select(lp[i], score[i], live[i], K)[:K]):
            out[i, k] = (b, v)
    return out


def _planted(case, K, V1, n_img, rng):
    """log-prob rows [n_img, K, V1] (any floats: the selector only orders them), scores, live flags"""
    lp = -rng.uniform(1.0, 9.0, (n_img, K, V1)).astype(np.float32)
    score = -rng.uniform(0.0, 4.0, (n_img, K))
    live = np.ones((n_img, K), np.int32)
    if case == 'ties_across_beams':         # equal scores and the same best rows: (b ascending, v ascending) decides
        lp[:] = lp[:, :1]
        score[:] = -1.25
    elif case == 'ties_across_ids':         # a handful of values only: every row is full of exact ties
        lp = -rng.integers(1, 4, (n_img, K, V1)).astype(np.float32)
        score[:] = np.round(score)
    elif case == 'dead_rows':
        live = (rng.uniform(size=(n_img, K)) < 0.5).astype(np.int32)
        live[0] = 0                          # an image with no candidate at all
        live[1] = 0
        live[1, K - 1] = 1                   # only the last row alive
    elif case == 'best_in_last_stage':      # V1 = 68: ids 64..67 are the last 32-id stage's four columns
        lp[:, :, 64:] = -rng.uniform(0.0, 0.5, (n_img, K, V1 - 64)).astype(np.float32)
    elif case == 'both_lane_halves':        # ids 0-3 / 8-11 are one lane half, 4-7 / 12-15 the other
        for j in range(K):
            lp[:, :, (4 * j) % V1] = np.float32(-0.01 * (j + 1))
    elif case == 'all_in_one_row':
        score[:, K // 2] = 50.0
    return lp, score, live


SELECT_CASES = [('ties_across_beams', 3, 128), ('ties_across_beams', 8, 8), ('ties_across_ids', 5, 128),
                ('ties_across_ids', 8, 8), ('ties_across_ids', 2, 68), ('dead_rows', 3, 128), ('dead_rows', 8, 8),
                ('plain', 8, 8), ('plain', 1, 128), ('best_in_last_stage', 3, 68), ('best_in_last_stage', 8, 68),
                ('both_lane_halves', 5, 128), ('both_lane_halves', 8, 68), ('all_in_one_row', 3, 128),
                ('all_in_one_row', 8, 8), ('plain', 7, 300)]


@pytest.mark.parametrize('case,K,V1', SELECT_CASES)
def test_selection_on_planted_rows(small, case, K, V1):
    rng = np.random.Generator(np.random.PCG64(1000 + SELECT_CASES.index((case, K, V1))))
    n_img = 2 * (32 // K) + 3               # more than one wave, the last one partly filled
    lp, score, live = _planted(case, K, V1, n_img, rng)
    got = small.test_beam_select(lp, score, live).cpu().numpy()
    want = _select_ref(lp, score, live, K)
    assert np.array_equal(got, want), (case, K, V1, np.argwhere((got != want).any((1, 2)))[:4].tolist())


# ------------------------------------------------------------------ tokens and scores --------------------------------
@pytest.fixture(scope='module', params=list(BR.WORKLOADS))
def world(request):
    dims, theta, fc, cases, ref = BR.workload(request.param)
    e = _engine(dims)
    e.set_theta(theta)
    split = e.make_split(fc)
    yield request.param, e, split, dims, theta, fc, cases, ref
    split.close()
    e.close()


def test_tokens_and_scores_against_the_restatement(world):
    name, e, split, dims, theta, fc, cases, ref = world
    for K, first, count in cases:
        seq, score = split.decode_beam(first, count, K, return_score=True)
        seq, score = seq.cpu().numpy(), score.cpu().numpy()
        assert seq.shape == (count, dims.T) and seq.dtype == np.int32 and score.shape == (count,)
        checked = 0
        for j in range(count):
            r = ref[(K, first + j)]
            if r['fragile']:
                continue
            checked += 1
            print('%s K%d image %d score %.9f want %.9f' % (name, K, first + j, score[j], r['score']))
            assert np.array_equal(seq[j], r['tokens']), (name, K, first + j, seq[j].tolist(), r['tokens'].tolist())
            assert abs(score[j] - r['score']) <= BR.SCORE_TOL, (name, K, first + j, score[j], r['score'])
        assert checked >= (1.0 - BR.FRAGILE_CAP) * count, (name, K, checked, count)


def test_beam_1_is_the_greedy_decode(world):
    name, e, split, dims, theta, fc, cases, ref = world
    oseq, _, fragile = O.decode(dims, theta, fc)
    keep = ~np.asarray(fragile).reshape(fc.shape[0], -1).any(1)
    assert keep.sum() >= 0.9 * fc.shape[0]
    greedy = split.decode().cpu().numpy()
    beam1, score = split.decode_beam(0, None, 1, return_score=True)
    beam1, score = beam1.cpu().numpy(), score.cpu().numpy()
    assert np.array_equal(beam1[keep], greedy[keep]), (name, np.argwhere((beam1 != greedy).any(1)).ravel()[:8].tolist())
    # the score is the fp64 sum of the log-probs Split.decode reports (0 after a row's end token). Logits and row maximum
    # are the same bits on both sides; the exp-sums add the same terms in another order (32-id tiles here, the greedy
    # decode's stages there), so a step's log-prob may differ by the project's 1e-5 log-prob bar at the most
    _, lp = split.decode(return_lp=True)
    lp = lp.cpu().numpy().astype(np.float64)
    steps = np.minimum((np.cumsum(greedy == 0, 1) == 0).sum(1) + 1, dims.T)
    diff = np.abs(score - lp.sum(1))
    print('%s beam-1 score against the greedy log-probs: max |diff| %.3g' % (name, diff[keep].max()))
    assert (diff[keep] <= steps[keep] * 1e-5).all(), (name, diff[keep].max())


def test_repeats_bit_for_bit_and_halves_equal_the_whole(world):
    name, e, split, dims, theta, fc, cases, ref = world
    N = fc.shape[0]
    for K in (2, 3, 8):
        a, sa = split.decode_beam(0, N, K, return_score=True)
        b, sb = split.decode_beam(0, N, K, return_score=True)
        assert torch.equal(a, b) and torch.equal(sa.view(torch.int64), sb.view(torch.int64)), (name, K)
        cut = N // 2 + 1
        lo, slo = split.decode_beam(0, cut, K, return_score=True)
        hi, shi = split.decode_beam(cut, N - cut, K, return_score=True)
        assert torch.equal(torch.cat([lo, hi]), a), (name, K)
        assert torch.equal(torch.cat([slo, shi]).view(torch.int64), sa.view(torch.int64)), (name, K)


def test_both_workgroup_shapes_give_the_same_bits(world):
    """the launch picks 4 or 8 waves per workgroup from the range's size (4 at these sizes); set_beam_waves forces
    either: the last workgroup partly filled, and waves with no image at all"""
    name, e, split, dims, theta, fc, cases, ref = world
    try:
        for K, first, count in cases[:3]:
            want, wscore = split.decode_beam(first, count, K, return_score=True)
            for nw in (4, 8):
                e.set_beam_waves(nw)
                got, gscore = split.decode_beam(first, count, K, return_score=True)
                e.set_beam_waves(0)
                assert torch.equal(got, want), (name, K, nw)
                assert torch.equal(gscore.view(torch.int64), wscore.view(torch.int64)), (name, K, nw)
        with pytest.raises(Exception):
            e.set_beam_waves(2)
    finally:
        e.set_beam_waves(0)


# ------------------------------------------------------------------ metrics, other state, arguments -----------------
@pytest.fixture(scope='module')
def scored():
    """the v128 workload's model with references, a training batch and a fitness mode set"""
    import nicnes
    import nicnes.synthetic as S
    dims, theta, fc, _ = BR.workload_inputs('v128')
    fc = fc[:40]
    e = _engine(dims, max_batch=40)
    e.set_noise_table(O.noise_table(max(NOISE_LEN, dims.D), 123))
    e.set_theta(theta)
    base, _, _ = O.decode(dims, theta, fc)
    gts, df, n = S.build_references(base, dims.vocab_size, seed=3, df_sets=64)
    keys, vals = nicnes.df_table_arrays(df)
    e.set_df_table(keys, vals, np.log(float(n)))
    e.set_batch(fc[:16], gts[:16])
    split = e.make_split(fc, gts)
    yield e, split
    split.close()
    e.close()


def _bits(res):
    m, totals, rows = res
    return (np.asarray([m[k] for k in sorted(m)], np.float64).view(np.int64).tolist(), totals.tolist(),
            rows.view(np.int64).tolist())


def test_evaluate_with_a_beam_is_score_of_decode_beam(scored):
    e, split = scored
    for K in (1, 3, 5):
        seq = split.decode_beam(0, None, K)
        res, seq2 = split.evaluate(detail=True, return_seq=True, beam_size=K)
        assert torch.equal(seq, seq2)
        assert _bits(res) == _bits(split.score(seq, detail=True)), K


def test_beam_size_none_is_todays_evaluate(scored):
    e, split = scored
    res, seq = split.evaluate(detail=True, return_seq=True)
    res2, seq2 = split.evaluate(detail=True, return_seq=True, beam_size=None)
    assert torch.equal(seq, seq2) and torch.equal(seq, split.decode())
    assert _bits(res) == _bits(res2) == _bits(split.score(seq, detail=True))


def test_a_beam_decode_leaves_other_state_untouched(scored):
    e, split = scored
    fit0, seq0 = e.evaluate(1, 0, 2, 0.01, return_seq=True)
    ev0 = _bits(split.evaluate(detail=True))
    split.decode_beam(0, None, 5)
    split.evaluate(beam_size=3)
    fit1, seq1 = e.evaluate(1, 0, 2, 0.01, return_seq=True)
    assert torch.equal(seq0, seq1) and torch.equal(fit0.view(torch.int64), fit1.view(torch.int64))
    assert _bits(split.evaluate(detail=True)) == ev0
    assert e.stats()['coop_timeouts'] == 0


def test_beam_width_outside_1_to_8_is_refused(scored):
    import ctypes
    e, split = scored
    for K in (0, 9, -1):
        with pytest.raises(ValueError):
            split.decode_beam(0, 4, K)
        with pytest.raises(ValueError):
            split.evaluate(beam_size=K)
    seq = torch.zeros((4, e.cfg.seq_length), dtype=torch.int32, device=e.device)
    for K in (0, 9):                         # the C entry itself: NICNES_ERR_INVALID
        rc = e.L.nicnes_split_decode_beam(e.h, split.sp, 0, 4, K, ctypes.c_void_p(seq.data_ptr()), None, None)
        assert rc == 1, (K, rc)
