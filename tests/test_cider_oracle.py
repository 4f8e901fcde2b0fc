"""Known-answer tests of the restated CIDEr-D (oracle/cider_ref.py). The reference scorer lives in
the unvendored `cider` submodule, so these pin the restatement by hand-derived values
(parity with the reference implementation itself: unpinned)."""
import math
import os

import numpy as np
import pytest

from oracle import cider_ref as CR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def test_array_to_str_includes_first_zero():
    # /root/reference/src/algorithm/tools/utils.py:34-40
    assert CR.array_to_str(np.array([5, 7, 0, 3, 0])) == '5 7 0'
    assert CR.array_to_str(np.array([0, 4])) == '0'
    assert CR.array_to_str(np.array([1, 2, 3])) == '1 2 3'


def test_identical_single_ref_scores_ten():
    s = CR.CiderDOracle({}, 10)            # empty df: every idf = log(10) > 0
    assert s.score_one('1 2 3 4 5', ['1 2 3 4 5']) == pytest.approx(10.0, rel=1e-12)


def test_disjoint_scores_zero():
    s = CR.CiderDOracle({}, 10)
    assert s.score_one('1 2 3', ['4 5 6']) == 0.0


def test_df_equal_ref_len_zeroes_the_ngram():
    # an n-gram seen in every reference set has idf = log(N) - log(N) = 0
    df = {('7',): 10.0}
    s = CR.CiderDOracle(df, 10)
    vec, norm, length = s.counts2vec(CR.precook('7 8'))
    assert vec[0][('7',)] == 0.0 and vec[0][('8',)] == pytest.approx(math.log(10))
    assert length == 1                      # one bigram: the 'length' is the bigram count


def test_length_penalty_uses_bigram_counts():
    s = CR.CiderDOracle({}, 100)
    hyp, ref = '1 2', '1 2 9 9 9 9 9'
    # unigrams/bigrams of hyp all in ref; delta = (1 - 6) bigrams
    sc = s.score_one(hyp, [ref])
    vh, nh, lh = s.counts2vec(CR.precook(hyp))
    vr, nr, lr = s.counts2vec(CR.precook(ref))
    assert (lh, lr) == (1, 6)
    pen = np.e ** (-(5.0 ** 2) / (2 * 36.0))
    val1 = sum(min(vh[0][g], vr[0][g]) * vr[0][g] for g in vh[0]) / (nh[0] * nr[0]) * pen
    val2 = sum(min(vh[1][g], vr[1][g]) * vr[1][g] for g in vh[1]) / (nh[1] * nr[1]) * pen
    assert sc == pytest.approx((val1 + val2) / 4 * 10, rel=1e-12)


def test_clipping_min_term():
    s = CR.CiderDOracle({}, 100)
    # hyp repeats a word more often than the ref: min(vh, vr) clips
    vh, nh, _ = s.counts2vec(CR.precook('3 3 3'))
    vr, nr, _ = s.counts2vec(CR.precook('3'))
    assert vh[0][('3',)] == pytest.approx(3 * math.log(100))
    sc = s.sim(vh, vr, nh, nr, 2, 0)
    assert sc[0] == pytest.approx(min(vh[0][('3',)], vr[0][('3',)]) * vr[0][('3',)] / (nh[0] * nr[0])
                                  * np.e ** (-4 / 72.0))


def test_rollout_fitness_dedup_equals_duplicated():
    """mean over 5x-duplicated rows == mean over unique rows (fixed df): the engine decodes
    unique images only."""
    rng = np.random.default_rng(3)
    B = 6
    seq = rng.integers(0, 20, (B, 16))
    gts = [rng.integers(1, 20, (5, 16)) for _ in range(B)]
    df, n = CR.document_frequency_from_refs([[CR.array_to_str(r) for r in g] for g in gts])
    s = CR.CiderDOracle(df, n)
    f_unique, _ = CR.rollout_fitness(s, seq, gts, 1)
    f_dup, _ = CR.rollout_fitness(s, np.repeat(seq, 5, axis=0), gts, 5)
    assert f_unique == pytest.approx(f_dup, rel=1e-12)


@pytest.mark.parametrize('mode', ['greedy_logprob', 'greedy_expprob', 'greedy_linprob', 'greedy_avgprob', 'sc_loss'])
def test_criterion_oracle_matches_reference_golden(mode):
    """greedy_* criteria (src/captioning/fitness.py:43-132) against the reference's own classes
    (tests/golden/fitness_criteria.npz, scripts/make_golden.py); the reference sums in fp32."""
    z = np.load(os.path.join(GOLDEN, 'fitness_criteria.npz'))
    for c in range(3):
        got = CR.criterion_fitness(mode, z['lp_%d' % c], z['seq_%d' % c], z['scores_%d' % c])
        ref = float(z['%s_%d' % (mode, c)])
        assert abs(got - ref) <= 1e-6 * max(1.0, abs(ref)), (c, got, ref)


def test_criterion_duplicate_rows_invariant():
    """The engine scores unique images once; the reference decodes each 5x (dataloader.py:175).
    The criterion is a ratio of sums, so 5 identical copies give the same value."""
    rng = np.random.Generator(np.random.PCG64(5))
    seq = rng.integers(0, 9, (6, 16))
    lp = -rng.exponential(1.0, (6, 16)).astype(np.float32)
    sc = rng.uniform(0, 2, 6)
    for mode in ('greedy_logprob', 'greedy_expprob', 'greedy_linprob', 'greedy_avgprob'):
        a = CR.criterion_fitness(mode, lp, seq, sc)
        b = CR.criterion_fitness(mode, np.repeat(lp, 5, 0), np.repeat(seq, 5, 0), np.repeat(sc, 5))
        assert abs(a - b) <= 1e-12 * max(1.0, abs(a))


# ---- semantics the given-rows scorer tests (tests/test_gpu_cider.py) lean on, derived by hand ----
def test_df_below_one_counts_as_one():
    """counts2vec takes log(max(1, df)): df = 0.5, df = 1 and an absent n-gram all weigh tf * log(N).
    N = 10, '7 8' against itself: unigrams and the one bigram match exactly (val = 1 each), there are
    no 3- or 4-grams (val = 0, norms 0), equal lengths (penalty 1): (1 + 1 + 0 + 0) / 4 / 1 * 10 = 5."""
    for df in ({('7',): 0.5}, {('7',): 1.0}, {}):
        s = CR.CiderDOracle(df, 10)
        vec, norm, _ = s.counts2vec(CR.precook('7 8'))
        assert vec[0][('7',)] == math.log(10) == vec[0][('8',)]
        assert norm[0] == pytest.approx(math.sqrt(2) * math.log(10), rel=1e-15)
        assert s.score_one('7 8', ['7 8']) == pytest.approx(5.0, rel=1e-12)


def test_df_equal_ref_len_gives_zero_norm_and_undivided_val():
    """df = N: weight tf * (log N - log N) = 0 exactly. With every unigram of the hypothesis at df = N its
    unigram norm is 0, so sim leaves val[0] undivided; val[0] is then 0 anyway (every min(0, vr) * vr has
    vr = tf_r * 0 = 0, the same n-gram having the same df on both sides), never 0 / 0.
    N = 10, df('7') = df('8') = 10, '7 8' against itself: val[0] = 0 (undivided), the bigram ('7', '8') is
    absent from df: weight log 10 on both sides, val[1] = 1; no 3- / 4-grams; penalty 1:
    (0 + 1 + 0 + 0) / 4 * 10 = 2.5."""
    s = CR.CiderDOracle({('7',): 10.0, ('8',): 10.0}, 10)
    vec, norm, _ = s.counts2vec(CR.precook('7 8'))
    assert vec[0][('7',)] == 0.0 and vec[0][('8',)] == 0.0 and norm[0] == 0.0
    assert s.score_one('7 8', ['7 8']) == pytest.approx(2.5, rel=1e-12)
    # hypothesis norm 0, reference norm not: '7' against '7 9' -> val[0] = min(0, 0) * 0 = 0, score 0
    assert s.score_one('7', ['7 9']) == 0.0


def test_df_above_ref_len_gives_negative_weights_through_min():
    """df = 4 N: weight tf * (log N - log 4N) = -tf * log 4 < 0, and min() picks the MORE negative side.
    N = 10, df('7') = 40, hypothesis '7' against '7 7': vh = -log 4, vr = -2 log 4, min = vr,
    val[0] = vr * vr = 4 log^2 4, / (|vh| |vr| = 2 log^2 4) = 2 (a 'cosine' of 2). The reference's bigram
    ('7', '7') has no partner (the hypothesis has no bigram: val[1] = 0). Lengths in bigrams 0 and 1:
    penalty e^(-1 / 72). Score = 2 e^(-1/72) / 4 * 10 = 5 e^(-1/72)."""
    s = CR.CiderDOracle({('7',): 40.0}, 10)
    vh, nh, lh = s.counts2vec(CR.precook('7'))
    vr, nr, lr = s.counts2vec(CR.precook('7 7'))
    assert vh[0][('7',)] == pytest.approx(-math.log(4), rel=1e-15)
    assert vr[0][('7',)] == pytest.approx(-2 * math.log(4), rel=1e-15)
    assert (lh, lr) == (0, 1)
    assert s.sim(vh, vr, nh, nr, lh, lr)[0] == pytest.approx(2.0 * math.exp(-1 / 72.0), rel=1e-12)
    assert s.score_one('7', ['7 7']) == pytest.approx(5.0 * math.exp(-1 / 72.0), rel=1e-12)


def test_caption_of_only_the_zero_token():
    """A row starting with 0 is the string '0': one unigram, no bigram, so its 'length' (bigram count) is 0.
    Against the reference '0': val[0] = 1, orders 2-4 empty, penalty 1: 1 / 4 * 10 = 2.5.
    Against '3 0' (N = 10, empty df): vh('0') = log 10; vr = {3: log 10, 0: log 10}, |vr| = sqrt(2) log 10;
    val[0] = log^2 10 / (log 10 * sqrt(2) log 10) = 1 / sqrt(2); lengths 0 and 1: penalty e^(-1/72).
    Score = e^(-1/72) / sqrt(2) / 4 * 10."""
    hyp = CR.array_to_str(np.array([0, 5, 6, 0]))
    assert hyp == '0'
    s = CR.CiderDOracle({}, 10)
    vec, norm, length = s.counts2vec(CR.precook(hyp))
    assert dict(vec[0]) == {('0',): math.log(10)} and not vec[1] and length == 0
    assert s.score_one(hyp, ['0']) == pytest.approx(2.5, rel=1e-12)
    assert s.score_one(hyp, ['3 0']) == pytest.approx(math.exp(-1 / 72.0) / math.sqrt(2) / 4 * 10, rel=1e-12)


def test_tf_clipping_sixteen_against_two():
    """One token 16 times against '4 4' (N = 100, empty df, w = log 100):
    unigram: vh = 16 w, vr = 2 w, min = 2 w: val = 4 w^2 / (16 w * 2 w) = 1 / 8;
    bigram ('4', '4'): tf 15 against 1: val = w^2 / (15 w * w) = 1 / 15;
    3- / 4-grams: the reference has none (norm 0): min(vh, 0) * 0 = 0, undivided;
    lengths 15 and 1 bigrams: penalty e^(-14^2 / 72). Score = (1/8 + 1/15) * e^(-196/72) / 4 * 10."""
    s = CR.CiderDOracle({}, 100)
    hyp = CR.array_to_str(np.full(16, 4))
    assert hyp == ' '.join(['4'] * 16)
    vh, nh, lh = s.counts2vec(CR.precook(hyp))
    assert vh[0][('4',)] == pytest.approx(16 * math.log(100), rel=1e-15) and lh == 15
    want = (1 / 8 + 1 / 15) * math.exp(-196 / 72.0) / 4 * 10
    assert s.score_one(hyp, ['4 4']) == pytest.approx(want, rel=1e-12)
