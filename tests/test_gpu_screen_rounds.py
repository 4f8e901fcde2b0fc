"""The screened decode's certify rounds and its wave-gated fp32 fallback, on the GPU.

A lane whose hits weigh more than one hit list holds (SCREEN_HIT_CAP = 8, a crowded lane-stage counts 4) used to send
its workgroup's step to the fp32 loop. It now certifies its hits in further rounds of 8 hit weights, up to the round
budget R (NICNES_SCREEN_ROUNDS, default 2; 1 is the behaviour before); a step the rounds cannot settle runs the fp32
loop on the waves that hold a bad row only.

Inputs (P = 2, sigma = 0, theta = make_theta(dims, 0, 4.0, 0.1), both signs and members decode the same tokens).
Lane (row, half 0) owns ids 64 s + 32 c + 8 g + e (c < 2, g < 4, e < 4) of stage s, in pairs (e = 0, 1), (e = 2, 3).
Every id planted here lies in lane half 0, tile c = 0, group g = 0, pair 0 or 1, and tied ids share one logit row, so the
screen keeps their order; lane half 1, tile 1, pairs 2 .. 15 and ids the screen misorders are the worlds of
tests/screen_worlds.py (tests/test_gpu_screen_misorder.py).
  tied K          K ids 64 (2 j + 1), j < K, one per stage, share one logit row; b = 30 - j 2^-12. The span is below
                  2 eps (eps >= 2^-13 30) and far above the tie window (2^-24 at lse < 2), and chains of identical
                  products started a multiple of ulp(30) apart stay that far apart: every tied id is a candidate of
                  the lane and id 64 wins outright. K hit weights: K = 8 fits the list, 9 and 12 take a second round.
  crowded         three stages s with 64 s and 64 s + 2 tied (two pairs of one lane-stage: crowded): 12 hit weights.
  over the budget 8 R + 1 hit weights, the least the budget refuses: 8 R + 1 tied ids, one per stage from stage 1 on
                  (were R raised until a vocabulary has fewer stages than that, 2 R crowded stages and one single id
                  make the same weight). The biases fall by 2^-14 per id, so that the span (at most 32 2^-14 = 2^-9)
                  stays below 2 eps for R <= 4.
  evicted         an input no number of rounds settles: an evicted record inside the tie window. Records change only
                  on a strictly greater logit, so three equal logits never evict one; the logits have to rise with
                  the id within the window, and a window of several ulps needs logits below 1 under an lse above 8.
                  W = 0 makes every logit its bias for every row: b = 0.499 everywhere (lse = 8.5 .. 9.2, window
                  2^-21) but three ids of one lane-stage at 0.5 + (1, 2, 3) 2^-24. They are the only candidates
                  (eps ~ 2^-13 0.5 << 0.001), the third evicts the first, all within 2^-23: the fp32 loop and then
                  the exact pass decide, and the token is the lowest of the three.
  partial         the random theta and decode whose counters test_gpu_certify pins (3 bad rows in the whole decode,
                  each among good rows of the other waves and the other sign): with R = 1 the fp32 loop runs for
                  them, and screen_resweep_waves shows that only their waves ran it.

Every case runs on two engines, default rounds and NICNES_SCREEN_ROUNDS=1: each must decode what the unscreened
decode does (_on_off), both must count the same screen_candidates."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from oracle import oracle as O                                                  # noqa: E402
from tests.test_gpu_screen import _evaluator, _logit_views, _on_off             # noqa: E402

R_DEFAULT = 2                               # decode_kernel.h SCREEN_ROUNDS_DEFAULT
P = 2


def _base(vocab):
    dims = O.Dims(vocab_size=vocab)
    theta = O.make_theta(dims, 0, 4.0, 0.1).copy()
    W, b = _logit_views(dims, theta)
    return dims, theta, W, b


def _tie(W, b, ids, step):
    for j, v in enumerate(ids):
        W[v] = W[ids[0]]
        b[v] = np.float32(30.0) - np.float32(j * step)


def _tied_theta(vocab, K):
    dims, theta, W, b = _base(vocab)
    ids = [64 * (2 * j + 1) for j in range(K)]
    assert ids[-1] <= vocab
    _tie(W, b, ids, 2.0 ** -12)
    return theta, ids[0]


def _crowded_theta(vocab):
    dims, theta, W, b = _base(vocab)
    ids = [v for s in (1, 2, 3) for v in (64 * s, 64 * s + 2)]
    _tie(W, b, ids, 2.0 ** -12)
    return theta, ids[0]


def _over_budget_theta(vocab, R):
    dims, theta, W, b = _base(vocab)
    nst = (vocab + 1 + 63) // 64
    if nst - 1 >= 8 * R + 1:
        ids = [64 * s for s in range(1, 8 * R + 2)]                      # 8 R + 1 single hits
    else:
        ids = [v for s in range(1, 2 * R + 1) for v in (64 * s, 64 * s + 2)] + [64 * (2 * R + 1)]   # 2 R crowded + 1
    assert ids[-1] <= vocab and len(ids) <= 33
    _tie(W, b, ids, 2.0 ** -14)
    return theta, ids[0]


def _evicted_theta(vocab):
    dims, theta, W, b = _base(vocab)
    W[:] = 0.0
    b[:] = 0.499
    ids = [64 * 5, 64 * 5 + 1, 64 * 5 + 2]                               # one lane-stage: a pair and the next pair
    for j, v in enumerate(ids):
        b[v] = np.float32(0.5) + np.float32((j + 1) * 2.0 ** -24)
    assert b[ids[0]] < b[ids[1]] < b[ids[2]]
    return theta, ids[0]


def _both(monkeypatch, vocab, B, theta, sigma=0.0, env=None, members=P):
    """(seq, counters) of the screened decode under the default rounds and under NICNES_SCREEN_ROUNDS=1"""
    out = []
    for rounds in (None, '1'):
        ev = dict(env or {})
        if rounds:
            ev['NICNES_SCREEN_ROUNDS'] = rounds
        else:
            monkeypatch.delenv('NICNES_SCREEN_ROUNDS', raising=False)
        e = _evaluator(monkeypatch, vocab, B, members, theta, env=ev)
        try:
            seq, d = _on_off(e, members, sigma=sigma)
        finally:
            e.close()
        print('V %d B %d rounds %s: %s' % (vocab, B, rounds or 'default', {k: v for k, v in d.items() if v}))
        out.append((seq, d))
    assert np.array_equal(out[0][0], out[1][0])
    assert out[0][1]['screen_candidates'] == out[1][1]['screen_candidates'] > 0
    return out


def _settled_by_rounds(out, tok):
    (seq, d), (_, d1) = out
    assert d['screen_fallback_rows'] > 0                                 # the first round left them
    assert d['screen_rows_over_cap'] == d['screen_fallback_rows']
    assert d['screen_resweep_rows'] == 0 and d['screen_resweep_steps'] == 0
    assert d['screen_rows_settled_later'] == d['screen_fallback_rows']
    assert (seq == tok).all()
    # one round: the same rows go to the fp32 loop, so the input does take the lanes over the cap
    assert d1['screen_fallback_rows'] == d['screen_fallback_rows']
    assert d1['screen_resweep_rows'] == d1['screen_fallback_rows'] > 0
    assert d1['screen_resweep_steps'] > 0 and d1['screen_rows_settled_later'] == 0


@pytest.mark.parametrize('vocab', [9487, 1999])
@pytest.mark.parametrize('K', [8, 9, 12])
def test_tied_ids_over_the_cap_are_settled_by_later_rounds(monkeypatch, vocab, K):
    theta, tok = _tied_theta(vocab, K)
    out = _both(monkeypatch, vocab, 40, theta)
    if K == 8:                                                           # fits the list: no round but the first
        for seq, d in out:
            assert d['screen_fallback_rows'] == 0 and d['screen_resweep_steps'] == 0
            assert (seq == tok).all()
    else:
        _settled_by_rounds(out, tok)
        assert out[0][1]['screen_over_cap_rounds_2'] == out[0][1]['screen_fallback_rows']


@pytest.mark.parametrize('vocab', [9487, 1999])
def test_crowded_lane_stages_over_the_cap_are_settled_by_later_rounds(monkeypatch, vocab):
    theta, tok = _crowded_theta(vocab)
    _settled_by_rounds(_both(monkeypatch, vocab, 40, theta), tok)


@pytest.mark.parametrize('vocab', [9487, 1999])
def test_a_lane_over_the_round_budget_goes_to_the_fp32_loop(monkeypatch, vocab):
    theta, tok = _over_budget_theta(vocab, R_DEFAULT)
    for seq, d in _both(monkeypatch, vocab, 40, theta):
        assert d['screen_resweep_rows'] == d['screen_fallback_rows'] > 0
        assert d['screen_resweep_steps'] > 0 and d['screen_rows_settled_later'] == 0
        assert d['screen_over_cap_rounds_%d' % (R_DEFAULT + 1)] == d['screen_fallback_rows']
        assert (seq == tok).all()


@pytest.mark.parametrize('B', [8, 40, 128])
def test_an_evicted_record_in_the_window_runs_the_gated_fp32_loop(monkeypatch, B):
    theta, tok = _evicted_theta(9487)
    for seq, d in _both(monkeypatch, 9487, B, theta):
        assert d['screen_resweep_steps'] > 0
        assert d['screen_rows_evicted'] == d['screen_fallback_rows'] == d['screen_resweep_rows'] > 0
        assert d['screen_rows_over_cap'] == 0 and d['screen_rows_settled_later'] == 0
        # every row is bad, the padding rows (copies of the decode's first rows) with them: no wave sits out
        assert d['screen_resweep_waves'] == 8 * d['screen_resweep_steps']
        assert (seq == tok).all()                                        # the lowest of the three


def test_flat_logits_are_over_any_budget(monkeypatch):
    dims, theta, W, b = _base(9487)
    W[:] = W[17]
    b[:] = 0.25
    for seq, d in _both(monkeypatch, 9487, 40, theta):
        assert d['screen_resweep_rows'] == d['screen_fallback_rows'] > 0 and d['screen_resweep_steps'] > 0
        assert d['screen_over_cap_rounds_9'] == d['screen_rows_over_cap'] > 0
        assert (seq == 0).all()                                          # the first id of the window: the end token


def test_the_fp32_loop_runs_with_waves_sitting_out(monkeypatch):
    # test_gpu_certify's pinned decode (P = 3, B = 40, gain 4, bias std 0.1, sigma 0.01): 3 rows go bad in all of it,
    # among good rows of their own wave, of the other waves and of the other sign
    theta = O.make_theta(O.Dims(), 0, 4.0, 0.1)
    out = _both(monkeypatch, 9487, 40, theta, sigma=0.01, members=3)
    d, d1 = out[0][1], out[1][1]
    assert d1['screen_fallback_rows'] == d['screen_fallback_rows'] == 3
    # one round: each is re-swept. A bad row puts its own wave into the loop and no other, so over the decode at most 3
    # waves ran it, at least one per re-swept step; each workgroup has 4 waves with real rows (2 per sign at B = 40) and
    # 4 of padding, so fewer than 4 waves in a step means that a wave with real, needed rows sat the loop out and kept
    # the tokens of its records (which _on_off found equal to the unscreened decode's)
    steps, waves = d1['screen_resweep_steps'], d1['screen_resweep_waves']
    assert d1['screen_resweep_rows'] == 3 and 1 <= steps <= waves <= 3
    # the three rows fall into three different workgroup steps: each ran one wave of one sign, the other sign's tile
    # was not even staged
    assert waves < 2 * steps
    assert d['screen_rows_settled_later'] + d['screen_resweep_rows'] == 3
    assert (d['screen_resweep_steps'] > 0) == (d['screen_resweep_rows'] > 0)
    assert d['screen_resweep_steps'] <= d['screen_resweep_waves'] <= d['screen_resweep_rows']
