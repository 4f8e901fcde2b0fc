"""The preconditions of tests/screen_worlds.py, on the CPU: what makes each planted world a case in which the bf16
screen ranks the exact greedy winner below another id, checked against the header's bound (nn_screen_eps through the
helper of tests/test_screen_bound.py), an emulated bf16 MFMA under three accumulation models (screened()) and the
oracle. A world that misses a bar gets another seed or position, never another bar.

On every target row at the planted step (the target rows share one image, so one h):
  bf16(W_a) == bf16(W_b) element for element; greedy_pick(z) == a, not fragile; z[a] - z[b] >= 64 spacing(z[a]);
  the argmax of each of the three screened rows is the leader b; the screened lead l~_b - l~_a is at least the
  accumulation term 2^-15.9 (babs + hnorm wnorm) of the comment above nn_screen_eps; the depth m~ - l~_a is at most eps
  (half the window: a sound kernel must keep a) and at least 0.02 (shallow) / 0.10 (aligned) of the window 2 eps; the
  case's positions (pair, half, tile, stage, last valid id); the oracle's decode of the whole batch starts the target
  rows with a, with at most 5 % of (row, step) fragile.

The positional ties (tie_case): bit-equal rows and biases, bit-equal logits, the pick is the lower id, each copy alone
in its lane-stage.

Achieved (printed per case by test_planted_world_meets_its_preconditions; acc = the accumulation term; a case's figures
depend on its vocabulary and variant, not on where its ids lie, except as listed):

  V     variant  case             G        eps      exact a - b          screened b - a        depth / (2 eps)
  999   shallow  (all others)     1.08e-2  8.88e-2  5.38e-3 (11290 ulps)  5.38e-3 ( 21.8 acc)   0.030
  999   shallow  triple_reversed  1.08e-2  8.88e-2  2.69e-3 ( 5648 ulps)  5.38e-3 ( 21.8 acc)   0.030
  999   shallow  negative_logits  1.08e-2  9.32e-2  5.41e-3 ( 1419 ulps)  5.39e-3 (  6.4 acc)   0.029
  999   shallow  sigma_member     1.17e-2  8.60e-2  5.83e-3 (12216 ulps)  5.83e-3 ( 24.3 acc)   0.034
  9487  shallow  (all others)     4.95e-3  3.25e-2  2.47e-3 ( 5189 ulps)  2.48e-3 ( 18.6 acc)   0.038
  9487  shallow  triple_reversed  4.95e-3  3.25e-2  1.24e-3 ( 2590 ulps)  2.48e-3 ( 18.6 acc)   0.038
  9487  shallow  sigma_member     4.81e-3  3.21e-2  2.40e-3 ( 5043 ulps)  2.41e-3 ( 18.2 acc)   0.037
  9487  aligned  (all others)     1.63e-2  3.38e-2  4.08e-3 ( 8559 ulps)  1.22e-2 (135.8 acc)   0.181
  9487  aligned  triple_reversed  1.63e-2  3.38e-2  2.04e-3 ( 4284 ulps)  1.22e-2 (135.8 acc)   0.181
  9487  aligned  sigma_member     1.61e-2  3.34e-2  4.02e-3 ( 8438 ulps)  1.21e-2 (137.6 acc)   0.181

(triple_reversed: "exact a - b" is the smaller of a's two exact leads, over a + 8; the screened lead and the depth are
those of a + 16 over a. negative_logits: L_a = -33.5, so an ulp is 8 times as large and babs = 40 raises acc.)
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import ln_ref as L
from tests import screen_worlds as SW
from tests.test_screen_bound import bf16, eps_of, helper, screened      # noqa: F401  (helper: the fixture)

U32 = np.uint32


def _norms(hl, W, b, h):
    """(hnorm, wnorm, babs) as eps_of forms them"""
    ss_h = np.float32(0)
    for x in h.astype(np.float32):
        ss_h = np.float32(ss_h + np.float32(x * x))
    ss_w = (W.astype(np.float32) ** 2).astype(np.float32).sum(axis=1, dtype=np.float32).max()
    return float(hl.screen_norm(ss_h)), float(hl.screen_norm(ss_w)), float(np.abs(b).max())


def _positions(case, ids, V1):
    a, b = ids[0], ids[-1]
    same_lane_stage = SW.lane_stage(a) == SW.lane_stage(b)
    if case in ('same_pair_lo', 'same_pair_hi'):
        assert b == a ^ 1 and same_lane_stage and SW.pair(a) == SW.pair(b) == 13 and SW.lane_half(a) == 1
        assert (a < b) == (case == 'same_pair_lo')
    elif case == 'other_pair_same_group':
        assert b == a ^ 2 and same_lane_stage and SW.group(a) == SW.group(b) and SW.pair(a) != SW.pair(b)
    elif case == 'other_group_same_tile':
        assert b == a + 8 and same_lane_stage and SW.tile(a) == SW.tile(b) and SW.group(a) != SW.group(b)
    elif case == 'other_tile':
        assert b == a ^ 32 and same_lane_stage and SW.tile(a) != SW.tile(b) and SW.pair(a) == SW.pair(b) ^ 8
    elif case in ('pair_15_wins', 'pair_15_leads'):
        hi, lo = (a, b) if case == 'pair_15_wins' else (b, a)
        assert same_lane_stage and SW.pair(hi) == 15 and SW.pair(lo) == 0 and hi == 64 * SW.stage(hi) + 32 + 24 + 2
    elif case == 'other_half':
        assert b == a ^ 4 and SW.stage(a) == SW.stage(b) and SW.lane_half(a) != SW.lane_half(b)
        assert SW.pair(a) == SW.pair(b) >= 2
    elif case in ('next_stage', 'negative_logits'):
        assert b == a + 64 and SW.lane_half(a) == SW.lane_half(b) and SW.pair(a) == SW.pair(b) >= 2
    elif case == 'far_stage':
        assert b == a + 64 * 17 and SW.stage(b) // 16 > SW.stage(a) // 16      # another 16-word block of the scan
    elif case in ('last_id_wins', 'last_id_leads'):
        last, first = (a, b) if case == 'last_id_wins' else (b, a)
        assert last == V1 - 1 and V1 % 32 != 0 and SW.stage(first) == 0 and first > 0
        assert SW.stage(last) == (V1 + 63) // 64 - 1
    elif case == 'end_token_wins':
        assert a == 0 and b > 0 and SW.lane_stage(a) != SW.lane_stage(b)
    elif case == 'triple_reversed':
        assert ids[1] == a + 8 and ids[2] == a + 16 and len({SW.lane_stage(v) for v in ids}) == 1
        assert len({SW.pair(v) for v in ids}) == 3
    elif case == 'sigma_member':
        assert SW.stage(b) == SW.stage(a) - 3 and SW.pair(a) == SW.pair(b) == 14
    else:
        raise KeyError(case)
    return same_lane_stage


def check_plant(hl, case, vocab, variant):
    """asserts the preconditions of one planted world; -> its figures"""
    p = SW.planted(case, vocab, variant)
    W, b, h, ids = p['W'], p['b'], p['h'], p['ids']
    a, lead = p['a'], p['lead']
    V1 = p['dims'].V1
    what = (case, vocab, variant)
    for v in ids[1:]:
        assert np.array_equal(bf16(W[a]).view(U32), bf16(W[v]).view(U32)), what
        assert not np.array_equal(W[a], W[v])
    z = O.gemv(W, b, h)
    tok, _, fragile = L.greedy_pick(z)
    assert tok == a and fragile == 0, what + (tok, fragile)
    sp = float(np.spacing(np.abs(z[a])))
    exact = min(float(z[a]) - float(z[v]) for v in ids[1:])
    assert exact >= 64 * sp, what + (exact / sp,)
    assert all(z[ids[i]] > z[ids[i + 1]] for i in range(len(ids) - 1)), what
    lt = screened(hl, W, b, h)
    for l in lt:
        assert int(np.argmax(l)) == lead, what + (int(np.argmax(l)),)
        assert all(l[ids[i]] < l[ids[i + 1]] for i in range(len(ids) - 1)), what       # the reverse of the exact order
    led = min(float(l[lead]) - float(l[a]) for l in lt)
    depth = max(float(l.max()) - float(l[a]) for l in lt)
    hn, wn, babs = _norms(hl, W, b, h)
    acc = 2.0 ** -15.9 * (babs + hn * wn)
    assert led >= acc, what + (led, acc)
    eps = eps_of(hl, W, b, h)
    assert depth <= eps, what + (depth, eps)
    share = depth / (2 * eps)
    assert share >= SW.VARIANTS[variant]['floor'], what + (share,)
    _positions(case, ids, V1)
    first = SW.target_first(p['oseq'], p['tsel'])
    assert (first == a).all(), what + (first.tolist(),)
    assert not SW.target_first(p['ofr'], p['tsel']).any(), what
    frag = float(p['ofr'].mean())
    assert frag <= SW.FRAGILE_CAP, 'too many fragile (row, step)s (%.3f): change the seed, not the cap' % frag
    if case == 'end_token_wins':
        assert (p['oseq'][:, :, list(SW.TARGET_ROWS)] == 0).all()
    if case == 'negative_logits':
        assert z[a] < -20
    return dict(G=p['G'], eps=eps, exact=exact, ulps=exact / sp, lead=led, acc=acc, share=share, za=float(z[a]))


@pytest.mark.parametrize('case,vocab,variant', SW.plant_list(), ids=lambda v: str(v))
def test_planted_world_meets_its_preconditions(helper, case, vocab, variant):
    f = check_plant(helper, case, vocab, variant)
    print('%-22s %5d %-8s G %.2e eps %.2e exact a - b %.2e (%6.0f ulps) screened b - a %.2e (%5.1f x acc) depth / 2 eps %.3f'
          % (case, vocab, variant, f['G'], f['eps'], f['exact'], f['ulps'], f['lead'], f['lead'] / f['acc'], f['share']))


def test_the_case_lists_are_the_ones_the_worlds_name():
    names = set(SW.CASES)
    starred = {n for n, c in SW.CASES.items() if c['star']}
    assert starred == {'same_pair_lo', 'same_pair_hi', 'other_group_same_tile', 'other_tile', 'other_half', 'next_stage',
                       'far_stage', 'last_id_wins', 'triple_reversed', 'sigma_member'}
    assert len(names) == 16 and len(SW.plant_list()) == 15 + 20 and len(SW.starred_list()) == 20
    assert ('far_stage', 999, 'shallow') not in SW.plant_list()
    # the batch: the target image in every 32-row group of slab 0 and in slab 1
    w = SW.world(999)
    rows = list(SW.TARGET_ROWS)
    assert {r // 32 for r in rows if r < 128} == {0, 1, 2, 3} and max(rows) == SW.B - 1 >= 128
    assert all(np.array_equal(w['fc'][r], w['fc'][0]) for r in rows)
    assert len({w['fc'][r].tobytes() for r in range(SW.B)}) == SW.B - len(rows) + 1
    # the vocabularies' last stages
    assert (9488 + 63) // 64 == 149 and 9488 % 64 == 16 and 1000 % 64 == 40 and (64 + 63) // 64 == 1


@pytest.mark.parametrize('pr,vocab', SW.tie_list())
def test_positional_tie_meets_its_preconditions(pr, vocab):
    c = SW.tie_case(pr, vocab)
    twin, other, pick = c['twin'], c['other'], c['pick']
    V1 = c['dims'].V1
    assert 0 < twin < V1 and 0 < other < V1 and twin != other
    assert SW.pair(twin) == pr and SW.lane_half(twin) == SW.tie_hh(pr, vocab) and twin & 1
    assert SW.tie_hh(pr, 999) != SW.tie_hh(pr, 63)
    assert SW.lane_stage(twin) != SW.lane_stage(other)                  # each has its lane-stage's word to itself
    if vocab == 999:
        assert SW.stage(twin) != SW.stage(other) and pick == twin < other
        assert SW.lane_half(other) != SW.lane_half(twin) and SW.pair(other) == 15 - pr
    assert np.array_equal(c['W'][twin], c['W'][other]) and c['b'][twin] == c['b'][other]
    z = O.gemv(c['W'], c['b'], c['h'])
    assert z[twin].view(U32) == z[other].view(U32) and z[twin] == z.max()
    assert np.sort(z)[-3] < z[twin] - 1.0                               # nothing else near: a two-way tie
    tok, _, fragile = L.greedy_pick(z)
    assert tok == pick == min(twin, other) and fragile == 0
    assert (c['oseq'][0, 0, list(SW.TARGET_ROWS), 0] == pick).all()
    assert not (c['oseq'] == max(twin, other)).any()                    # bit-equal on every row: the higher id never wins
    assert c['ofr'].mean() <= SW.FRAGILE_CAP, 'too many fragile (row, step)s: change the seed, not the cap'
