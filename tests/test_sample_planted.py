"""CPU: the oracle's planted draws (oracle.decode_sample_planted) and its restatement of the engine's draw stream
(oracle.sample_draws). The planted draws are what tests/test_gpu_sample_pick.py aims the GPU's sampled pick with; here
they are checked against the oracle's own sampled decode: fed back through oracle.decode_sample they give the targets
at every position, none flagged fragile, every candidate id of the world is hit, and every draw sits at least
MIN_HALF_WIDTH (1e-5, ten times the suite's U_MARGIN) from both ends of its interval, so that a different summation
order of the probabilities cannot move a boundary across it."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import sample_worlds as W
from tests.test_oracle_golden import U_MARGIN


@pytest.mark.parametrize('world', W.PLANTED_WORLDS)
def test_planted_draws_give_the_targets(world):
    tg = W.targets(world)
    u, hw, seq, lp = W.planted(world)
    cand = W.candidates(world)
    print('%s: %d positions, %d candidates, min half-width %.3g' % (world, tg.size, len(cand), hw.min()))
    assert W.MIN_HALF_WIDTH >= 10 * U_MARGIN
    assert hw.min() >= W.MIN_HALF_WIDTH, hw.min()
    assert (u > 0).all() and (u < 1).all()
    assert np.array_equal(seq, tg)                            # no target is 0: no row ends
    assert set(np.unique(tg)) == set(cand.tolist())           # every candidate is hit
    oseq, olp, ofr = W.decode_with(world, u)
    assert np.array_equal(oseq, tg)
    assert not ofr.any()
    assert np.array_equal(olp.view(np.int32), lp.view(np.int32))


def test_candidates_cover_the_boundaries():
    """The candidate sets hold what they are for: both sides of the block boundary 7|8 in every world that has one, of
    the level-1 round boundary (stages 159|160) where V1 > 10240, every column of the tail stage, and in the stairs
    worlds the ids either side of each step and spike."""
    want = {'flat': 783, 'wc': 783, 'stairs': 793, 'v16384': 1279, 'stairs1000': 428, 'v68': 67, 'v60': 59, 'v8': 7}
    for world in W.PLANTED_WORLDS:
        c = set(W.candidates(world).tolist())
        V1 = W.WORLDS[world]['vocab'] + 1
        nst = (V1 + 63) // 64
        assert len(c) == want[world], (world, len(c))
        assert set(range(max(1, 64 * (nst - 1)), V1)) <= c
        if nst > 8:
            assert {511, 512} <= c
        if nst > 160:
            assert {64 * 160 - 1, 64 * 160} <= c
        for s in W.WORLDS[world].get('steps', ()):
            assert {64 * s - 1, 64 * s} <= c
        for v in W.WORLDS[world].get('spikes', ()):
            assert {v - 1, v, v + 1} <= c


def test_planted_rows_that_end():
    """A target of 0 ends the row: seq is 0 from there on while the draws go on (it = tok * unfinished), and the
    oracle's sampled decode of the planted draws agrees on every position."""
    world = 'stairs1000'
    tg = W.targets(world).copy()
    tg[0, 0, 3, 5] = 0
    tg[0, 1, :, 3] = 0
    u, hw, seq, lp = W.plant(world, tg)
    assert hw.min() >= W.MIN_HALF_WIDTH
    want = tg.copy()
    want[0, 0, 3, 5:] = 0
    want[0, 1, :, 3:] = 0
    assert np.array_equal(seq, want)
    assert (lp[0, 1, :, 4:] == 0).all() and (lp[0, 1, :, :4] != 0).all()      # the global early exit's zeros
    assert (lp[0, 0] != 0).all()
    oseq, olp, ofr = W.decode_with(world, u)
    assert np.array_equal(oseq, want) and not ofr.any()
    assert np.array_equal(olp.view(np.int32), lp.view(np.int32))


def test_planted_rejects_targets_outside_the_vocabulary():
    d = W.dims('v8')
    tg = np.full((40, d.T), d.V1, np.int32)
    with pytest.raises(ValueError):
        O.decode_sample_planted(d, W.theta('v8'), W.fc('v8'), tg)


def test_sample_draws_stream():
    seed, it, B, T = 7, 3, 5, 4
    a = O.sample_draws(seed, it, 0, 3, B, T)
    assert a.shape == (3, 2, B, T) and a.dtype == np.float64
    assert (a >= 0).all() and (a < 1).all()
    assert np.array_equal(O.sample_draws(seed, it, 2, 1, B, T)[0], a[2])
    b = O.sample_draws(seed, it + 1, 0, 3, B, T)
    assert not (a == b).any()
    assert len(np.unique(a)) == a.size
    # the 53-bit formula by hand: splitmix64 written out, member m0 + k, r the flat index in [2, B, T]
    M = (1 << 64) - 1

    def sm(x):
        z = (x + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    for (k, s, r, t) in [(0, 0, 0, 0), (1, 0, 2, 3), (2, 1, 4, 1), (0, 1, 0, 0), (2, 1, 4, 3)]:
        key = sm(seed ^ 0x6a09e667f3bcc909 ^ ((it << 32) | k))
        flat = (s * B + r) * T + t
        want = (sm(key ^ flat) >> 11) / float(1 << 53)
        assert a[k, s, r, t] == want, (k, s, r, t)
    # the eval rollouts' member
    e = O.sample_draws(seed, it, 0xffffffff, 1, B, T)
    key = sm(seed ^ 0x6a09e667f3bcc909 ^ ((it << 32) | 0xffffffff))
    assert e[0, 1, 2, 3] == (sm(key ^ ((B + 2) * T + 3)) >> 11) / float(1 << 53)
