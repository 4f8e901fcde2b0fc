"""CPU: the preconditions of the edge tests of the wide / layer-norm step-loop frame (tests/wide_edge_worlds.py; the GPU
side is tests/test_gpu_wide_edges.py). Each planted case is shown live on the references alone: the pick as stated with
fragile = 0, the raw argmax elsewhere where the case says so, the finishing steps that define a batch, at most 5 % of a
world's rows fragile. A GPU test that passes on a world whose precondition failed would prove nothing.

The figures that chose the constants of tests/wide_edge_worlds.py (printed by these tests with -s):

Tie worlds, V1 = 200, B = 40, xavier theta, lse = 5.29 .. 5.39, so the window is 2^-22.
  plain (256, 384), theta seed 0: tok = 42 on rows 0, 12, 29, logit 0.17 .. 0.23 (ulp 2^-26). Step 2^-25: k = +-2 puts
    a twin 4 logit ulps away, the triple's k = (2, 4) 4 and 8; all of k = 1 .. 7 (2 .. 14 ulps) stay in the window and
    not fragile, k = 8 (16 ulps = 2^-22) is fragile, k = 9 is out.
  ln (128, 256) affine, theta seed 10: tok = 108 on rows 0 and 10, logit 0.80 .. 0.88 (ulp 2^-24). Step 2^-24: k = +-2
    gives 2 ulps, the triple's k = (1, 3) 1 and 3; k = 4 (4 ulps = 2^-22) is fragile, k = 5 is out. Seeds whose tok has
    a logit above 1 on some row (ulp 2^-23, a window of 2 ulps) leave no room for a triple and were passed over.
  No row of any of the 16 planted worlds is fragile.
Early exits, V1 = 68, logit.bias[0] raised by 2.5, a pool of 600 rows, none fragile; fin = 0 .. 16:
  plain (256, 128): 167 46 36 24 20 22 27 15 9 8 10 7 6 3 5 5 190
  ln (128, 256) affine: 229 95 70 44 36 17 14 11 7 12 6 6 5 11 12 5 20
Full slabs: no fragile row among the 771 / 390 / 384 of plain (512, 512) B = 257, ln affine (512, 512) B = 130 and ln
  (256, 384) B = 128.
Vocabulary edges: no fragile row; the planted last id wins on 5 .. 32 of the 40 rows."""
import numpy as np
import pytest

from tests import wide_edge_worlds as W


@pytest.mark.parametrize('case', list(W.TIE_CASES))
@pytest.mark.parametrize('world', list(W.TIE_WORLDS))
def test_planted_tie_is_live_on_the_reference(world, case):
    ulps = W.check_tie_case(world, case)
    c = W.tie_case(world, case)
    print(world, case, 'tok', c['tok'], 'twins', c['twins'], 'pick', c['pick'], 'rows', c['rows'].tolist(),
          'ulps from tok', ulps, 'fragile rows', int(c['fr'].any(1).sum()))


@pytest.mark.parametrize('world', list(W.TIE_WORLDS))
def test_tie_world_window_leaves_room_for_whole_ulps(world):
    """flat logits: |z| < 2 and lse in [4, 8), so half an ulp of lse is 2^-22 and a logit ulp at most 2^-23"""
    w = W.tie_world(world)
    z = w['z1'].astype(np.float64)
    lse = np.log(np.exp(z).sum(1))
    assert np.abs(z).max() < 2 and lse.min() >= 4 and lse.max() < 8
    assert len(w['rows']) >= 2


@pytest.mark.parametrize('batch', list(W.EXIT_BATCHES))
@pytest.mark.parametrize('world', list(W.EXIT_WORLDS))
def test_exit_batch_finishes_where_it_says(world, batch):
    hist = W.check_exit_batch(world, batch)
    print(world, batch, 'fin histogram', hist.tolist())


@pytest.mark.parametrize('world', list(W.EXIT_WORLDS))
def test_exit_pool_spreads_the_finishing_steps(world):
    p = W.exit_pool(world)
    hist = np.bincount(p['fin'], minlength=W.T + 1)
    print(world, 'pool fin histogram', hist.tolist(), 'fragile rows', int((~p['ok']).sum()))
    assert (hist > 0).all()
    assert (~p['ok']).mean() <= W.FRAGILE_CAP


@pytest.mark.parametrize('world', list(W.FULL_WORLDS))
def test_full_slab_world_stays_within_the_fragile_cap(world):
    w = W.full_world(world)
    B = W.FULL_WORLDS[world]['B']
    assert B >= 128                                # every 32-row group of slab 0 holds valid rows
    frag = W.fragile_rows(w['bfr'], w['ofr'])
    print(world, 'fragile rows', int(frag.sum()), 'of', frag.size)
    assert frag.mean() <= W.FRAGILE_CAP, 'too many fragile rows (%d of %d): change the seed, not the cap' % (
        frag.sum(), frag.size)
    assert np.unique(w['oseq']).size >= 12
    assert not np.array_equal(w['oseq'][0], w['oseq'][1])          # the two signs are two models


@pytest.mark.parametrize('planted', [False, True], ids=['random', 'last_id'])
@pytest.mark.parametrize('cell,E,R,V1', W.VOCAB_WORLDS, ids=['%s_V%d' % (c[0], c[3]) for c in W.VOCAB_WORLDS])
def test_vocab_edge_world(cell, E, R, V1, planted):
    wins = W.check_vocab_world(cell, E, R, V1, planted)
    print(cell, V1, 'planted' if planted else 'random', 'rows with the last id', wins)
