"""The screened decode's cooperative certify ("bf16 screening"), on the GPU.

Items == MFMA tile: the test entry (nicnes_test_certify_items) pushes given (row, id) items through the work queue,
the coalesced row staging, the fmaf chain and the result slots a screened decode certifies with; each logit must be
the fp32 MFMA tile's accumulator (nicnes_test_logit_chain's out_mfma) bit for bit, whatever the list's length, order
and skew.

Screened == unscreened under heavy certify load: theta and eps scales chosen on the CPU (the oracle's logits under the
kernel's window and lane-stage rule, fp64 forward along the oracle's tokens) so that a step's workgroup certifies
hundreds to thousands of items, many of them in crowded lane-stages:
  gain 0.05, scale 1     ~230 items per workgroup step (V = 9487, 999), ~1200 (V = 63); no lane over the cap
  gain 1, scale 8        up to ~1800 items per workgroup step (V = 9487), ~2400 (V = 999), 5120 (V = 63: every id of
                         every row); at V = 9487 / 999 some lanes go over the cap in 13 / 25 of 32 (sign, step)s, the
                         other steps are decided by the queue
  gain 1, scale 32       V = 63: every id of every row, no lane over the cap (one stage: two crowded hits). V = 9487 and
                         999: every lane is over the cap at every step and no row finishes, so every row sends every
                         step to the fp32 loop: there the certify has nothing to decide and only equality, the
                         candidate count and the fallback count itself are asserted
  40 tied ids, sigma 0   lane (row, half 0)'s 32 ids of stage 0 and 8 of stage 1 share one logit row and bias 30:
                         every row's lane half 0 holds 40 items, half 1 none; the lowest tied id is 0, the end token,
                         so every row ends at the first step

Counters: screen_candidates and screen_fallback_rows of one fixed evaluate are those of the commit before the
cooperative certify (pass 1 and the fallback conditions are unchanged)."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from oracle import oracle as O                                                  # noqa: E402
from tests.test_gpu_screen import SIGMA, _engine, _evaluator, _logit_views, _on_off     # noqa: E402

CERT_ROWS, CERT_BATCH = 192, 1536           # decode_kernel.hip: items of a round, of a batch


def _h128(seed):
    return np.random.Generator(np.random.PCG64(seed)).uniform(-1, 1, (128, 128)).astype(np.float32)


def _item_lists(V1):
    rng = np.random.Generator(np.random.PCG64(99))
    rnd = lambda n: np.stack([rng.integers(0, 128, n), rng.integers(0, V1, n)], 1)
    last0 = 64 * ((V1 - 1) // 64)                                # first id of the last, partly valid stage
    edge = sorted({0, 1, V1 - 1, V1 - 2, last0, min(last0 + 31, V1 - 1), min(last0 + 32, V1 - 1), max(last0 - 1, 0)})
    one_id = int(rng.integers(0, V1))
    return {
        'empty': np.zeros((0, 2), np.int64),
        'one': np.array([[77, V1 // 2]]),
        'round - 1': rnd(CERT_ROWS - 1), 'round': rnd(CERT_ROWS), 'round + 1': rnd(CERT_ROWS + 1),
        'batch - 1': rnd(CERT_BATCH - 1), 'batch': rnd(CERT_BATCH), 'batch + 1': rnd(CERT_BATCH + 1),
        'several batches': rnd(3 * CERT_BATCH + 700),
        'one row': np.stack([np.full(700, 45), rng.integers(0, V1, 700)], 1),
        'one row, a batch and more': np.stack([np.full(CERT_BATCH + 5, 127), rng.integers(0, V1, CERT_BATCH + 5)], 1),
        'one id, every row': np.stack([np.arange(128), np.full(128, one_id)], 1),
        'duplicates': np.repeat(rnd(50), 7, axis=0),
        'edge ids': np.array([[r, v] for r in (0, 31, 32, 127) for v in edge]),
        'random 2000': rnd(2000),
    }


@pytest.mark.parametrize('vocab', [9487, 999, 63])
@pytest.mark.parametrize('gain,bias_std', [(1.0, 0.0), (4.0, 0.1)])
def test_items_equal_the_mfma_tile_bit_for_bit(vocab, gain, bias_std):
    e = _engine(vocab)
    try:
        V1 = vocab + 1
        e.set_theta(O.make_theta(O.Dims(vocab_size=vocab), 0, gain, bias_std))
        h = _h128(5)
        lists = _item_lists(V1)
        for sign in (0, 1):
            om = np.concatenate([e.test_logit_chain(7, 2, SIGMA, sign, h[32 * w: 32 * w + 32])[0].cpu().numpy()
                                 for w in range(4)])            # [128, V1], 32 rows per call
            assert np.isfinite(om).all()
            for name, items in lists.items():
                got = e.test_certify_items(7, 2, SIGMA, sign, h, items).cpu().numpy()
                want = om[items[:, 0], items[:, 1]]
                assert got.shape == want.shape
                ne = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
                assert ne.size == 0, '%s, sign %d: %d of %d logits differ, first item %s: %r against %r' % (
                    name, sign, ne.size, len(items), items[ne[:1]].tolist(), got[ne[:1]], want[ne[:1]])
        import nicnes
        for bad in ([[0, V1]], [[3, 5], [4, V1 + 100]], [[0, -1]], [[128, 0]]):       # refused, not computed
            with pytest.raises(nicnes.NicnesError):
                e.test_certify_items(7, 2, SIGMA, 0, h, bad)
    finally:
        e.close()


def _tied_theta(vocab):
    dims = O.Dims(vocab_size=vocab)
    theta = O.make_theta(dims, 0, 4.0, 0.1).copy()
    W, b = _logit_views(dims, theta)
    # lane (row, half 0) holds ids 64 s + 32 c + 8 g + e (c < 2, g < 4, e < 4) of stage s: its 32 ids of stage 0 and
    # 8 of the next stage that exists (V = 63 has one stage: the 32 ids only, less the invalid ones)
    ids = [32 * c + 8 * g + e for c in range(2) for g in range(4) for e in range(4)] + \
          [64 + 8 * g + e for g in range(2) for e in range(4)]
    ids = [v for v in ids if v <= vocab]
    W[ids] = W[ids[0]]
    b[ids] = 30.0
    return theta


SHAPES = [(9487, 3, 40), (999, 2, 40), (63, 2, 40), (9487, 2, 128)]
LOADS = [('gain 0.05', None), ('gain 1', '8'), ('gain 1', '32'), ('tied', None)]


@pytest.mark.parametrize('vocab,P,B', SHAPES)
@pytest.mark.parametrize('load,scale', LOADS)
def test_screened_tokens_equal_the_fp32_loops_under_certify_load(monkeypatch, vocab, P, B, load, scale):
    dims = O.Dims(vocab_size=vocab)
    theta = (_tied_theta(vocab) if load == 'tied' else
             O.make_theta(dims, 0, 0.05 if load == 'gain 0.05' else 1.0, 0.0))
    e = _evaluator(monkeypatch, vocab, B, P, theta, env={'NICNES_SCREEN_EPS_SCALE': scale} if scale else None)
    try:
        seq, d = _on_off(e, P, sigma=0.0 if load == 'tied' else SIGMA)
        # the counter takes the rows of the workgroups' 128-row slabs, the padding rows of the last slab with them
        rows_steps = P * 2 * 128 * ((B + 127) // 128) * dims.T
        print('%s scale %s V %d P %d B %d: candidates %d, fallback rows %d of %d' % (
            load, scale, vocab, P, B, d['screen_candidates'], d['screen_fallback_rows'], rows_steps))
        assert d['screen_candidates'] > 0
        if scale == '32' and vocab != 63:
            # every lane over the cap at every step (module docstring): the fp32 loop decides them all
            assert 0 < d['screen_fallback_rows'] <= rows_steps
        else:
            assert d['screen_fallback_rows'] < rows_steps       # some step was decided by the certified records
        if load == 'tied':
            assert (seq == 0).all()                              # the lowest tied id: the end token
    finally:
        e.close()


# screen_candidates, screen_fallback_rows of _on_off(e, 3) (iteration 5, sigma 0.01, P = 3, B = 40, V = 9487) at commit
# 70cf890, the last with the per-lane certify
PARENT_COUNTERS = {(1.0, 0.0): (36392, 1), (4.0, 0.1): (58396, 3)}


@pytest.mark.parametrize('gain,bias_std', sorted(PARENT_COUNTERS))
def test_counters_are_the_per_lane_certifys(monkeypatch, gain, bias_std):
    e = _evaluator(monkeypatch, 9487, 40, 3, O.make_theta(O.Dims(), 0, gain, bias_std))
    try:
        _, d = _on_off(e, 3)
        assert (d['screen_candidates'], d['screen_fallback_rows']) == PARENT_COUNTERS[(gain, bias_std)]
    finally:
        e.close()
