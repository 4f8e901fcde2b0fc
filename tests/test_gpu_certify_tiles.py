"""The screened decode's wave-local tile certify ("bf16 screening"), on the GPU.

certify_tiles: every wave compacts the items behind its own lanes into a wave-private list, stages them 32 at a time
into a private tile and multiplies the tile with its own B operand on the fp32 MFMA pipe; lane (row, half) of the MFMA
holds the logits of the tile's slots (a & 3) + 8 (a >> 2) + 4 half, the owner of an item is the lane its id's bit 2
names, so the results cross lane halves through the item words. The test entry runs given (row, id) items of one
workgroup through exactly that function, in both owner modes (every item to lane half 0 of its row, or to the half its
id's bit 2 names, each lane's ids in increasing order as a decode's hit lists yield them). Every logit must be the fp32
MFMA tile's accumulator (nicnes_test_logit_chain's out_mfma[row, id]) bit for bit.

The lists aim at the places the function can go wrong: the tile boundary (31 / 32 / 33 items in a wave, 64 / 65), waves
with nothing to do beside busy ones, one wave far longer than the others, a wave over its batch (CERT_ITEMS items, then
the rest), one lane holding 64 ids while its partner half holds none, one staged row wanted by all 32 rows of a wave,
repeats, and the ids at both ends of the vocabulary and of the last, partly valid stage.

The decode itself always owns by id, and tests/test_gpu_certify.py's screened-against-unscreened cases (V = 9487, P = 3,
B = 40 among them) already run it end to end with screen_candidates > 0, so no end-to-end case is repeated here."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from oracle import oracle as O                                                  # noqa: E402
from tests.test_gpu_certify import _h128                                       # noqa: E402
from tests.test_gpu_screen import SIGMA, _engine                               # noqa: E402

CERT_ITEMS = 320                            # decode_kernel.hip: items of a wave's batch


def _in_group(rng, g, n, V1):
    """n random items of row group g (the 32 rows of one wave)"""
    return np.stack([32 * g + rng.integers(0, 32, n), rng.integers(0, V1, n)], 1)


def _item_lists(V1):
    rng = np.random.Generator(np.random.PCG64(2024))
    none = np.zeros((0, 2), np.int64)
    lists = {'empty': none}
    for k, c in enumerate((0, 1, 31, 32, 33, 64, 65)):
        lists['%d in one wave' % c] = _in_group(rng, k % 4, c, V1)
        lists['%d in every wave' % c] = np.concatenate([_in_group(rng, g, c, V1) for g in range(4)])
    lists['1000 in the last wave'] = _in_group(rng, 3, 1000, V1)
    lists['5, 700, 0, 64'] = np.concatenate([_in_group(rng, g, c, V1) for g, c in enumerate((5, 700, 0, 64))])
    # one lane with 64 ids over the stages, its partner half with none (by id: bit 2 set only, then clear only)
    for bit in (1, 0):
        pool = np.array([v for v in range(V1) if (v >> 2) & 1 == bit])
        ids = np.sort(pool[rng.integers(0, len(pool), 64)] if len(pool) < 64 else rng.choice(pool, 64, replace=False))
        lists['64 ids of one lane, bit 2 %s' % ('set' if bit else 'clear')] = np.stack([np.full(64, 37), ids], 1)
    lists['a batch and more in one wave'] = _in_group(rng, 2, 4096 + 7, V1)
    one_id = int(rng.integers(0, V1))
    lists['one id, every row of a wave'] = np.stack([32 + np.arange(32), np.full(32, one_id)], 1)
    lists['one item seven times'] = np.repeat(np.array([[70, one_id]]), 7, axis=0)
    last0 = 64 * ((V1 - 1) // 64)                                # first id of the last, partly valid stage
    edge = sorted({0, 1, V1 - 1, V1 - 2, last0, min(last0 + 31, V1 - 1), min(last0 + 32, V1 - 1)})
    lists['edge ids'] = np.array([[r, v] for r in (0, 31, 32, 127) for v in edge])
    return lists


@pytest.mark.parametrize('vocab', [9487, 999, 63])
@pytest.mark.parametrize('gain,bias_std', [(1.0, 0.0), (4.0, 0.1)])
def test_tile_certify_equals_the_mfma_tile_bit_for_bit(vocab, gain, bias_std):
    e = _engine(vocab)
    try:
        V1 = vocab + 1
        e.set_theta(O.make_theta(O.Dims(vocab_size=vocab), 0, gain, bias_std))
        h = _h128(5)
        lists = _item_lists(V1)
        assert max(len(v) for v in lists.values()) > 12 * CERT_ITEMS
        for sign in (0, 1):
            om = np.concatenate([e.test_logit_chain(7, 2, SIGMA, sign, h[32 * w: 32 * w + 32])[0].cpu().numpy()
                                 for w in range(4)])            # [128, V1], 32 rows per call
            assert np.isfinite(om).all()
            for name, items in lists.items():
                want = om[items[:, 0], items[:, 1]]
                for by_id in (False, True):
                    got = e.test_certify_items(7, 2, SIGMA, sign, h, items, owner_by_id=by_id).cpu().numpy()
                    assert got.shape == want.shape
                    ne = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
                    assert ne.size == 0, '%s, sign %d, by id %d: %d of %d logits differ, first item %s: %r against %r' % (
                        name, sign, by_id, ne.size, len(items), items[ne[:1]].tolist(), got[ne[:1]], want[ne[:1]])
    finally:
        e.close()
