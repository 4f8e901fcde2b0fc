"""nicnes.es.es_shard, the balanced split of a generation's pairs over ranks (include/nicnes_math.h nn_es_shard), and
the padded gather + compact of the torch binding of the fitness exchange."""
import numpy as np
import pytest
import torch

from nicnes.es import compact_shards, es_shard, pad_shard

CASES = [(500, 8), (8, 8), (9, 2), (4, 3)]


@pytest.mark.parametrize('n,world', CASES)
def test_shards_tile_the_pairs_in_rank_order(n, world):
    shards = [es_shard(n, r, world) for r in range(world)]
    at = 0
    for begin, count in shards:
        assert begin == at and count >= 1
        at += count
    assert at == n
    counts = [c for _, c in shards]
    assert max(counts) - min(counts) <= 1 and counts == sorted(counts, reverse=True)
    assert counts == [n // world + (1 if r < n % world else 0) for r in range(world)]


def test_the_eight_gpu_shares_of_mscoco_es():
    assert [es_shard(500, r, 8)[1] for r in range(8)] == [63, 63, 63, 63, 62, 62, 62, 62]
    assert [es_shard(4, r, 3) for r in range(3)] == [(0, 2), (2, 1), (3, 1)]


def test_fewer_pairs_than_ranks_raises():
    with pytest.raises(ValueError):
        es_shard(7, 0, 8)
    with pytest.raises(ValueError):
        es_shard(8, 8, 8)


@pytest.mark.parametrize('n,world', CASES)
def test_padded_gather_then_compact_is_the_concatenation(n, world):
    rng = np.random.Generator(np.random.PCG64(n * 31 + world))
    fit = torch.from_numpy(rng.standard_normal((n, 2)))
    fit[0, 1] = float('nan')
    fit[n - 1, 0] = -0.0
    shards = [fit[b:b + c].clone() for b, c in (es_shard(n, r, world) for r in range(world))]
    padded = [pad_shard(s, n, world) for s in shards]
    assert all(p.shape == (-(-n // world), 2) for p in padded)
    got = compact_shards(torch.cat(padded, 0), n, world)          # what all_gather_into_tensor leaves on every rank
    assert got.shape == (n, 2)
    assert np.array_equal(got.numpy().view(np.uint64), torch.cat(shards, 0).numpy().view(np.uint64))
