"""Host side of nic_es (nicnes.es): the experiment reader, the parent draws, the podium and the wire codec. No GPU."""
import copy
from collections import Counter

import numpy as np
import pytest

from nicnes.config import NotSupported
from nicnes.es import ESExperimentSpec, ESTask, ESResult, Podium, draw_parents, tournament_draws, splitmix64

ES_JSON = {     # the shape of mscoco_es.json
    'algorithm': 'nic_es', 'dataset': 'mscoco', 'nb_offspring': 1000, 'population_size': 50, 'num_elites': 3,
    'num_elite_cands': 2, 'selection': 'uniform', 'tournament_size': 5, '_from_single': 'disabled.pth',
    'config': {'noise_stdev': 0.005, 'batch_size': 256, 'patience': 10, 'stdev_divisor': 1.2, 'bs_multiplier': 1.0,
               'snapshot_freq': 10, 'num_val_items': 5000, 'l2coeff': 0.0, 'eval_prob': 0.02},
    'policy_options': {'net': 'fc_caption', 'fitness': 'greedy',
                       'model_options': {'safe_mutations': 'SM-PROPORTIONAL', 'rnn_size': 128,
                                         'input_encoding_size': 128, 'fc_feat_size': 2048}},
}


def _exp(**over):
    e = copy.deepcopy(ES_JSON)
    for k, v in over.items():
        if v is None:
            e.pop(k, None)
        else:
            e[k] = v
    return e


def test_spec_reads_an_es_experiment():
    s = ESExperimentSpec(ES_JSON)
    assert (s.nb_offspring, s.n_pairs, s.population_size, s.num_elites, s.num_elite_cands) == (1000, 500, 50, 3, 2)
    assert s.selection == 'uniform' and s.mutation == 'SM-PROPORTIONAL' and s.fitness == 'greedy'
    assert s.sigma == 0.005 and s.batch_size == 256 and s.config.patience == 10
    assert '_from_single' not in s.exp and 'from_single' not in s.exp
    kw = s.engine_kwargs(noise_len=1 << 24, noise_seed=7)
    assert kw['max_members'] == 500 and kw['max_batch'] == 256 and kw['vocab_size'] == 9487
    # population_size defaults to nb_offspring (nic_es/experiment.py:16); tournament needs its size
    assert ESExperimentSpec(_exp(population_size=None)).population_size == 1000
    assert ESExperimentSpec(_exp(selection='tournament')).tournament_size == 5


@pytest.mark.parametrize('over', [
    {'algorithm': 'nic_nes'}, {'nb_offspring': 999}, {'selection': 'roulette'},
    {'selection': 'tournament', 'tournament_size': None}, {'num_elites': 50}, {'num_elite_cands': 48},
    {'population_size': 1200}, {'dataset': 'mnist'},
])
def test_spec_refusals(over):
    with pytest.raises(NotSupported):
        ESExperimentSpec(_exp(**over))


def test_spec_refuses_options_outside_the_engine():
    for key, val in (('fitness', 'sample'), ('fitness', 'self_critical'), ('net', 'att_caption')):
        e = _exp()
        e['policy_options'][key] = val
        with pytest.raises(NotSupported):
            ESExperimentSpec(e)
    for sm in ('SM-G-SUM', 'SM-VECTOR', 'SM-G-ABS'):
        e = _exp()
        e['policy_options']['model_options']['safe_mutations'] = sm
        with pytest.raises(NotSupported):
            ESExperimentSpec(e)


def test_draw_parents_deterministic_in_range_sorted():
    for sel, k in (('uniform', None), ('tournament', 4)):
        a = draw_parents(5, 3, 500, 50, sel, k)
        assert a.dtype == np.int32 and a.shape == (500,)
        assert np.array_equal(a, draw_parents(5, 3, 500, 50, sel, k))
        assert a.min() >= 0 and a.max() < 50
        assert (np.diff(a) >= 0).all()
        raw = draw_parents(5, 3, 500, 50, sel, k, sort_parents=False)
        assert not (np.diff(raw) >= 0).all()
        assert Counter(raw.tolist()) == Counter(a.tolist())          # the same multiset, only reordered
        assert not np.array_equal(raw, draw_parents(5, 4, 500, 50, sel, k, sort_parents=False))   # per generation
        assert not np.array_equal(raw, draw_parents(6, 3, 500, 50, sel, k, sort_parents=False))   # per seed
    # the pair's draw does not depend on how many pairs are drawn (shards agree)
    assert np.array_equal(draw_parents(5, 3, 500, 50, sort_parents=False)[:20],
                          draw_parents(5, 3, 20, 50, sort_parents=False))
    u = draw_parents(1, 1, 5000, 50, sort_parents=False)
    assert len(set(u.tolist())) == 50 and np.bincount(u).min() > 50      # uniform: every parent, about 100 each
    assert (draw_parents(1, 1, 9, 1) == 0).all()
    with pytest.raises(ValueError):
        draw_parents(1, 1, 4, 0)
    with pytest.raises(ValueError):
        draw_parents(1, 1, 4, 3, 'roulette')


def test_tournament_is_the_minimum_of_distinct_draws():
    for key in (1, 2, 12345):
        for n, k in ((50, 5), (3, 5), (7, 7), (10, 1)):
            picks = tournament_draws(key, n, k)
            assert len(picks) == min(n, k) == len(set(picks))
            assert all(0 <= p < n for p in picks)
    # draw_parents takes each pair's minimum
    from nicnes.es import _PARENT_STREAM, MASK64
    raw = draw_parents(9, 2, 6, 20, 'tournament', 3, sort_parents=False)
    for pair in range(6):
        key = splitmix64((9 ^ _PARENT_STREAM ^ ((2 << 32) | pair)) & MASK64)
        assert raw[pair] == min(tournament_draws(key, 20, 3))
    # more draws pull the winner towards slot 0 (the best parent), as the lowest index of the tournament does
    assert draw_parents(1, 1, 2000, 50, 'tournament', 8).mean() < draw_parents(1, 1, 2000, 50, 'tournament', 2).mean() \
        < draw_parents(1, 1, 2000, 50, 'uniform').mean()
    # a tournament over all the parents always finds slot 0
    assert (draw_parents(1, 1, 50, 6, 'tournament', 6) == 0).all()


def test_podium_hand_worked():
    p = Podium(3)
    assert p.best_elites() == [] and p.is_bad_generation()
    # fewer candidates than places: both enter, best first; the bottom place is written first
    moves = p.record_elites([('a', 1.0, 4), ('b', 2.0, 5)])
    assert p.best_elites() == [('b', 2.0), ('a', 1.0)]
    assert moves == [(1, 'parents', 4), (0, 'parents', 5)]
    assert p.is_bad_generation() is False and p.is_bad_generation() is True     # the flag resets once read
    # a tie with a held elite keeps the held one ahead (stable sort, held first); c enters between, a moves down
    moves = p.record_elites([('c', 2.0, 7), ('d', 0.5, 8)])
    assert p.best_elites() == [('b', 2.0), ('c', 2.0), ('a', 1.0)]
    assert moves == [(2, 'elites', 1), (1, 'parents', 7)]
    assert p.is_bad_generation() is False
    # a generation that adds nothing: worse candidates, and no candidates at all
    assert p.record_elites([('e', 0.9, 2), ('f', 1.0, 3)]) == []
    assert p.best_elites() == [('b', 2.0), ('c', 2.0), ('a', 1.0)] and p.is_bad_generation() is True
    assert p.record_elites([]) == [] and p.is_bad_generation() is True
    # a new best pushes every place down and the last elite off
    moves = p.record_elites([('g', 5.0, 1)])
    assert p.best_elites() == [('g', 5.0), ('b', 2.0), ('c', 2.0)]
    assert moves == [(2, 'elites', 1), (1, 'elites', 0), (0, 'parents', 1)]
    assert p.is_bad_generation() is False
    # two candidates of equal score: the earlier one first
    q = Podium(1)
    q.record_elites([('x', 1.0, 0), ('y', 1.0, 1)])
    assert q.best_elites() == [('x', 1.0)]


def test_podium_moves_replayed_on_rows():
    """Applying the moves in order to a row table gives the podium's order (no row is read after it was overwritten)."""
    rng = np.random.Generator(np.random.PCG64(3))
    p, rows = Podium(4), [None] * 4
    for gen in range(30):
        cands = [('g%dc%d' % (gen, i), float(np.round(rng.standard_normal(), 1)), i) for i in range(int(rng.integers(0, 4)))]
        for place, table, src in p.record_elites(cands):
            rows[place] = cands[src][0] if table == 'parents' else rows[src]
        assert rows[:len(p.best_elites())] == [k for k, _ in p.best_elites()]
        scores = [sc for _, sc in p.best_elites()]
        assert scores == sorted(scores, reverse=True)


def test_codec_round_trip():
    from nicnes import transport as T
    task = ESTask(elites=[(0, 4), (1, 5)], parents=[(i, i) for i in range(6)], noise_stdev=0.005,
                  batch_data={'fc_feats': np.arange(12, dtype=np.float32).reshape(3, 4)}, log_dir='logs/x')
    back = T.deserialize(T.serialize(task))
    assert isinstance(back, ESTask) and back._fields == ESTask._fields
    assert back.parents == [(i, i) for i in range(6)] and back.elites == [(0, 4), (1, 5)]
    assert back.noise_stdev == 0.005 and back.elite is None and back.ref_batch is None
    assert np.array_equal(back.batch_data['fc_feats'], task.batch_data['fc_feats'])
    res = ESResult(worker_id=3, evaluated_model_id=2, evaluated_model=(17, 1), fitness=np.array([41.5]), mem_usage=123)
    back = T.deserialize(T.serialize(res))
    assert isinstance(back, ESResult) and back.evaluated_model == (17, 1) and back.evaluated_model_id == 2
    assert back.fitness.dtype == np.float64 and back.fitness[0] == 41.5 and back.score is None
    ev = T.deserialize(T.serialize(ESResult(worker_id=1, evaluated_cand_id=0, evaluated_cand=4, score=0.93)))
    assert ev.evaluated_cand_id == 0 and ev.evaluated_cand == 4 and ev.score == 0.93 and ev.fitness is None
    # the reference's field names (nic_es_master.py:27-34)
    assert ESResult._fields == ('worker_id', 'evaluated_model_id', 'fitness', 'evaluated_model', 'eval_return',
                                'mem_usage', 'evaluated_cand', 'evaluated_cand_id', 'score')
    assert ESTask._fields == ('elite', 'population', 'batch_data', 'parents', 'noise_stdev', 'log_dir', 'elites',
                              'ref_batch')


def test_exports_name_the_es_group():
    from nicnes import _lib
    es = sorted(n for n in _lib.EXPORTS if n.startswith('nicnes_es_'))
    assert es == sorted(['nicnes_es_create', 'nicnes_es_free', 'nicnes_es_set_mutation', 'nicnes_es_set_parent',
                         'nicnes_es_set_parent_count', 'nicnes_es_get_row', 'nicnes_es_row_stats',
                         'nicnes_es_evaluate', 'nicnes_es_offspring', 'nicnes_es_select', 'nicnes_es_advance',
                         'nicnes_es_set_elite', 'nicnes_es_load_theta'])
