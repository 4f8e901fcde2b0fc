"""nicnes.es.EngineESMaster over gloo ranks on the CPU (tests/cpu_es_engine.OracleESEngine): 4 pairs over worlds of 2
(shards 2, 2) and 3 (shards 2, 1, 1), 3 generations of tournament selection with a scripted validator. Every rank must
end each run with the single-rank run's parents, elites, podium, candidates, schedule and stats, bit for bit; only rank 0
validates and writes snapshots; a NaN in one rank's shard raises DecodeFault on every rank and records nothing."""
import json
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import oracle as O
from tests.cpu_engine import tiny_workload
from tests.cpu_es_engine import OracleESEngine, ScriptedValidator

GENERATIONS = 3
ES_EXP = {
    'algorithm': 'nic_es', 'dataset': 'mscoco', 'nb_offspring': 8, 'population_size': 6, 'num_elites': 2,
    'num_elite_cands': 2, 'selection': 'tournament', 'tournament_size': 2,
    'config': {'noise_stdev': 0.02, 'batch_size': 4, 'patience': 1, 'stdev_divisor': 2.0, 'bs_multiplier': 1.0,
               'snapshot_freq': 1},
    'policy_options': {'net': 'fc_caption', 'fitness': 'greedy', 'model_options': {}},
}


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _state(m, eng):
    return {'parents': np.stack(eng.parents), 'elites': np.stack([eng.elites[i] for i in sorted(eng.elites)]),
            'n_parents': m.n_parents,
            'meta': json.dumps({'podium': m.podium.best_elites(), 'cands': m.cands, 'schedule': m.sched.to_dict(),
                                'stats': [{k: v for k, v in r.items() if k != 'step_time'} for r in m.stats]})}


def _run(rank, world, port, out_dir):
    from nicnes import DecodeFault
    from nicnes.es import ESExperimentSpec, EngineESMaster, es_shard
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    if world > 1:
        dist.init_process_group('gloo', rank=rank, world_size=world)
    dims, _, fc, gts, df, n, table = tiny_workload()
    spec = ESExperimentSpec(ES_EXP, vocab_size=dims.vocab_size)
    eng = OracleESEngine(dims, fc, gts, df, n, table, max_members=spec.n_pairs, noise_seed=5)
    val = ScriptedValidator(eng)
    start = [O.make_theta(dims, 40 + i, 4.0, 0.1) for i in range(spec.population_size)]
    log_dir = os.path.join(out_dir, 'w%d' % world, 'log%d' % rank)
    m = EngineESMaster(spec, eng, validator=val, log_dir=log_dir, seed=3, thetas=start, rank=rank, world_size=world)
    assert m.shard == es_shard(spec.n_pairs, rank, world)
    assert eng.decode == (('fused', 0) if world == 1 else ('auto', 0))
    m.run([(fc, gts)] * GENERATIONS, generations=GENERATIONS)
    assert eng.evaluated == [(g, m.shard[0], m.shard[1]) for g in range(1, GENERATIONS + 1)]
    done = _state(m, eng)
    # a NaN in the last rank's shard (pair 3 of the next generation): every rank raises, nothing is recorded
    eng.nan_at = (GENERATIONS + 1, spec.n_pairs - 1)
    calls = val.calls
    raised = False
    try:
        m.step((fc, gts))
    except DecodeFault:
        raised = True
    after = _state(m, eng)
    same = all(np.array_equal(done[k], after[k]) if isinstance(done[k], np.ndarray) else done[k] == after[k] for k in done)
    np.savez(os.path.join(out_dir, 'r%d_w%d.npz' % (rank, world)), parents=done['parents'], elites=done['elites'],
             n_parents=done['n_parents'], meta=done['meta'], val_calls=calls, val_calls_after_fault=val.calls,
             raised=raised, unchanged_by_fault=same, snapshot=os.path.isdir(os.path.join(log_dir, 'models')))
    if world > 1:
        dist.destroy_process_group()


@pytest.fixture(scope='module')
def single(tmp_path_factory):
    d = tmp_path_factory.mktemp('es_ranks')
    _run(0, 1, _free_port(), str(d))
    return d, dict(np.load(d / 'r0_w1.npz'))


@pytest.mark.parametrize('world', [2, 3])
def test_every_rank_equals_the_single_rank_run(single, world):
    d, one = single
    mp.spawn(_run, args=(world, _free_port(), str(d)), nprocs=world, join=True)
    assert int(one['val_calls']) == GENERATIONS * ES_EXP['num_elite_cands'] and bool(one['snapshot'])
    for rank in range(world):
        r = np.load(d / ('r%d_w%d.npz' % (rank, world)))
        assert np.array_equal(r['parents'].view(np.uint32), one['parents'].view(np.uint32)), rank
        assert np.array_equal(r['elites'].view(np.uint32), one['elites'].view(np.uint32)), rank
        assert int(r['n_parents']) == int(one['n_parents'])
        assert str(r['meta']) == str(one['meta']), rank                 # podium, candidates, schedule, stats
        assert int(r['val_calls']) == (int(one['val_calls']) if rank == 0 else 0), 'only rank 0 validates'
        assert bool(r['snapshot']) == (rank == 0), 'only rank 0 writes snapshots'
        assert bool(r['raised']) and bool(r['unchanged_by_fault']), 'rank %d after a NaN in the last shard' % rank
        assert int(r['val_calls_after_fault']) == int(r['val_calls'])
    assert bool(one['raised']) and bool(one['unchanged_by_fault'])
