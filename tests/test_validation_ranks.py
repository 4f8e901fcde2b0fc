"""CPU, gloo, two ranks: EngineMaster with validation on every rank. Rank 0 holds the validator and scores; the score
is shared in a collective, so both ranks record the same val_score / best_val_score and their schedules (the patience
rule's curriculum step) move alike; rank 1 passes validator=True and never scores."""
import json
import os
import socket

import torch.distributed as dist
import torch.multiprocessing as mp

from nicnes import config as C
from nicnes import master as M
from tests.cpu_engine import OracleEngine, tiny_workload

SCORES = [1.0, 0.5, 0.25]


class _Scripted:
    def __init__(self):
        self.calls = 0

    def eval_split(self, incl_gts=False):
        self.calls += 1
        return {'CIDEr': SCORES[self.calls - 1]}, []


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(rank, world, port, out_dir):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        dims, theta, fc, gts, df, n, table = tiny_workload()
        e = OracleEngine(dims, theta, fc, gts, df, n, table)
        exp = {'algorithm': 'nic_nes', 'dataset': 'mscoco', 'nb_offspring': 4,
               'config': {'noise_stdev': 0.05, 'batch_size': 4, 'l2coeff': 1e-3, 'snapshot_freq': 0, 'patience': 1,
                          'stdev_divisor': 2.0, 'stepsize_divisor': 2.0},
               'policy_options': {'net': 'fc_caption', 'fitness': 'greedy'},
               'optimizer_options': {'type': 'adam', 'args': {'stepsize': 0.01}}}
        v = _Scripted() if rank == 0 else True
        m = M.EngineMaster(C.ExperimentSpec(exp, vocab_size=dims.vocab_size), e,
                           log_dir=os.path.join(out_dir, 'log%d' % rank), rank=rank, world_size=world, theta=theta,
                           validator=v)
        for k in range(1, 4):
            m.run([(fc, gts)] * 4, max_iterations=k)
        with open(os.path.join(out_dir, 'r%d.json' % rank), 'w') as f:
            json.dump({'val': [r['val_score'] for r in m.stats], 'best': [r['best_val_score'] for r in m.stats],
                       'sigma': [r['noise_stdev'] for r in m.stats], 'stepsize': m.opt.stepsize,
                       'bad': m.sched.bad_generations, 'calls': v.calls if rank == 0 else 0,
                       'best_file': os.path.exists(m.best_model_path())}, f)
    finally:
        dist.destroy_process_group()


def test_rank0_validates_and_every_rank_follows(tmp_path):
    mp.spawn(_run, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a, b = [json.load(open(tmp_path / ('r%d.json' % r))) for r in range(2)]
    assert a['calls'] == 3
    for r in (a, b):
        assert r['val'] == SCORES and r['best'] == [1.0, 1.0, 1.0]
        assert r['sigma'] == [0.05, 0.05, 0.025]            # bad, bad with patience 1: one curriculum step
        assert r['stepsize'] == 0.005 and r['bad'] == 0
    assert a['best_file'] and not b['best_file']            # rank 0 writes the best theta
