"""nic_es generations sharded over ranks on the GPU: `python -m nicnes.es` as two ranks time-sharing one GPU over gloo
against the same command as one rank, the engine's C-ABI communicator at one rank against no communicator, and (where
the machine has two GPUs) two ranks over RCCL."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from oracle import oracle as O          # noqa: E402
from tests import es_ref as R           # noqa: E402
from tests import test_gpu_es as E      # noqa: E402  (ES_EXP and the world only)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'nes-img-captioning_amd')
GENERATIONS = 3
RANK_TIMEOUT = 240                      # seconds, each rank's own; a run takes a few


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(exp_path, dump, world, extra):
    """The ranks of one world as fresh child processes, each under its own timeout; every exit status is returned."""
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), PYTHONPATH=PKG + os.pathsep + os.environ.get('PYTHONPATH', ''))
        cmd = ['timeout', '-k', '10', str(RANK_TIMEOUT), sys.executable, '-m', 'nicnes.es', exp_path, '--synthetic',
               '--generations', str(GENERATIONS), '--seed', '3', '--noise_len', str(1 << 23), '--dump', dump] + extra
        procs.append(subprocess.Popen(cmd, env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate()[0] for p in procs]
    return [p.returncode for p in procs], outs


def _dump(d, rank):
    with open(os.path.join(d, 'rank%d.json' % rank)) as f:
        meta = json.load(f)
    return dict(np.load(os.path.join(d, 'rank%d.npz' % rank))), meta


def _same(a, b):
    (ra, ma), (rb, mb) = a, b
    assert np.array_equal(ra['parents'].view(np.uint32), rb['parents'].view(np.uint32))
    assert np.array_equal(ra['elites'].view(np.uint32), rb['elites'].view(np.uint32))
    for k in ('podium', 'cands', 'schedule', 'fitness', 'stats'):
        assert ma[k] == mb[k], k


@pytest.fixture(scope='module')
def one_rank(tmp_path_factory):
    d = tmp_path_factory.mktemp('es_cli')
    exp = str(d / 'es_exp.json')
    with open(exp, 'w') as f:
        json.dump(E.ES_EXP, f)
    codes, outs = _launch(exp, str(d / 'w1'), 1, ['--share-gpu', '--backend', 'gloo'])
    assert codes == [0], outs[0][-2000:]
    return d, exp, _dump(str(d / 'w1'), 0)


def test_two_ranks_sharing_the_gpu_equal_one_rank(one_rank):
    d, exp, one = one_rank
    codes, outs = _launch(exp, str(d / 'w2'), 2, ['--share-gpu', '--backend', 'gloo'])
    assert codes == [0, 0], '\n'.join(o[-2000:] for o in outs)
    r0, r1 = _dump(str(d / 'w2'), 0), _dump(str(d / 'w2'), 1)
    assert r0[1]['shard'] == [0, 2] and r1[1]['shard'] == [2, 2] and r0[1]['world'] == 2
    assert r0[1]['decode_path'] == 'fused'                   # ranks sharing a GPU keep the coop path off
    assert one[0]['parents'].shape[0] == E.ES_EXP['population_size'] and len(one[1]['fitness']) == GENERATIONS
    assert len(one[1]['podium']) == E.ES_EXP['num_elites']
    _same(r0, r1)
    _same(r0, one)


def test_engine_communicator_at_one_rank_equals_none():
    """EngineESMaster(comm='engine') at world size 1 (the only RCCL shape one GPU runs: the padded gather and the
    compaction as an identity) against comm=None, bit for bit; a count that is not the rank's share is refused."""
    import nicnes
    import nicnes.synthetic as S
    from nicnes.es import ESExperimentSpec, EngineESMaster
    from nicnes.validation import Validator
    dims, _, table = E._world()
    spec = ESExperimentSpec(E.ES_EXP)
    B = 16
    fc, gts, df, n = E._workload(B)
    start = [O.make_theta(dims, 40 + i, 4.0, 0.1) for i in range(6)]
    vfc = np.random.Generator(np.random.PCG64(77)).standard_normal((40, dims.F)).astype(np.float32)
    vbase, _, _ = O.decode(dims, start[0], vfc)
    vgts, _, _ = S.build_references(vbase, dims.vocab_size, seed=5, n_refs=5, df_sets=40)
    e = nicnes.Engine(**spec.engine_kwargs(noise_len=E.NOISE_LEN, noise_seed=E.SEED, max_batch=B))
    try:
        e.set_noise_table(table)
        keys, vals = nicnes.df_table_arrays(df)
        e.set_df_table(keys, vals, np.log(float(n)))
        val = Validator(e, R.FakeLoader(vfc, vgts), 'val', 40)
        runs = []
        for comm in (None, 'engine'):
            if comm:
                e.es_free()
                e.comm_init(1, 0, nicnes.Engine.comm_unique_id())
            m = EngineESMaster(spec, e, validator=val, seed=3, thetas=start, comm=comm)
            fits = []
            for _ in range(GENERATIONS):
                m.step((fc, gts))
                fits.append(m.last['fitness'].copy())
            runs.append((np.stack(fits), np.stack([e.es_row(i).cpu().numpy() for i in range(m.n_parents)]),
                         np.stack([e.es_row(i, 'elites').cpu().numpy() for i in range(2)]),
                         m.podium.best_elites(), m.sched.to_dict(), m.cands))
        a, b = runs
        for x, y in zip(a[:3], b[:3]):
            assert np.array_equal(x.view(np.uint32 if x.dtype == np.float32 else np.uint64),
                                  y.view(np.uint32 if y.dtype == np.float32 else np.uint64))
        assert a[3:] == b[3:]
        fl = torch.arange(8, dtype=torch.float64, device=e.device).reshape(4, 2)
        assert torch.equal(e.es_allgather_fitness(fl, 4), fl)
        with pytest.raises(nicnes.NicnesError, match='share'):
            e.es_allgather_fitness(fl[:3].contiguous(), 4)
        e.comm_destroy()
        val.close()
    finally:
        e.close()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='two ranks over RCCL need two GPUs; this machine shows %d'
                    % torch.cuda.device_count())
@pytest.mark.parametrize('comm', ['torch', 'engine'])
def test_two_ranks_over_rccl_equal_one_rank(one_rank, comm):
    d, exp, one = one_rank
    out = str(d / ('rccl_' + comm))
    codes, outs = _launch(exp, out, 2, ['--backend', 'nccl', '--comm', comm])
    assert codes == [0, 0], '\n'.join(o[-2000:] for o in outs)
    r0, r1 = _dump(out, 0), _dump(out, 1)
    _same(r0, r1)
    _same(r0, one)
