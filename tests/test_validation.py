"""CPU: the host side of validation-split evaluation (nicnes.validation, EngineMaster(validator=...),
python -m nicnes.evaluate) on a stub engine built from the oracle, and the known answers of the BLEU / ROUGE_L
restatement the GPU scorer tests compare against (tests/coco_metrics_ref.py)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from nicnes import config as C
from nicnes import data as Dt
from nicnes import master as M
from nicnes import validation as V
from oracle import cider_ref as CR
from oracle import oracle as O
from tests import coco_metrics_ref as R
from tests.cpu_engine import OracleEngine, tiny_workload

T = 16


def row(*w):
    return list(w) + [0] * (T - len(w))


# ---------------------------------------------------------------- the restatement's own known answers
def test_restatement_bleu_known_answers():
    assert R.bleu_stats([5, 6, 7, 8, 9], [[5, 6, 7, 8, 9]]) == [5, 4, 3, 2, 5, 4, 3, 2, 5, 5]
    assert all(abs(b - 1.0) <= 1e-9 for b in R.bleu_from_totals([5, 4, 3, 2, 5, 4, 3, 2, 5, 5]))
    assert R.bleu_stats([20, 21, 22, 23], [[10, 11, 12, 13]]) == [0, 0, 0, 0, 4, 3, 2, 1, 4, 4]
    assert all(b <= 1e-9 for b in R.bleu_from_totals([0, 0, 0, 0, 4, 3, 2, 1, 4, 4]))
    assert R.bleu_stats([], [[14, 15, 16]]) == [0, 0, 0, 0, 0, 0, 0, 0, 0, 3]            # empty: length 0, no division
    assert all(math.isfinite(b) and b <= 1e-9 for b in R.bleu_from_totals([0, 0, 0, 0, 0, 0, 0, 0, 0, 3]))
    assert R.bleu_stats([30], [[30, 31, 32]]) == [1, 0, 0, 0, 1, 0, 0, 0, 1, 3]          # one word: guess[2..4] = 0
    s = R.bleu_stats([40, 41, 42, 43], [[40, 41, 42, 43, 44, 45]])                       # brevity penalty
    assert s == [4, 3, 2, 1, 4, 3, 2, 1, 4, 6]
    assert all(abs(b - math.exp(1 - 6 / 4)) <= 1e-8 for b in R.bleu_from_totals(s))
    # |6 - 5| == |4 - 5|: the shorter reference length
    assert R.bleu_stats([80, 81, 82, 88, 89], [[80, 81, 82, 83, 84, 85], [80, 81, 86, 87]])[8:] == [5, 4]
    # a repeated word is clipped by the max over the references
    assert R.bleu_stats([50, 50, 50, 50], [[50, 51, 52, 53], [50, 50, 54, 55]])[:4] == [2, 1, 0, 0]


def test_restatement_rouge_known_answers():
    assert R.lcs([60, 61, 62, 63], [60, 70, 62, 71, 63]) == 3           # not a common substring
    p, r, b2 = 3 / 4, 3 / 5, 1.44
    assert abs(R.rouge_l([60, 61, 62, 63], [[60, 70, 62, 71, 63]]) - (1 + b2) * p * r / (r + b2 * p)) <= 1e-15
    assert R.rouge_l([1, 2, 3, 4], [[1, 2, 3, 4]]) == 1.0
    assert R.rouge_l([1, 2], [[3, 4]]) == 0.0 and R.rouge_l([], [[3, 4]]) == 0.0
    # P and R are maximised separately over the references
    assert abs(R.rouge_l([1, 2, 3], [[1, 2, 3, 4, 5, 6], [1, 9]]) - (1 + b2) * 1.0 * 0.5 / (0.5 + b2 * 1.0)) <= 1e-15


# ---------------------------------------------------------------- corpus_df, decode_sequence
def _random_gts(rng, n_img, vocab=30):
    gts = []
    for _ in range(n_img):
        refs = []
        for _ in range(int(rng.integers(1, 6))):
            L = int(rng.integers(0, T + 1))
            refs.append(row(*[int(t) for t in rng.integers(1, vocab, L)]))
        gts.append(np.asarray(refs, np.int32))
    return gts


def test_corpus_df_equals_the_oracle():
    gts = _random_gts(np.random.Generator(np.random.PCG64(1)), 30)
    keys, vals = V.corpus_df(gts)
    df, n = CR.document_frequency_from_refs([[R.as_str(R.words(r)) for r in g] for g in gts])
    assert n == 30
    assert {tuple(str(t) for t in V.unpack_ngram(k)): v for k, v in zip(keys, vals)} == df
    assert keys.dtype == np.uint64 and bool(np.all(keys[1:] > keys[:-1]))
    assert not any(0 in V.unpack_ngram(k) for k in keys)             # no n-gram holds the end token
    k0, v0 = V.corpus_df([])
    assert k0.size == 0 and v0.size == 0


def test_decode_sequence():
    vocab = {str(i): 'w%d' % i for i in range(1, 10)}
    seq = np.asarray([row(1, 2, 3), row(), row(*range(1, 10), 1, 2, 3, 4, 5, 6, 7), [4, 0, 5] + [0] * 13])
    assert V.decode_sequence(vocab, seq) == ['w1 w2 w3', '', ' '.join('w%d' % (i % 9 + 1) for i in range(16)), 'w4']
    assert V.decode_sequence({1: 'a', 2: 'b'}, [[2, 1, 0]]) == ['b a']


# ---------------------------------------------------------------- a stub engine with make_split
class StubSplit:
    def __init__(self, engine, fc, gts):
        self.e, self.fc, self.gts, self.closed = engine, np.asarray(fc, np.float32), gts, False

    def evaluate(self, return_seq=False):
        seq, _, _ = O.decode(self.e.dims, self.e.theta32, self.fc)
        _, m, _ = R.corpus_metrics(seq, self.gts)
        return (m, seq) if return_seq else m

    def close(self):
        self.closed = True


class StubEngine(OracleEngine):
    def make_split(self, fc, gts=None, df=None, ref_len_raw=None):
        self.last_split = StubSplit(self, fc, gts)
        return self.last_split


DIMS = dict(vocab_size=29, E=32, R=32, F=16)


def _stub_engine():
    dims = O.Dims(**DIMS)
    theta = O.make_theta(dims, 2, 4.0, 0.1)
    return StubEngine(dims, theta, np.zeros((3, 16), np.float32), [], {}, 8.0, O.noise_table(1 << 16, 123))


def stub_engine_factory(spec, args):
    """--engine_factory tests.test_validation:stub_engine_factory"""
    return _stub_engine()


@pytest.fixture()
def dataset(tmp_path):
    rng = np.random.default_rng(0)
    splits = ['train', 'val', 'test', 'val', 'train', 'val', 'restval', 'val', 'test']
    images = [{'id': 100 + 7 * i, 'split': sp, 'file_path': 'img%d.jpg' % i} for i, sp in enumerate(splits)]
    info = {'ix_to_word': {str(i): 'w%d' % i for i in range(1, 30)}, 'images': images}
    with open(tmp_path / 'cocotalk.json', 'w') as f:
        json.dump(info, f)
    os.makedirs(tmp_path / 'fc')
    for im in images:
        np.save(tmp_path / 'fc' / ('%d.npy' % im['id']), rng.standard_normal(16).astype(np.float32))
    ncap = [5, 6, 2, 5, 7, 5, 1, 5, 3]
    start = np.cumsum([0] + ncap[:-1]) + 1
    labels = rng.integers(1, 30, (sum(ncap), 16))
    labels[:, 10:] = 0
    Dt.LabelStore(labels, start, start + np.array(ncap) - 1).save_npz(str(tmp_path / 'labels.npz'))
    loader = Dt.CocoFcDataLoader(str(tmp_path / 'cocotalk.json'), str(tmp_path / 'fc'), str(tmp_path / 'labels.npz'),
                                 batch_size=3)
    return tmp_path, loader, images, labels, start, ncap


def test_validator_takes_the_first_num_images_in_split_order(dataset):
    tmp_path, loader, images, labels, start, ncap = dataset
    e = _stub_engine()
    assert loader.split_ix['val'] == [1, 3, 5, 7]
    v = V.Validator(e, loader, 'val', num=3)
    assert v.ixs == [1, 3, 5] and v.image_ids == [107, 121, 135]
    assert e.last_split.fc.shape == (3, 16)
    for k, ix in enumerate(v.ixs):
        assert np.array_equal(e.last_split.fc[k], np.load(tmp_path / 'fc' / ('%d.npy' % images[ix]['id'])))
        assert np.array_equal(v.gts[k], labels[start[ix] - 1: start[ix] - 1 + ncap[ix]])     # every label row
    stats, preds = v.eval_split(incl_gts=True)
    assert sorted(stats) == sorted(V.METRIC_KEYS)
    assert [p['image_id'] for p in preds] == [107, 121, 135]
    seq, _, _ = O.decode(e.dims, e.theta32, e.last_split.fc)
    assert [p['caption'] for p in preds] == V.decode_sequence(loader.ix_to_word, seq)
    assert preds[1]['gts'] == V.decode_sequence(loader.ix_to_word, v.gts[1]) and len(preds[1]['gts']) == 5
    assert 'gts' not in v.eval_split()[1][0]
    assert len(V.Validator(e, loader, 'val', num=-1).ixs) == 4 and len(V.Validator(e, loader, 'val', num=50).ixs) == 4
    assert V.Validator(e, loader, 'test', num=1).image_ids == [114]
    from nicnes.nes import EnginePolicy
    assert EnginePolicy(e).accuracy_on(v) == float(stats['CIDEr'])
    loader.split_ix['val'] = []
    with pytest.raises(ValueError):
        V.Validator(e, loader, 'val')


# ---------------------------------------------------------------- the master: podium of one, patience
class Scripted:
    """a validator whose scores are given"""

    def __init__(self, scores):
        self.scores, self.calls = list(scores), 0

    def eval_split(self, incl_gts=False):
        self.calls += 1
        return {'CIDEr': self.scores[self.calls - 1]}, []


def _master(tmp_path, name, validator, **cfg):
    dims, theta, fc, gts, df, n, table = tiny_workload()
    e = OracleEngine(dims, theta, fc, gts, df, n, table)
    exp = {'algorithm': 'nic_nes', 'dataset': 'mscoco', 'nb_offspring': 4,
           'config': dict({'noise_stdev': 0.05, 'batch_size': 4, 'l2coeff': 1e-3, 'snapshot_freq': 1}, **cfg),
           'policy_options': {'net': 'fc_caption', 'fitness': 'greedy'},
           'optimizer_options': {'type': 'adam', 'args': {'stepsize': 0.01}}}
    m = M.EngineMaster(C.ExperimentSpec(exp, vocab_size=dims.vocab_size), e, log_dir=str(tmp_path / name),
                       theta=theta, validator=validator)
    return m, [(fc, gts)] * 8


def test_patience_rule_over_a_scripted_score_sequence(tmp_path):
    """good, bad, bad, bad with patience 2 -> one curriculum step; then a new best"""
    v = Scripted([1.0, 0.5, 1.0, 0.25, 2.0])
    m, batches = _master(tmp_path, 'p', v, patience=2, stdev_divisor=2.0, bs_multiplier=1.0, stepsize_divisor=4.0)
    best = os.path.join(str(tmp_path / 'p'), 'models', 'best', 'best_elite', '0_0_elite.pth')
    seen = []

    for k in range(1, 6):
        m.run(batches, max_iterations=k)
        seen.append((m.sched.bad_generations, m.sched.noise_stdev, m.opt.stepsize, m.sched.patience_reached,
                     open(best, 'rb').read()))
    assert v.calls == 5
    assert [s[0] for s in seen] == [0, 1, 2, 0, 0]                     # the counter, reset by the step and by a best
    assert [s[1] for s in seen] == [0.05, 0.05, 0.05, 0.025, 0.025]    # one curriculum step, at the third bad one
    assert [s[2] for s in seen] == [0.01, 0.01, 0.01, 0.0025, 0.0025]  # ... which divides the step size once
    assert [s[3] for s in seen] == [False, False, False, True, False]
    assert seen[0][4] == seen[1][4] == seen[2][4] == seen[3][4] != seen[4][4]      # written only on improvement
    assert [r['val_score'] for r in m.stats] == [1.0, 0.5, 1.0, 0.25, 2.0]
    assert [r['best_val_score'] for r in m.stats] == [1.0, 1.0, 1.0, 1.0, 2.0]
    # the best theta of iteration 1 is the theta that iteration evaluated: the start theta
    dims, theta = tiny_workload()[:2]
    from nicnes.nes import vector_from_state_dict, param_shapes
    first = vector_from_state_dict(torch.load(__import__('io').BytesIO(seen[0][4]), weights_only=True), param_shapes(m.e))
    assert np.array_equal(first.numpy().astype(np.float32), theta)
    info = [f for f in os.listdir(tmp_path / 'p' / 'snapshot') if f.startswith('z_info')]
    z = json.load(open(tmp_path / 'p' / 'snapshot' / info[0]))
    assert z['best_elites'] == [[best, 2.0]] and z['bad_generations'] == 0


def test_patience_zero_disables_the_rule(tmp_path):
    v = Scripted([1.0, 0.5, 0.5, 0.5, 0.5])
    m, batches = _master(tmp_path, 'z', v, patience=0, stdev_divisor=2.0, stepsize_divisor=4.0)
    m.run(batches, max_iterations=5)
    assert m.sched.bad_generations == 0 and m.sched.noise_stdev == 0.05 and m.opt.stepsize == 0.01


PARENT_STAT_KEYS = ['iter', 'update_ratio', 'score_mean', 'score_max', 'score_min', 'noise_stdev', 'batch_size',
                    'step_time']
PARENT_INFO_KEYS = ['iter', 'epoch', 'noise_stdev', 'batch_size', 'bad_generations', 'times_orig_bs',
                    'nb_samples_used', 'current_model', 'optimizer_state', 'stats']


def test_without_a_validator_nothing_changes(tmp_path):
    """validator=None: the stats rows and the snapshot carry exactly the keys they had, no best-elite directory
    appears, and the run's numbers are those of a validated run (validation reads theta, it changes nothing)"""
    m0, batches = _master(tmp_path, 'a', None, patience=2, stdev_divisor=2.0, stepsize_divisor=4.0)
    m0.run(batches, max_iterations=4)
    m1, _ = _master(tmp_path, 'b', Scripted([4.0, 3.0, 2.0, 1.0]), patience=0, stdev_divisor=2.0, stepsize_divisor=4.0)
    m1.run(batches, max_iterations=4)
    assert [list(r) for r in m0.stats] == [PARENT_STAT_KEYS] * 4
    assert m0.sched.bad_generations == 0 and m0.sched.noise_stdev == 0.05 and m0.opt.stepsize == 0.01
    assert not os.path.exists(tmp_path / 'a' / 'models' / 'best')
    snap = tmp_path / 'a' / 'snapshot'
    z = json.load(open(snap / [f for f in os.listdir(snap) if f.startswith('z_info')][0]))
    assert list(z) == PARENT_INFO_KEYS
    for r0, r1 in zip(m0.stats, m1.stats):
        assert all(r0[k] == r1[k] for k in PARENT_STAT_KEYS if k != 'step_time'), (r0, r1)
    assert torch.equal(m0.e.theta()[0], m1.e.theta()[0])


# ---------------------------------------------------------------- python -m nicnes.evaluate
def test_evaluate_cli_json_shape(dataset, tmp_path):
    from nicnes import evaluate as E
    from nicnes.nes import state_dict_from_vector, param_shapes
    dpath = dataset[0]
    e = _stub_engine()
    model = str(tmp_path / 'theta.pth')
    torch.save(state_dict_from_vector(torch.from_numpy(e.theta32), param_shapes(e)), model)
    exp = {'algorithm': 'nic_nes', 'dataset': 'mscoco', 'nb_offspring': 4,
           'config': {'noise_stdev': 0.05, 'batch_size': 3, 'num_val_items': 2},
           'policy_options': {'net': 'fc_caption', 'fitness': 'greedy',
                              'model_options': {'input_encoding_size': 32, 'rnn_size': 32, 'fc_feat_size': 16}},
           'caption_options': {'input_json': 'cocotalk.json', 'input_fc_dir': 'fc', 'input_label_h5': 'labels.npz'}}
    exp_path = str(tmp_path / 'exp.json')
    json.dump(exp, open(exp_path, 'w'))
    out = str(tmp_path / 'eval.json')
    common = ['--exp', exp_path, '--model', model, '--data_root', str(dpath), '--out', out,
              '--engine_factory', 'tests.test_validation:stub_engine_factory']
    assert E.main(common + ['--split', 'val']) == 0
    res = json.load(open(out))
    assert sorted(res) == ['predictions', 'stats'] and sorted(res['stats']) == sorted(V.METRIC_KEYS)
    assert all(isinstance(res['stats'][k], float) for k in V.METRIC_KEYS)
    assert [p['image_id'] for p in res['predictions']] == [107, 121]               # config.num_val_items = 2
    assert all(sorted(p) == ['caption', 'image_id'] and isinstance(p['caption'], str) for p in res['predictions'])
    assert E.main(common + ['--split', 'test', '--num', '-1', '--incl_gts']) == 0
    res = json.load(open(out))
    assert [p['image_id'] for p in res['predictions']] == [114, 156] and len(res['predictions'][0]['gts']) == 2


# ---------------------------------------------------------------- the reference wire's eval result
@pytest.mark.parametrize('validated', [False, True])
def test_reference_wire_eval_score_is_the_validation_cider(tmp_path, validated):
    import threading
    from nicnes import nes as N
    from nicnes import refwire as W
    from nicnes import transport as Tr
    dims, theta, fc, gts, df, n, table = tiny_workload()
    eng = OracleEngine(dims, theta, fc, gts, df, n, table)
    path = str(tmp_path / '0_current_params.pth')
    torch.save(N.state_dict_from_vector(torch.from_numpy(theta), N.param_shapes(eng)), path)
    exp = {'algorithm': 'nic_nes', 'dataset': 'mscoco', 'nb_offspring': 4,
           'config': {'noise_stdev': 0.05, 'batch_size': 4, 'l2coeff': 1e-3, 'single_batch': True},
           'policy_options': {'net': 'fc_caption', 'fitness': 'greedy'},
           'optimizer_options': {'type': 'adam', 'args': {'stepsize': 0.01}}}
    spec = C.ExperimentSpec(exp, vocab_size=dims.vocab_size)
    store = Tr.LocalStore()
    mc = Tr.MasterClient(store, codec=W.RefPickleCodec)           # plays the reference master
    mc.declare_experiment(spec.exp)
    batch = {'fc_feats': np.repeat(fc, 5, axis=0), 'gts': gts, 'labels': np.zeros((20, 18), dtype='int')}
    tid = mc.declare_task(W.RefNESTask(current=path, batch_data=batch, noise_stdev=0.05, log_dir=str(tmp_path),
                                       batch_size=4))
    worker = N.EngineWorker(eng, spec, worker_id=11)
    v = Scripted([0.875] * 64) if validated else None
    stop = threading.Event()
    th = threading.Thread(target=W.run_reference_worker, daemon=True,
                          args=(Tr.WorkerClient(store, codec=W.RefPickleCodec), worker),
                          kwargs=dict(chunk=2, eval_prob=1.0, seed=0, stop=stop, validator=v))
    th.start()
    try:
        t, r = mc.pop_result(timeout=60)
    finally:
        stop.set()
        th.join(60)
    assert t == tid and r.fitness is None
    want = 0.875 if validated else float(eng.evaluate_theta(0)[0])   # default: the training batch's fitness
    assert r.eval_score == want
