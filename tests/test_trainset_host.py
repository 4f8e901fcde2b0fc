"""The resident training loader's host side (nicnes.data.ResidentTrainLoader, DrawnBatch) against CocoFcDataLoader on a
small dataset written here: the same image sequence, bounds, wrapped flags and rng draws, call for call; the packed fc
cache; one draw_batches call per iteration from the master. The engine is a stub that records calls. CPU only."""
import json
import os

import numpy as np
import pytest

from nicnes import data as Dt

F, T = 16, 16
SPLITS = ['train', 'val', 'train', 'restval', 'train', 'test', 'train', 'train', 'restval', 'train', 'train', 'val',
          'train', 'restval', 'test']                     # 8 train + 3 restval = 11 training images
NCAP = [1, 5, 3, 5, 6, 2, 7, 5, 1, 3, 6, 5, 7, 5, 5]          # both branches of get_captions (fewer than 5, and more)


@pytest.fixture()
def dataset(tmp_path):
    rng = np.random.default_rng(0)
    images = [{'id': 100 + i, 'split': sp, 'file_path': 'img%d.jpg' % i} for i, sp in enumerate(SPLITS)]
    with open(tmp_path / 'cocotalk.json', 'w') as f:
        json.dump({'ix_to_word': {str(i): 'w%d' % i for i in range(1, 30)}, 'images': images}, f)
    os.makedirs(tmp_path / 'fc')
    for im in images:
        np.save(tmp_path / 'fc' / ('%d.npy' % im['id']), rng.standard_normal(F).astype(np.float32))
    start = np.cumsum([0] + NCAP[:-1]) + 1
    labels = rng.integers(1, 30, (sum(NCAP), T))
    labels[:, 10:] = 0
    Dt.LabelStore(labels, start, start + np.array(NCAP) - 1).save_npz(str(tmp_path / 'labels.npz'))
    return tmp_path, images, labels, start


def _loader(tmp_path, **kw):
    return Dt.CocoFcDataLoader(str(tmp_path / 'cocotalk.json'), str(tmp_path / 'fc'), str(tmp_path / 'labels.npz'),
                               batch_size=4, **kw)


class StubSet:
    def __init__(self, fc, gts, fc_rows):
        self.fc = np.concatenate([np.asarray(fc[i:i + 4], np.float32) for i in range(0, fc.shape[0], 4)])  # by slices
        self.gts = [np.asarray(g) for g in gts]
        self._rows = fc_rows
        self.closed = False

    def fc_rows(self, ix):
        return self.fc[np.asarray(ix)] if self._rows is None else np.asarray(self._rows(ix), np.float32)

    def close(self):
        self.closed = True


class StubEngine:
    """Records what the loader and the master ask of an engine."""
    fitness_mode = 0

    def __init__(self):
        self.draws, self.sets, self.rpi = [], [], []

    def make_trainset(self, fc, gts, fc_rows=None):
        self.sets.append(StubSet(fc, gts, fc_rows))
        return self.sets[-1]

    def draw_batches(self, trainset, image_ix):
        self.draws.append((trainset, np.array(image_ix)))

    def set_rows_per_image(self, n):
        self.rpi.append(n)


def test_the_set_holds_every_training_image_once(dataset):
    tmp_path, images, labels, start = dataset
    e = StubEngine()
    R = Dt.ResidentTrainLoader(_loader(tmp_path), e)
    train = [i for i, sp in enumerate(SPLITS) if sp in ('train', 'restval')]
    assert R.images == train and len(train) == 11
    s = e.sets[0]
    assert s.fc.shape == (11, F)
    for r, ix in enumerate(train):
        assert np.array_equal(s.fc[r], np.load(tmp_path / 'fc' / ('%d.npy' % images[ix]['id'])))
        assert np.array_equal(s.gts[r], labels[start[ix] - 1: start[ix] - 1 + NCAP[ix]])
    assert R.vocab_size == 29 and R.seq_length == T          # the wrapped loader's attributes pass through


@pytest.mark.parametrize('seed', [0, 3])
@pytest.mark.parametrize('bs', [4, 5])
def test_batches_equal_the_host_loaders_call_for_call(dataset, seed, bs):
    """2.5 epochs of 11 images: batch sizes 4 and 5 both straddle the wrap."""
    tmp_path, images, labels, start = dataset
    H = _loader(tmp_path, seed=seed)
    R = Dt.ResidentTrainLoader(_loader(tmp_path, seed=seed), StubEngine())
    wraps = 0
    for call in range(-(-int(2.5 * 11) // bs)):
        hb = H.get_batch('train', batch_size=bs)
        rb = R.get_batch('train', batch_size=bs)
        assert isinstance(rb, Dt.DrawnBatch) and 'fc_feats' not in rb
        assert [R.images[r] for r in rb['image_ix']] == [x['ix'] for x in hb['infos']], call
        assert rb['infos'] == hb['infos'] and rb['bounds'] == hb['bounds'], call
        assert rb['seq_per_img'] == 5 and rb['image_ix'].dtype == np.int32
        # the rows the host batch carries are the set's rows at those indices
        assert np.array_equal(rb.fc_rows(), hb['fc_feats'][::5])
        for r, g in zip(rb['image_ix'], hb['gts']):
            assert np.array_equal(rb['trainset'].gts[r], g)
        wraps += bool(hb['bounds']['wrapped'])
        # the loaders' generators stay in step (get_captions draws differently for images with < 5 captions)
        assert R.loader.rng.getstate() == H.rng.getstate(), call
        assert R.loader.split_ix['train'] == H.split_ix['train']
    assert wraps == 2


def test_other_splits_delegate(dataset):
    tmp_path = dataset[0]
    H, R = _loader(tmp_path, seed=1), Dt.ResidentTrainLoader(_loader(tmp_path, seed=1), StubEngine())
    for split in ('val', 'test'):
        hb, rb = H.get_batch(split, batch_size=2), R.get_batch(split, batch_size=2)
        assert not isinstance(rb, Dt.DrawnBatch)
        assert np.array_equal(rb['fc_feats'], hb['fc_feats']) and rb['infos'] == hb['infos']
        assert np.array_equal(rb['labels'], hb['labels'])


def test_fc_cache_round_trips(dataset, monkeypatch):
    tmp_path = dataset[0]
    cache = str(tmp_path / 'train_fc.npy')
    e1 = StubEngine()
    R1 = Dt.ResidentTrainLoader(_loader(tmp_path), e1, fc_cache=cache)
    packed = np.load(cache)
    assert packed.shape == (11, F) and packed.dtype == np.float32 and np.array_equal(packed, e1.sets[0].fc)
    # a later start maps the file and opens no per-image file beyond the one that tells it F
    L2 = _loader(tmp_path)
    opened = []
    real = L2.fc_feature
    monkeypatch.setattr(L2, 'fc_feature', lambda ix: (opened.append(ix), real(ix))[1])
    e2 = StubEngine()
    R2 = Dt.ResidentTrainLoader(L2, e2, fc_cache=cache)
    assert len(opened) == 1 and np.array_equal(e2.sets[0].fc, packed)
    b1, b2 = R1.get_batch('train'), R2.get_batch('train')
    assert np.array_equal(b1['image_ix'], b2['image_ix']) and np.array_equal(b1.fc_rows(), b2.fc_rows())
    np.save(cache, np.zeros((3, F), np.float32))             # another split's file is refused
    with pytest.raises(ValueError):
        Dt.ResidentTrainLoader(_loader(tmp_path), StubEngine(), fc_cache=cache)


def _spec(fitness='greedy', single_batch=True):
    from nicnes import config as C
    exp = {'algorithm': 'nic_nes', 'dataset': 'mscoco', 'nb_offspring': 6,
           'config': {'noise_stdev': 0.05, 'batch_size': 4, 'l2coeff': 1e-3, 'snapshot_freq': 0,
                      'single_batch': single_batch},
           'policy_options': {'net': 'fc_caption', 'fitness': fitness},
           'optimizer_options': {'type': 'adam', 'args': {'stepsize': 0.01}}}
    return C.ExperimentSpec(exp, vocab_size=29)


def test_set_batch_makes_one_draw_for_a_list(dataset):
    from nicnes import master as M
    from nicnes.mutations import batch_fc
    tmp_path = dataset[0]
    e = StubEngine()
    R = Dt.ResidentTrainLoader(_loader(tmp_path), e)
    m = M.EngineMaster.__new__(M.EngineMaster)
    m.e, m._batch_key, m._n_batches = e, None, 1
    got = [R.get_batch('train') for _ in range(3)]
    m._set_batch(got)
    assert len(e.draws) == 1 and m._n_batches == 3
    ts, ix = e.draws[0]
    assert ts is R.trainset and ix.shape == (3, 4) and ix.dtype == np.int32
    assert np.array_equal(ix, np.stack([b['image_ix'] for b in got]))
    m._set_batch(got)                                        # the same object: nothing is drawn again
    assert len(e.draws) == 1
    one = R.get_batch('train', batch_size=5)
    m._set_batch(one)
    assert len(e.draws) == 2 and e.draws[1][1].shape == (1, 5) and m._n_batches == 1
    assert e.rpi == []                                       # greedy: rows_per_image is left alone
    e.fitness_mode = 5                                       # a sampled mode is told the batch's seq_per_img
    m._set_batch([R.get_batch('train')])
    assert e.rpi == [5]
    # the mutator's view of a drawn batch: the first batch's unique rows
    assert np.array_equal(batch_fc(got), got[0].fc_rows()) and batch_fc(got).shape == (4, F)


def test_batch_stream_draws_per_member_batches_and_counts_epochs(dataset):
    """_batch_stream is unchanged: it asks the resident loader as it asks the host loader, and sees the wrap."""
    from nicnes import master as M
    tmp_path = dataset[0]
    spec = _spec(single_batch=False)
    assert spec.batches_per_iteration == 6                   # one batch per member
    streams = []
    for make in (lambda: _loader(tmp_path, seed=2),
                 lambda: Dt.ResidentTrainLoader(_loader(tmp_path, seed=2), StubEngine())):
        m = M.EngineMaster.__new__(M.EngineMaster)
        m.spec, m.sched = spec, M.Schedule(spec.config, spec.nb_offspring)
        it = m._batch_stream(make())
        got = [next(it) for _ in range(2)]
        streams.append(([[x['ix'] for b in g for x in b['infos']] for g in got], m.sched.epoch))
    assert streams[0] == streams[1] and streams[0][1] >= 1


def test_run_dispatched_refuses_drawn_batches(dataset):
    """The dispatched path ships batches to other processes: it keeps host batches and says so."""
    from nicnes import master as M
    tmp_path = dataset[0]
    R = Dt.ResidentTrainLoader(_loader(tmp_path), StubEngine())
    m = M.EngineMaster.__new__(M.EngineMaster)
    m.spec, m.sched = _spec(), M.Schedule(_spec().config, 6)

    class Client:
        def declare_experiment(self, exp):
            pass
    with pytest.raises(ValueError, match='host loader'):
        m.run_dispatched(Client(), R, max_iterations=1)


def test_fc_cache_is_written_under_a_per_process_name(dataset):
    """Ranks that start together each build the cache: none may truncate a file another is writing or has mapped."""
    tmp_path = dataset[0]
    cache = str(tmp_path / 'train_fc.npy')
    other = cache + '.tmp.%d' % (os.getpid() + 1)            # another process's half-written file
    with open(other, 'wb') as f:
        f.write(b'partial')
    with open(cache + '.tmp', 'wb') as f:                    # and a fixed name, if anything still used one
        f.write(b'fixed')
    Dt.ResidentTrainLoader(_loader(tmp_path), StubEngine(), fc_cache=cache)
    assert open(other, 'rb').read() == b'partial' and open(cache + '.tmp', 'rb').read() == b'fixed'
    left = sorted(p for p in os.listdir(tmp_path) if p.startswith('train_fc.npy'))
    assert left == ['train_fc.npy', 'train_fc.npy.tmp', os.path.basename(other)]
    first = np.load(cache)
    mapped = np.load(cache, mmap_mode='r')                   # a rank that mapped this file ...
    os.remove(cache + '.tmp')
    os.remove(other)
    os.remove(cache)
    Dt.ResidentTrainLoader(_loader(tmp_path), StubEngine(), fc_cache=cache)    # ... keeps it when another replaces it
    assert np.array_equal(np.asarray(mapped), first) and np.array_equal(np.load(cache), first)
