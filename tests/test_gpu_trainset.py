"""GPU: the resident training set (nicnes_trainset_*, nicnes_draw_batches, nicnes.data.ResidentTrainLoader).

A draw must leave the handle in the state nicnes_set_batches leaves for host-assembled batches of the same images in
the same order. The gathered buffers are byte copies and the same kernels then run on them, so EVERY comparison here is
bit for bit (torch.equal / np.array_equal on the raw outputs): there is no tolerance to choose.

The data: 37 images with random fc rows; the references derive from the engine's own greedy captions of theta
(nicnes.synthetic.substituted_refs), so the CIDEr-D scores are not all zero. Data set 'r8' has 1-8 references per image
(the image-table scorer), 'r9' has images with 9 (the per-reference scan). Two configurations: F = 128 with
seq_length 16, F = 384 with seq_length 7 (28-byte reference rows: not 16-byte aligned), vocabulary 59."""
import ctypes
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

NOISE_LEN = 1 << 22
N = 37
VOCAB = 59
SIGMA = 0.01
P = 4
CFGS = {'F128_T16': (128, 16), 'F384_T7': (384, 7)}
# The fc gather moves a row in groups of 8 wave-wide 16-byte pieces (512 float4) and finishes with a piece-by-piece tail:
# F = 128 and 384 are all tail. F = 2048 (the default) is exactly one group and no tail; F = 2176 is one group and a
# half-wave tail piece in the same row; F = 4480 is two groups and a tail of one and a half pieces.
WIDE = {'F2048_T16': (2048, 16), 'F2176_T16': (2176, 16), 'F4480_T7': (4480, 7)}
ALL = {**CFGS, **WIDE}
_cache = {}


def _theta(F, T):
    import nicnes.synthetic as S
    return S.init_theta(S.Dims(VOCAB, 128, 128, F, T), 5, 4.0, 0.1)


def _table():
    if 'table' not in _cache:
        import nicnes.synthetic as S
        _cache['table'] = S.noise_table(NOISE_LEN, 123)
    return _cache['table']


def _engine(cfg, max_batch=130, max_refs=None, members=P):
    import nicnes
    F, T = ALL[cfg]
    e = nicnes.Engine(vocab_size=VOCAB, fc_feat_size=F, seq_length=T, max_batch=max_batch, max_refs=max_refs,
                      max_members=members, noise_len=NOISE_LEN, noise_seed=7)
    e.set_noise_table(_table())
    e.set_theta(_theta(F, T))
    return e


def _data(cfg, e=None):
    """(fc [N, F], {'r8': gts, 'r9': gts}, df, n) of a configuration, made once with any engine of that
    configuration (the captions the references derive from are the engine's greedy decode of theta)."""
    import nicnes.synthetic as S
    if cfg not in _cache:
        F, T = ALL[cfg]
        own = e is None
        e = e or _engine(cfg, max_batch=8)
        try:
            fc = S.fc_feats(N, F, 900 + F)
            sp = e.make_split(fc)
            base = sp.decode().cpu().numpy()
            sp.close()
        finally:
            if own:
                e.close()
        rng = np.random.Generator(np.random.PCG64(17))
        counts8 = [1 + (3 * i) % 8 for i in range(N)]                     # 1..8, image 0 has 1, image 36 has 5
        counts9 = list(counts8)
        for i in (5, 20, 36):
            counts9[i] = 9
        gts = {k: [S.substituted_refs(base[i], VOCAB, rng, c, T) for i, c in enumerate(cs)]
               for k, cs in (('r8', counts8), ('r9', counts9))}
        assert max(g.shape[0] for g in gts['r8']) == 8 and min(g.shape[0] for g in gts['r8']) == 1
        df = {}
        for refs in gts['r8'] + gts['r9']:
            grams = set()
            for r in refs:
                grams |= S._row_ngrams(r, T)
            for g in grams:
                df[g] = df.get(g, 0.0) + 1.0
        df2 = {g: v + 3.0 for g, v in list(df.items())[::2]}              # another table: other scores
        fc.setflags(write=False)
        _cache[cfg] = (fc, gts, df, 2 * N, df2)
    return _cache[cfg]


def _set_df(e, df, n):
    import nicnes
    keys, vals = nicnes.df_table_arrays(df)
    e.set_df_table(keys, vals, np.log(float(n)))


@pytest.fixture(scope='module')
def engines():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    made = {}

    def get(cfg):
        if cfg not in made:
            e = _engine(cfg)
            fc, gts, df, n, _ = _data(cfg, e)
            _set_df(e, df, n)
            made[cfg] = (e, {k: e.make_trainset(fc, g) for k, g in gts.items()})
        return made[cfg]
    yield get
    for e, sets in made.values():
        for ts in sets.values():
            ts.close()
        e.close()


def _indices(G, B, seed=0):
    """[G, B] image indices holding image 0, image N - 1, image 0 twice inside a batch (B >= 3) and in two batches
    (G > 1)."""
    ix = np.random.default_rng(100 * G + B + seed).integers(0, N, (G, B)).astype(np.int32)
    ix[0, 0] = 0
    if B >= 3:
        ix[0, 1] = 0                      # image 0 twice inside batch 0
    if G > 1:
        ix[1, 0] = 0                      # ... and in two batches
    ix[-1, -1] = N - 1                    # (B = 1, G = 1: the one image is N - 1)
    return ix


def _host_batches(cfg, kind, ix):
    fc, gts = _data(cfg)[0], _data(cfg)[1][kind]
    return [(fc[row], [gts[i] for i in row]) for row in ix]


def _n_refs(cfg, kind, ix):
    gts = _data(cfg)[1][kind]
    return int(sum(gts[i].shape[0] for i in ix.ravel()))


def _state(e, n_refs=None):
    out = e.test_batch_state(n_refs)
    torch.cuda.synchronize()
    return [t.clone() for t in out]


def _same(a, b, what=''):
    """Bit-for-bit equality of two result dicts (or tensor lists)."""
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            _same(a[k], b[k], k)
        return
    if isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, '%s[%d]' % (what, i))
        return
    a, b = a.contiguous(), b.contiguous()
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), what       # raw bytes: NaN and -0 count too


# ---------------------------------------------------------------------------------------------- 1. batch state
@pytest.mark.parametrize('G', [1, 3])
@pytest.mark.parametrize('B', [1, 3, 33, 130])
@pytest.mark.parametrize('cfg', list(CFGS))
def test_batch_state_equals_set_batches(engines, cfg, B, G):
    e, sets = engines(cfg)
    for kind in (('r8', 'r9') if B == 33 else ('r8',)):
        ix = _indices(G, B)
        nr = _n_refs(cfg, kind, ix)
        e.set_batches(_host_batches(cfg, kind, ix))
        want = _state(e, nr)
        e.set_batches(_host_batches(cfg, kind, _indices(G, B, seed=1)))      # other bytes in between
        e.draw_batches(sets[kind], ix if G > 1 else ix[0])
        assert e.B == B and e.n_batches == G
        got = _state(e, nr)
        _same(got, want, 'state')
        fc, gts = _data(cfg)[0], _data(cfg)[1][kind]
        assert np.array_equal(got[0].cpu().numpy(), fc[ix.ravel()])          # and they are the images asked for
        assert np.array_equal(got[1].cpu().numpy(), np.concatenate([gts[i] for i in ix.ravel()]))
        assert got[2][0].item() == 0 and got[2][-1].item() == nr


@pytest.mark.parametrize('cfg', list(WIDE))
def test_wide_rows_take_the_unrolled_gather(cfg):
    """Rows of 512 float4 and more: the fc gather's unrolled main loop (every default-dims run takes it), alone and
    handing over to the tail inside one row. Bit for bit against set_batches and against the numpy gather, the
    evaluates too; every float of a row is distinct enough that a misplaced piece shows."""
    fc, gts, df, n, _ = _data(cfg)
    assert ALL[cfg][0] // 4 >= 512
    e = _engine(cfg, max_batch=33)
    try:
        _set_df(e, df, n)
        ts = e.make_trainset(fc, gts['r8'])
        for G, B in ((1, 33), (3, 5), (1, 1)):
            ix = _indices(G, B)
            nr = _n_refs(cfg, 'r8', ix)
            e.set_batches(_host_batches(cfg, 'r8', ix))
            want, want_res = _state(e, nr), _results(e, G, B, sampled=False)
            e.set_batches(_host_batches(cfg, 'r8', _indices(G, B, seed=1)))
            e.draw_batches(ts, ix)
            got = _state(e)                                  # sized from the handle's own starts
            _same(got, want, 'state')
            assert np.array_equal(got[0].cpu().numpy().view(np.uint32), fc[ix.ravel()].view(np.uint32))
            _same(_results(e, G, B, sampled=False), want_res)
        with pytest.raises(ValueError, match='reference rows'):
            e.test_batch_state(nr + 1)                       # a wrong count is refused before any copy
        ts.close()
    finally:
        e.close()


def test_chunked_upload_and_write_fc_ranges():
    """Host rows go into the set chunk by chunk (nicnes_trainset_write_fc), at chunk sizes that do and do not divide N;
    a range outside the set is refused."""
    import nicnes
    from nicnes import _lib
    from nicnes.engine import TrainSet
    cfg = 'F128_T16'
    fc, gts, df, n, _ = _data(cfg)
    e = _engine(cfg, max_batch=40)
    try:
        _set_df(e, df, n)
        ix = np.arange(N, dtype=np.int32)[None]
        for chunk in (5, 37, 4096):
            class Chunked(TrainSet):
                CHUNK_ROWS = chunk
            ts = Chunked(e, fc, gts['r8'])
            e.draw_batches(ts, ix)
            assert np.array_equal(_state(e)[0].cpu().numpy(), fc)
            rows = np.ascontiguousarray(fc[:2])
            for first, count in ((-1, 2), (N - 1, 2), (0, 0), (N, 1)):
                rc = e.L.nicnes_trainset_write_fc(e.h, ts.ts, first, count, rows.ctypes.data_as(ctypes.c_void_p), e._stream())
                assert rc == _lib.ERR_INVALID, (first, count)
            e.draw_batches(ts, ix)
            assert np.array_equal(_state(e)[0].cpu().numpy(), fc)            # nothing was written
            ts.close()
        with pytest.raises(nicnes.NicnesError):
            e.draw_batches(ts, ix)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------- 2. evaluates
def _results(e, G, B, sampled=True):
    """Everything an evaluate can return on the batches held, as GPU tensors."""
    T = e.cfg.seq_length
    mb = [(2 * k + 1) % G for k in range(P)] if G > 1 else None
    out = {}
    e.set_fitness_mode('greedy')
    out['lp'] = list(e.evaluate(3, 0, P, SIGMA, return_seq=True, return_lp=True, member_batch=[k % G for k in range(P)]
                                if G > 1 else None))
    if G > 1:
        out['map'] = list(e.evaluate(4, 1, P - 1, SIGMA, return_seq=True, member_batch=mb[:P - 1]))
    out['theta'] = [list(e.evaluate_theta(batch=k, return_seq=True, return_lp=True)) for k in range(G)]
    rows = np.random.default_rng(5).integers(0, VOCAB + 1, (4, B, T)).astype(np.int32)
    rows[:, :, T - 1] = 0
    out['rows'] = list(e.test_score_rows(rows, member_batch=[G - 1, 0] if G > 1 else None))
    out['sens'] = e.sum_sensitivity(min(B, 8), 0.1).clone()
    if sampled:
        e.set_fitness_mode('sample')
        e.set_rows_per_image(5)
        e.set_sample_draws(np.random.default_rng(6).random((2, 2, B * 5, T)))
        try:
            out['sample'] = list(e.evaluate(5, 0, 2, SIGMA, return_seq=True, member_batch=mb[:2] if G > 1 else None))
        finally:
            e.set_sample_draws(None)
            e.set_rows_per_image(1)
            e.set_fitness_mode('greedy')
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('kind', ['r8', 'r9'])
@pytest.mark.parametrize('cfg', list(CFGS))
def test_evaluates_equal_set_batches(engines, cfg, kind):
    """kind r8: the image-table scorer; r9: the per-reference scan (an image with 9 references is in every draw)."""
    e, sets = engines(cfg)
    for G, B in ((3, 33), (1, 9)):
        ix = _indices(G, B)
        if kind == 'r9':
            ix[0, -2] = 20
        e.set_batches(_host_batches(cfg, kind, ix))
        want = _results(e, G, B)
        assert float(want['lp'][0].abs().sum()) > 0                          # scores that could differ
        e.set_batches(_host_batches(cfg, kind, _indices(G, B, seed=2)))
        other = _results(e, G, B, sampled=False)
        assert not torch.equal(other['lp'][0], want['lp'][0])                # ... and do, on other images
        e.draw_batches(sets[kind], ix)
        _same(_results(e, G, B), want)


# ---------------------------------------------------------------------------------------------- 3. state changes
def test_draw_set_batches_draw(engines):
    cfg = 'F384_T7'
    e, sets = engines(cfg)
    ix, ix2 = _indices(3, 9), _indices(1, 5, seed=3)
    e.draw_batches(sets['r8'], ix)
    first = _results(e, 3, 9, sampled=False)
    e.set_batches(_host_batches(cfg, 'r9', ix2))
    mid = _results(e, 1, 5, sampled=False)
    e.draw_batches(sets['r9'], ix2[0])                                       # [B] form
    _same(_results(e, 1, 5, sampled=False), mid)
    e.draw_batches(sets['r8'], ix)
    _same(_results(e, 3, 9, sampled=False), first)


def test_draw_after_set_df_table_scores_against_the_new_table(engines):
    import nicnes
    cfg = 'F128_T16'
    e, sets = engines(cfg)
    fc, gts, df, n, df2 = _data(cfg)
    ix = _indices(1, 12)
    try:
        e.draw_batches(sets['r8'], ix)
        old = _results(e, 1, 12, sampled=False)
        _set_df(e, df2, n + 5)
        with pytest.raises(nicnes.NicnesError):                              # the batch is invalid, drawn or not
            e.evaluate(3, 0, 1, SIGMA)
        e.set_batches(_host_batches(cfg, 'r8', ix))
        want = _results(e, 1, 12, sampled=False)
        assert not torch.equal(want['lp'][0], old['lp'][0])
        _set_df(e, df2, n + 5)
        e.draw_batches(sets['r8'], ix)
        _same(_results(e, 1, 12, sampled=False), want)
    finally:
        _set_df(e, df, n)


@pytest.mark.parametrize('grow', ['batch', 'refs', 'images'])
def test_draw_grows_the_buffers(grow):
    """A draw beyond the handle's creation sizes, as its FIRST batch: B > max_batch; more references than max_refs;
    more images than the image capacity (= max_batch at creation)."""
    cfg = 'F384_T7'
    fc, gts, df, n, _ = _data(cfg)
    max_batch, max_refs, G, B = {'batch': (4, 1000, 1, 9), 'refs': (16, 16, 1, 16), 'images': (16, 4000, 3, 16)}[grow]
    ix = _indices(G, B)
    nr = _n_refs(cfg, 'r8', ix)
    assert (B > max_batch, nr > max_refs, G * B > max_batch) == (grow == 'batch', grow == 'refs', grow != 'refs')
    e = _engine(cfg, max_batch=max_batch, max_refs=max_refs)
    try:
        _set_df(e, df, n)
        ts = e.make_trainset(fc, gts['r8'])
        e.draw_batches(ts, ix)
        got_state, got = _state(e, nr), _results(e, G, B, sampled=False)
        e.set_batches(_host_batches(cfg, 'r8', ix))
        _same(got_state, _state(e, nr))
        _same(got, _results(e, G, B, sampled=False))
        e.draw_batches(ts, ix)                                               # and with nothing left to grow
        _same(_state(e, nr), got_state)
        _same(_results(e, G, B, sampled=False), got)
    finally:
        e.close()


def test_two_sets_on_one_handle_and_a_destroyed_set():
    import nicnes
    from nicnes import _lib
    cfg = 'F128_T16'
    fc, gts, df, n, _ = _data(cfg)
    e = _engine(cfg, max_batch=16)
    try:
        _set_df(e, df, n)
        a = e.make_trainset(fc, gts['r8'])
        fc_b, gts_b = np.ascontiguousarray(fc[::-1]), gts['r9'][::-1]        # another set: the images reversed
        b = e.make_trainset(torch.from_numpy(fc_b.copy()).to(e.device), gts_b)   # from a device tensor
        ix = _indices(1, 10)
        want = {}
        for name, f, g in (('a', fc, gts['r8']), ('b', fc_b, gts_b)):
            e.set_batch(f[ix[0]], [g[i] for i in ix[0]])
            want[name] = _results(e, 1, 10, sampled=False)
        assert not torch.equal(want['a']['lp'][0], want['b']['lp'][0])
        for name, ts in (('a', a), ('b', b), ('a', a)):
            e.draw_batches(ts, ix)
            _same(_results(e, 1, 10, sampled=False), want[name])
        stale = ctypes.c_void_p(b.ts.value)
        b.close()
        e.draw_batches(a, ix)                                                # the other set is untouched
        _same(_results(e, 1, 10, sampled=False), want['a'])
        host_ix = np.ascontiguousarray(ix)
        rc = e.L.nicnes_draw_batches(e.h, stale, host_ix.ctypes.data_as(ctypes.c_void_p), 1, 10, e._stream())
        assert rc == _lib.ERR_INVALID
        with pytest.raises(nicnes.NicnesError):
            e.draw_batches(b, ix)
        _same(_results(e, 1, 10, sampled=False), want['a'])
        a.close()
        a.close()                                                            # twice is harmless
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_leave_the_batch_held(engines):
    import nicnes
    from nicnes import _lib
    cfg = 'F128_T16'
    e, sets = engines(cfg)
    fc, gts, df, n, _ = _data(cfg)
    ix = _indices(3, 9)
    e.draw_batches(sets['r8'], ix)
    want_state, want = _state(e, _n_refs(cfg, 'r8', ix)), _results(e, 3, 9, sampled=False)

    def raw(ts, arr, G, B):
        arr = np.ascontiguousarray(arr, np.int32)
        return e.L.nicnes_draw_batches(e.h, ts, arr.ctypes.data_as(ctypes.c_void_p), G, B, e._stream())

    def still_held():
        assert e.B == 9 and e.n_batches == 3
        _same(_state(e, _n_refs(cfg, 'r8', ix)), want_state)
        _same(_results(e, 3, 9, sampled=False), want)

    ts = sets['r8'].ts
    bad = ix.copy()
    bad[2, 8] = N
    neg = ix.copy()
    neg[0, 0] = -1
    big = np.zeros(2048, np.int32)
    other = _engine(cfg, max_batch=8)
    try:
        _set_df(other, df, n)
        foreign = other.make_trainset(fc, gts['r8'])
        cases = [('index N', raw(ts, bad, 3, 9)), ('index -1', raw(ts, neg, 3, 9)), ('B 0', raw(ts, ix, 3, 0)),
                 ('B 1025', raw(ts, big, 1, 1025)), ('no batches', raw(ts, ix, 0, 9)),
                 ('too many images', raw(ts, big, (1 << 20) // 1024 + 1, 1024)),
                 ('another handle\'s set', raw(foreign.ts, ix, 3, 9)), ('no set', raw(None, ix, 3, 9)),
                 ('no indices', e.L.nicnes_draw_batches(e.h, ts, None, 3, 9, e._stream()))]
        for name, rc in cases:
            assert rc == _lib.ERR_INVALID, name
        for arr in (bad, neg):
            with pytest.raises(nicnes.NicnesError, match='image index'):
                e.draw_batches(sets['r8'], arr)
        still_held()
        # no df table: on a handle that has none (the other engine's set is its own here)
        nodf = _engine(cfg, max_batch=8)
        try:
            mine = nodf.make_trainset(fc, gts['r8'])
            with pytest.raises(nicnes.NicnesError, match='set_df_table'):
                nodf.draw_batches(mine, ix)
        finally:
            nodf.close()
        # create's own checks: a token outside the vocabulary, an image without references, ranges that do not tile
        broken = [g.copy() for g in gts['r8']]
        broken[3][0, 1] = VOCAB + 1
        with pytest.raises(nicnes.NicnesError, match='vocab'):
            e.make_trainset(fc, broken)
        with pytest.raises(nicnes.NicnesError, match='reference'):
            e.make_trainset(fc, [g if i != 4 else g[:0] for i, g in enumerate(gts['r8'])])
        still_held()
    finally:
        other.close()


# ---------------------------------------------------------------------------------------------- 5. masters
SPLITS = ['train'] * 30 + ['restval'] * 7 + ['val'] * 6 + ['test']


@pytest.fixture(scope='module')
def disk(tmp_path_factory):
    """The F128_T16 data set 'r8' as the files CocoFcDataLoader reads, plus val / test images."""
    from nicnes import data as Dt
    import nicnes.synthetic as S
    cfg = 'F128_T16'
    F, T = CFGS[cfg]
    fc, gts, df, n, _ = _data(cfg)
    root = tmp_path_factory.mktemp('coco')
    rng = np.random.Generator(np.random.PCG64(3))
    extra = len(SPLITS) - N
    all_fc = np.concatenate([fc, S.fc_feats(extra, F, 77)])
    all_gts = list(gts['r8']) + [S.substituted_refs(gts['r8'][k][0], VOCAB, rng, 5, T) for k in range(extra)]
    order = np.random.default_rng(1).permutation(len(SPLITS))                # the splits interleaved on disk
    images = [{'id': 500 + int(j), 'split': SPLITS[j], 'file_path': 'i%d.jpg' % j} for j in order]
    with open(root / 'cocotalk.json', 'w') as f:
        json.dump({'ix_to_word': {str(i): 'w%d' % i for i in range(1, VOCAB + 1)}, 'images': images}, f)
    os.makedirs(root / 'fc')
    for im, j in zip(images, order):
        np.save(root / 'fc' / ('%d.npy' % im['id']), all_fc[j])
    ncap = np.array([all_gts[j].shape[0] for j in order])
    start = np.cumsum(np.concatenate([[0], ncap[:-1]])) + 1
    Dt.LabelStore(np.concatenate([all_gts[j] for j in order]), start, start + ncap - 1).save_npz(str(root / 'labels.npz'))

    def loader(seed, batch_size=8):
        return Dt.CocoFcDataLoader(str(root / 'cocotalk.json'), str(root / 'fc'), str(root / 'labels.npz'),
                                   batch_size=batch_size, seed=seed)
    return loader, df, n


def _nes_spec(single_batch=True, G=None, schedule=False, mutation=None):
    from nicnes import config as C
    F, T = CFGS['F128_T16']
    conf = {'noise_stdev': 0.01, 'batch_size': 8, 'l2coeff': 1e-3, 'snapshot_freq': 0, 'single_batch': single_batch}
    if schedule:                                                             # the batch grows 8 -> 16 after iteration 1
        conf.update({'schedule_start': 1, 'schedule_limit': 2, 'bs_multiplier': 2, 'stdev_divisor': 2,
                     'stepsize_divisor': 2})
    mo = {'fc_feat_size': F}
    if mutation:
        mo.update({'safe_mutations': mutation, 'safe_mutation_underflow': 0.1})
    exp = {'algorithm': 'nic_nes', 'nb_offspring': P, 'config': conf,
           'policy_options': {'net': 'fc_caption', 'fitness': 'greedy', 'model_options': mo},
           'optimizer_options': {'type': 'adam', 'args': {'stepsize': 1e-3}}}
    if G:
        exp['batches_per_iteration'] = G
    return C.ExperimentSpec(exp, vocab_size=VOCAB, seq_length=T)


def _run_nes(e, spec, batches, iterations=3):
    from nicnes import master as M
    F, T = CFGS['F128_T16']
    e.set_mutation('plain')
    e.set_adam_state(np.zeros(e.D), np.zeros(e.D), 0)
    m = M.EngineMaster(spec, e, theta=_theta(F, T))
    fits, sizes, record = [], [], m._record

    def keep(fit, ratio, t0):
        fits.append(fit.clone())
        sizes.append((e.B, e.n_batches))
        return record(fit, ratio, t0)
    m._record = keep
    m.run(batches, max_iterations=iterations)
    mm, vv, t = e.adam_state()
    torch.cuda.synchronize()
    return {'theta': e.theta()[0].clone(), 'm': mm, 'v': vv, 'fit': fits}, t, sizes, m


@pytest.mark.parametrize('name', ['single_batch', 'per_member_G3', 'bs_multiplier', 'SM-PROPORTIONAL', 'SM-G-SUM'])
def test_engine_master_runs_identically_from_both_loaders(disk, name):
    from nicnes import data as Dt
    loader, df, n = disk
    spec = {'single_batch': lambda: _nes_spec(), 'per_member_G3': lambda: _nes_spec(False, 3),
            'bs_multiplier': lambda: _nes_spec(schedule=True), 'SM-PROPORTIONAL': lambda: _nes_spec(mutation=name),
            'SM-G-SUM': lambda: _nes_spec(mutation=name)}[name]()
    e = _engine('F128_T16', max_batch=8)
    try:
        _set_df(e, df, n)
        lh = loader(4)
        host, t_h, sizes_h, m_h = _run_nes(e, spec, lh)
        res = Dt.ResidentTrainLoader(loader(4), e)
        got, t_r, sizes_r, m_r = _run_nes(e, spec, res)
        assert t_h == t_r == 3 and sizes_h == sizes_r
        assert sizes_h == {'per_member_G3': [(8, 3)] * 3, 'bs_multiplier': [(8, 1), (16, 1), (16, 1)]}.get(
            name, [(8, 1)] * 3)
        _same(got, host)
        assert not torch.equal(host['fit'][0], host['fit'][1])               # the iterations saw different batches
        assert m_h.sched.to_dict() == m_r.sched.to_dict()
        assert res.loader.rng.getstate() == lh.rng.getstate()                # both loaders walked the same way
        if name.startswith('SM-'):
            assert e.mutation_mode == (2 if name == 'SM-PROPORTIONAL' else 1)
        res.close()
    finally:
        e.close()


def test_es_master_generations_are_identical(disk):
    from nicnes import data as Dt
    from nicnes.es import ESExperimentSpec, EngineESMaster
    from nicnes.validation import Validator
    import nicnes.synthetic as S
    loader, df, n = disk
    F, T = CFGS['F128_T16']
    exp = {'algorithm': 'nic_es', 'dataset': 'mscoco', 'nb_offspring': 8, 'population_size': 6, 'num_elites': 2,
           'num_elite_cands': 2, 'selection': 'tournament', 'tournament_size': 2,
           'config': {'noise_stdev': 0.01, 'batch_size': 8, 'patience': 1, 'stdev_divisor': 2.0, 'bs_multiplier': 1.0,
                      'snapshot_freq': 0, 'num_val_items': 6},
           'policy_options': {'net': 'fc_caption', 'fitness': 'greedy',
                              'model_options': {'safe_mutations': 'SM-PROPORTIONAL', 'rnn_size': 128,
                                                'input_encoding_size': 128, 'fc_feat_size': F}}}
    spec = ESExperimentSpec(exp, vocab_size=VOCAB, seq_length=T)
    start = [S.init_theta(S.Dims(VOCAB, 128, 128, F, T), 40 + i, 4.0, 0.1) for i in range(6)]
    e = _engine('F128_T16', max_batch=8)
    try:
        _set_df(e, df, n)
        val = Validator(e, loader(0), 'val', 6)
        runs = []
        for resident in (False, True):
            src = loader(9)
            if resident:
                src = Dt.ResidentTrainLoader(src, e)
            m = EngineESMaster(spec, e, validator=val, seed=3, thetas=start)
            fits = []
            for _ in range(2):
                m.step(src.get_batch('train', batch_size=8))
                fits.append(m.last['fitness'].copy())
            runs.append({'parents': [e.es_row(i).clone() for i in range(m.n_parents)],
                         'elites': [e.es_row(i, 'elites').clone() for i in range(len(m.podium.best_elites()))],
                         'podium': m.podium.best_elites(), 'cands': m.cands, 'sched': m.sched.to_dict(), 'fit': fits})
            torch.cuda.synchronize()
            e.es_free()
            if resident:
                src.close()
        a, b = runs
        assert len(a['parents']) == 6 and len(a['elites']) >= 1
        _same(b['parents'], a['parents'])
        _same(b['elites'], a['elites'])
        assert a['podium'] == b['podium'] and a['cands'] == b['cands'] and a['sched'] == b['sched']
        assert all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a['fit'], b['fit']))
        assert not np.array_equal(a['fit'][0], a['fit'][1])
        val.close()
    finally:
        e.close()
