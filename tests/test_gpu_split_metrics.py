"""GPU: the validation scorer (nicnes_split_score / nicnes_split_evaluate): COCOEvalCap's BLEU-1..4, ROUGE_L and
CIDEr (src/captioning/eval_utils.py:60-107) on token rows, captions being the tokens before the
first 0. Chosen rows with closed-form answers, random rows against the restatement of tests/coco_metrics_ref.py and
the CIDEr-D oracle (the ten BLEU totals exactly, the metrics and per-row CIDEr-D to 1e-9 relative, the same bits on
two runs), evaluate = score(decode), and NaN metrics on a handle with a contained decode fault."""
import math

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from oracle import oracle as O                      # noqa: E402
from tests import coco_metrics_ref as M             # noqa: E402

TOL = 1e-9          # relative; tests/test_gpu_cider.py's scorer bound
NOISE_LEN = 1 << 23
T = 16
KEYS = ('Bleu_1', 'Bleu_2', 'Bleu_3', 'Bleu_4', 'ROUGE_L', 'CIDEr')


def row(*w):
    return list(w) + [0] * (T - len(w))


def rows(*caps):
    return np.asarray([row(*c) for c in caps], np.int32)


def rel_close(got, ref):
    return abs(got - ref) <= TOL * abs(ref)


# (name, references, hypothesis)
CASES = [
    ('identical', [(5, 6, 7, 8, 9)], (5, 6, 7, 8, 9)),
    ('disjoint', [(10, 11, 12, 13)], (20, 21, 22, 23)),
    ('empty', [(14, 15, 16)], ()),
    ('one_word', [(30, 31, 32)], (30,)),
    ('brevity', [(40, 41, 42, 43, 44, 45)], (40, 41, 42, 43)),
    ('reflen_tie', [(80, 81, 82, 83, 84, 85), (80, 81, 86, 87)], (80, 81, 82, 88, 89)),
    ('clipped', [(50, 51, 52, 53), (50, 50, 54, 55)], (50, 50, 50, 50)),
    ('lcs', [(60, 70, 62, 71, 63)], (60, 61, 62, 63)),
    ('nine_refs', [(90 + k, 91, 92, 93 + k, 94) for k in range(9)], (98, 91, 92, 93, 94, 95)),
    ('wide_ids', [(1, 8192, 16383, 8192, 1), (16383, 1, 2)], (1, 8192, 16383, 8192, 1)),
]


@pytest.fixture(scope='module')
def eng():
    import nicnes
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    e = nicnes.Engine(vocab_size=16383, max_batch=64, max_members=2, noise_len=NOISE_LEN, noise_seed=7)
    yield e
    e.close()


@pytest.fixture(scope='module')
def chosen(eng):
    gts = [rows(*refs) for _, refs, _ in CASES]
    seq = rows(*[h for _, _, h in CASES])
    split = eng.make_split(np.zeros((len(CASES), 2048), np.float32), gts)
    yield split, gts, seq, {name: i for i, (name, _, _) in enumerate(CASES)}
    split.close()


def one(split, seq, i):
    m, tot, cider = split.score(seq[i:i + 1], first=i, detail=True)
    return m, [int(t) for t in tot], float(cider[0])


def test_closed_forms(chosen):
    split, gts, seq, ix = chosen
    m, tot, c = one(split, seq, ix['identical'])
    assert all(abs(m['Bleu_%d' % k] - 1.0) <= 1e-9 for k in range(1, 5)), m
    assert m['ROUGE_L'] == 1.0 and abs(m['CIDEr'] - 10.0) <= 1e-9 and abs(c - 10.0) <= 1e-9, (m, c)
    assert tot == [5, 4, 3, 2, 5, 4, 3, 2, 5, 5]

    m, tot, c = one(split, seq, ix['disjoint'])
    assert all(abs(m[k]) <= 1e-9 for k in KEYS) and c == 0.0, m
    assert tot == [0, 0, 0, 0, 4, 3, 2, 1, 4, 4]

    m, tot, c = one(split, seq, ix['empty'])
    assert tot == [0, 0, 0, 0, 0, 0, 0, 0, 0, 3]
    assert all(math.isfinite(m[k]) and abs(m[k]) <= 1e-9 for k in KEYS) and c == 0.0, m

    m, tot, c = one(split, seq, ix['one_word'])
    assert tot == [1, 0, 0, 0, 1, 0, 0, 0, 1, 3]

    m, tot, c = one(split, seq, ix['brevity'])
    assert tot == [4, 3, 2, 1, 4, 3, 2, 1, 4, 6]
    assert all(abs(m['Bleu_%d' % k] - math.exp(1 - 6 / 4)) <= 1e-8 for k in range(1, 5)), m

    m, tot, c = one(split, seq, ix['reflen_tie'])
    assert tot[8:] == [5, 4]                                    # |6 - 5| == |4 - 5|: the shorter

    m, tot, c = one(split, seq, ix['clipped'])
    assert tot[:4] == [2, 1, 0, 0]                              # min(4, max(1, 2)), min(3, max(0, 1))

    m, tot, c = one(split, seq, ix['lcs'])
    p, r, b2 = 3 / 4, 3 / 5, 1.2 ** 2
    assert rel_close(m['ROUGE_L'], (1 + b2) * p * r / (r + b2 * p)), m

    m, tot, c = one(split, seq, ix['wide_ids'])
    assert all(abs(m['Bleu_%d' % k] - 1.0) <= 1e-9 for k in range(1, 5)) and m['ROUGE_L'] == 1.0, m


def test_chosen_rows_against_the_restatement(chosen):
    split, gts, seq, ix = chosen
    scorer = M.corpus_scorer(gts)
    for i, (name, _, _) in enumerate(CASES):                    # each image alone (nine_refs: beyond the image tables)
        m, tot, c = one(split, seq, i)
        rt, rm, rc = M.corpus_metrics(seq[i:i + 1], gts[i:i + 1], scorer)
        assert tot == [int(t) for t in rt], name
        assert all(rel_close(m[k], rm[k]) for k in KEYS), (name, m, rm)
        assert rel_close(c, rc[0]), (name, c, rc[0])
    m, tot, cider = split.score(seq, detail=True)               # and the corpus of them
    rt, rm, rc = M.corpus_metrics(seq, gts, scorer)
    assert [int(t) for t in tot] == [int(t) for t in rt]
    assert all(rel_close(m[k], rm[k]) for k in KEYS), (m, rm)
    assert all(rel_close(a, b) for a, b in zip(cider, rc))


def _random_rows(rng, n_img=64, vocab=40):
    gts, seq = [], []
    for _ in range(n_img):
        refs = []
        for _ in range(int(rng.integers(1, 8))):
            L = int(rng.integers(0, T + 1))
            refs.append(row(*[int(t) for t in rng.integers(1, vocab + 1, L)]))
        if not any(r[0] for r in refs):
            refs[0] = row(int(rng.integers(1, vocab + 1)))
        g = np.asarray(refs, np.int32)
        L = int(rng.integers(0, T + 1))
        if rng.random() < 0.5:                                   # shares n-grams with a reference: a perturbed copy
            src = M.words(g[int(rng.integers(0, len(g)))])
            h = [(t if rng.random() < 0.7 else int(rng.integers(1, vocab + 1))) for t in src][:L]
        else:
            h = [int(t) for t in rng.integers(vocab + 1, 2 * vocab, L)]
        gts.append(g)
        seq.append(row(*h))
    return gts, np.asarray(seq, np.int32)


def test_random_rows_against_the_restatement(eng):
    rng = np.random.Generator(np.random.PCG64(2024))
    gts, seq = _random_rows(rng)
    split = eng.make_split(np.zeros((64, 2048), np.float32), gts)
    try:
        m, tot, cider = split.score(seq, detail=True)
        m2, tot2, cider2 = split.score(seq, detail=True)
        rt, rm, rc = M.corpus_metrics(seq, gts)
        print('totals', list(tot), list(rt))
        print('metrics', m, rm)
        assert [int(t) for t in tot] == [int(t) for t in rt]
        assert all(rel_close(m[k], rm[k]) for k in KEYS), (m, rm)
        bad = [(i, a, b) for i, (a, b) in enumerate(zip(cider, rc)) if not rel_close(a, b)]
        assert not bad, bad[:8]
        assert np.array_equal(tot, tot2) and np.array_equal(cider.view(np.uint64), cider2.view(np.uint64))
        assert [np.float64(m[k]).view(np.uint64) for k in KEYS] == [np.float64(m2[k]).view(np.uint64) for k in KEYS]
        # a range inside the split scores against that range's references
        m3, tot3, cider3 = split.score(seq[10:30], first=10, detail=True)
        assert np.array_equal(cider3.view(np.uint64), cider[10:30].view(np.uint64))
        assert [int(t) for t in tot3] == [int(t) for t in M.corpus_metrics(seq[10:30], gts[10:30])[0]]
    finally:
        split.close()


def test_token_range_checks(eng):
    """as set_batches: an id outside [0, vocab_size] would alias another word in the 14-bit key fields"""
    fc = np.zeros((2, 2048), np.float32)
    for bad in (16384, -1):
        with pytest.raises(ValueError):
            eng.make_split(fc, [rows((1, 2, 3)), rows((4, bad, 5))])
    split = eng.make_split(fc, [rows((1, 2, 3)), rows((4, 5, 6))])
    try:
        for bad in (16384, -1):
            with pytest.raises(ValueError):
                split.score(rows((1, 2), (bad, 3)))
        with pytest.raises(ValueError):
            split.score(rows((1, 2), (2, 3), (3, 4)))               # more rows than images
        with pytest.raises(ValueError):
            eng.make_split(fc, [rows((1, 2, 3))])                   # one image's references missing
    finally:
        split.close()


def _decoding_engine(max_members=8):
    import nicnes
    e = nicnes.Engine(max_batch=128, max_members=max_members, noise_len=NOISE_LEN, noise_seed=11)
    e.set_noise_table(O.noise_table(NOISE_LEN, 123))
    e.set_theta(O.make_theta(O.Dims(), 3, 4.0, 0.1))
    return e


def _split_of(e, n, seed=3):
    fc = np.random.Generator(np.random.PCG64(seed)).standard_normal((n, 2048)).astype(np.float32)
    gts = [np.asarray([row(*[(7 * b + k) % 60 + 1 for k in range(8)]), row(*[(5 * b + k) % 60 + 1 for k in range(6)])],
                      np.int32) for b in range(n)]
    return e.make_split(fc, gts), fc, gts


def test_evaluate_is_score_of_decode():
    e = _decoding_engine()
    try:
        split, _, _ = _split_of(e, 300)
        for first, count in ((0, None), (43, 130)):
            m, tot, cider = split.evaluate(first, count, detail=True)
            seq = split.decode(first, count)
            m2, tot2, cider2 = split.score(seq, first=first, detail=True)
            assert np.array_equal(tot, tot2) and np.array_equal(cider.view(np.uint64), cider2.view(np.uint64))
            assert all(np.float64(m[k]).view(np.uint64) == np.float64(m2[k]).view(np.uint64) for k in KEYS), (m, m2)
            (m3, seq3) = split.evaluate(first, count, return_seq=True)
            assert torch.equal(seq3, seq) and m3 == m
    finally:
        e.close()


def test_metrics_are_nan_on_a_faulted_handle(monkeypatch):
    """the coop stall hook of tests/test_gpu_faults.py, as it is: the training decode loses rows, the handle's fault
    is sticky, and the validation metrics of that handle are NaN like its fitness"""
    monkeypatch.setenv('NICNES_TEST_COOP_STALL', '700')      # past the 0.5 s spin bound
    monkeypatch.setenv('NICNES_TEST_COOP_STALL_LAUNCHES', '1')
    import nicnes
    e = _decoding_engine()
    try:
        split, fc, gts = _split_of(e, 128)
        good = split.evaluate()
        assert all(math.isfinite(good[k]) for k in KEYS), good
        keys, vals = nicnes.df_table_arrays({})
        e.set_df_table(keys, vals, np.log(4096.0))
        e.set_batch(fc, gts)
        e.set_decode_split(4, 4)
        assert e.decode_path(128, 4) == 'coop'
        fit = e.evaluate(1, 0, 4, 0.01)
        torch.cuda.synchronize()
        assert e.stats()['coop_timeouts'] > 0 and torch.isnan(fit).all()
        bad, tot, _ = split.evaluate(detail=True)
        assert all(math.isnan(bad[k]) for k in KEYS), bad
        e.clear_faults()
        again = split.evaluate()
        assert again == good, (again, good)
    finally:
        e.close()
