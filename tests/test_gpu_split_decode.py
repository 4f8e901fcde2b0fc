"""GPU: nicnes_split_decode, the one-call greedy decode of theta on a resident evaluation split (the decode of
eval_split, src/captioning/eval_utils.py:110-180). Its rows must be, bit for bit, the rows
nicnes_evaluate_theta gives for the same images as batches of 128 / 128 / 44, for every range and on every
decode shape; the log-probs agree to the 2.5e-7 relative of tests/test_gpu_eval_theta.py (compared up to and
including each row's end token, where both are defined: nicnes.h); the tokens equal the oracle's on the rows it does
not flag fragile. The split calls leave the training batch, df table, fitness mode, mutation and rows-per-image state
untouched (a following evaluate gives the same fitness bits), and need no noise table."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from oracle import oracle as O          # noqa: E402

NOISE_LEN = 1 << 23
N = 300
FC_SEED = 500        # the oracle flags no row of these images fragile (checked on the CPU with O.decode)
RANGES = [(0, 1), (0, 127), (0, 128), (0, 129), (1, 256), (43, 257), (0, 300)]
PATHS = {'auto': (0, 0, 1), 'fused': (1, 4, 1), 'fused64': (1, 2, 1), 'coop': (4, 4, 1), 'split': (4, 4, 0)}


def _fc(n, F, seed):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((n, F)).astype(np.float32)


def _placeholder(n):
    return [np.asarray([[1, 2, 3, 0] + [0] * 12], np.int32) for _ in range(n)]


def _lp_masked(seq, lp):
    """log-probs up to and including each row's end token; 0 after it"""
    ended = np.cumsum(seq == 0, 1) - (seq == 0) > 0
    return np.where(ended, np.float32(0), lp)


@pytest.fixture(scope='module')
def work():
    """engine + the 300-image split + evaluate_theta's rows of the same images (batches 128 / 128 / 44)"""
    import nicnes
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    dims = O.Dims()
    theta = O.make_theta(dims, 2, 4.0, 0.1)
    fc = _fc(N, dims.F, FC_SEED)
    e = nicnes.Engine(max_batch=128, max_members=4, noise_len=NOISE_LEN, noise_seed=7)
    e.set_noise_table(O.noise_table(NOISE_LEN, 123))
    e.set_theta(theta)
    e.set_df_table(np.zeros(0, np.uint64), np.zeros(0), np.log(64.0))
    refs = {}

    def reference(path):
        """evaluate_theta's rows under the decode shape forced for `path` (set by the caller), computed once"""
        if path not in refs:
            seqs, lps = [], []
            for a in range(0, N, 128):
                b = min(N, a + 128)
                e.set_batch(fc[a:b], _placeholder(b - a))
                _, s, lp = e.evaluate_theta(0, return_seq=True, return_lp=True)
                seqs.append(s.cpu().numpy())
                lps.append(lp.cpu().numpy())
            refs[path] = np.concatenate(seqs), np.concatenate(lps)
        return refs[path]
    split = e.make_split(fc)
    yield e, split, dims, theta, fc, reference
    split.close()
    e.close()


@pytest.mark.parametrize('path', list(PATHS))
def test_split_decode_equals_evaluate_theta(work, path):
    e, split, dims, theta, fc, reference = work
    S, G, coop = PATHS[path]
    try:
        e.set_decode_split(S, G)
        e.set_decode_coop(coop)
        # the same forced shape on both sides, as tests/test_gpu_eval_theta.py compares: the log-prob bound covers the
        # split's other slab filling, not another vocabulary split (the tokens are the same bits on every shape)
        ref_seq, ref_lp = reference(path)
        assert np.array_equal(ref_seq, reference('auto')[0])
        for first, count in RANGES:
            seq, lp = split.decode(first, count, return_lp=True)
            seq2 = split.decode(first, count)
            seq, lp, seq2 = seq.cpu().numpy(), lp.cpu().numpy(), seq2.cpu().numpy()
            want = ref_seq[first:first + count]
            assert seq.shape == (count, 16)
            assert np.array_equal(seq, want), (path, first, count)
            assert np.array_equal(seq2, want), (path, first, count)      # the greedy-only decode (bounded lse, screen)
            np.testing.assert_allclose(lp, _lp_masked(want, ref_lp[first:first + count]), rtol=2.5e-7, atol=0)
    finally:
        e.set_decode_split(0, 0)
        e.set_decode_coop(1)


def test_split_decode_equals_the_oracle(work):
    e, split, dims, theta, fc, _ = work
    oseq, olp, fragile = O.decode(dims, theta, fc)
    keep = ~np.asarray(fragile).reshape(N, -1).any(1)
    assert keep.sum() >= 0.95 * N, keep.sum()
    seq = split.decode().cpu().numpy()
    assert np.array_equal(seq[keep], oseq[keep])


def test_split_decode_small_vocabulary_tail_and_beyond_max_members():
    """V = 1023, N = 641: three pseudo-members (more than max_members = 2), an odd slab count with a 1-row tail;
    against evaluate_theta on batches of 128"""
    import nicnes
    dims = O.Dims(vocab_size=1023)
    theta = O.make_theta(dims, 5, 4.0, 0.1)
    n = 641
    fc = _fc(n, dims.F, 77)
    e = nicnes.Engine(vocab_size=1023, max_batch=128, max_members=2, noise_len=NOISE_LEN, noise_seed=7)
    try:
        e.set_noise_table(O.noise_table(NOISE_LEN, 123))
        e.set_theta(theta)
        e.set_df_table(np.zeros(0, np.uint64), np.zeros(0), np.log(64.0))
        rows = []
        for a in range(0, n, 128):
            b = min(n, a + 128)
            e.set_batch(fc[a:b], _placeholder(b - a))
            rows.append(e.evaluate_theta(0, return_seq=True)[1].cpu().numpy())
        want = np.concatenate(rows)
        split = e.make_split(fc)
        for path in ('auto', 'fused', 'split'):
            S, G, coop = PATHS[path]
            e.set_decode_split(S, G)
            e.set_decode_coop(coop)
            assert np.array_equal(split.decode().cpu().numpy(), want), path
            assert np.array_equal(split.decode(640, 1).cpu().numpy(), want[640:]), path
            assert np.array_equal(split.decode(129, 512).cpu().numpy(), want[129:641]), path
        with pytest.raises(ValueError):
            split.decode(0, 642)
        out = torch.empty((641, 16), dtype=torch.int32, device=e.device)
        for first, count in ((1, 641), (-1, 2), (0, 0)):            # the C ABI checks the range itself
            rc = e.L.nicnes_split_decode(e.h, split.sp, first, count, out.data_ptr(), None, None)
            assert rc == 1, (first, count, rc)                      # NICNES_ERR_INVALID
    finally:
        e.close()


def test_split_decode_of_captions_that_end_early():
    """V = 1023 with the end token's logit bias raised by 2: the oracle's captions of these images end after 0..16
    words, so rows finish at different steps, workgroups exit early, and the log-probs after a row's end token are 0.
    Tokens against evaluate_theta and the oracle, log-probs against evaluate_theta's up to each row's end token."""
    import nicnes
    dims = O.Dims(vocab_size=1023)
    theta = O.make_theta(dims, 5, 4.0, 0.1)
    theta[dims.offsets()['logit.bias'][0]] += np.float32(2.0)
    n = 300
    fc = _fc(641, dims.F, 77)[:n]
    oseq, _, fragile = O.decode(dims, theta, fc)
    lengths = np.array([(list(r) + [0]).index(0) for r in oseq])
    assert len(set(lengths)) == 17 and not np.asarray(fragile).any()        # every length 0..16 occurs
    e = nicnes.Engine(vocab_size=1023, max_batch=128, max_members=2, noise_len=NOISE_LEN, noise_seed=7)
    try:
        e.set_noise_table(O.noise_table(NOISE_LEN, 123))
        e.set_theta(theta)
        e.set_df_table(np.zeros(0, np.uint64), np.zeros(0), np.log(64.0))
        split = e.make_split(fc)
        for path in ('auto', 'fused', 'fused64', 'coop', 'split'):
            S, G, coop = PATHS[path]
            e.set_decode_split(S, G)
            e.set_decode_coop(coop)
            seqs, lps = [], []
            for a in range(0, n, 128):
                b = min(n, a + 128)
                e.set_batch(fc[a:b], _placeholder(b - a))
                _, s, lp = e.evaluate_theta(0, return_seq=True, return_lp=True)
                seqs.append(s.cpu().numpy())
                lps.append(lp.cpu().numpy())
            want, want_lp = np.concatenate(seqs), np.concatenate(lps)
            assert np.array_equal(want, oseq), path
            for first, count in ((0, n), (43, 257), (129, 1)):
                seq, lp = split.decode(first, count, return_lp=True)
                seq, lp = seq.cpu().numpy(), lp.cpu().numpy()
                assert np.array_equal(seq, want[first:first + count]), (path, first, count)
                assert np.array_equal(split.decode(first, count).cpu().numpy(), seq), (path, first, count)
                np.testing.assert_allclose(lp, _lp_masked(seq, want_lp[first:first + count]), rtol=2.5e-7, atol=0)
                ended = np.cumsum(seq == 0, 1) - (seq == 0) > 0
                assert (lp[ended] == 0).all() and (lp[~ended] < 0).all()
    finally:
        e.close()


def test_split_calls_leave_the_training_state_alone():
    """batch, df table, greedy_linprob, a scale mutation and rows_per_image = 5 set before: the evaluate after the
    split calls returns the fitness bits of the evaluate before them"""
    import nicnes
    import nicnes.synthetic as S
    dims = O.Dims()
    theta = O.make_theta(dims, 2, 4.0, 0.1)
    fc = _fc(40, dims.F, 9)
    base, _, _ = O.decode(dims, theta, fc)
    gts, df, n = S.build_references(base, dims.vocab_size, seed=10, df_sets=64)
    e = nicnes.Engine(max_batch=64, max_members=4, noise_len=NOISE_LEN, noise_seed=7)
    try:
        e.set_noise_table(O.noise_table(NOISE_LEN, 123))
        e.set_theta(theta)
        keys, vals = nicnes.df_table_arrays(df)
        e.set_df_table(keys, vals, np.log(float(n)))
        e.set_batch(fc, gts)
        e.set_fitness_mode('greedy_linprob')
        e.set_mutation('scale', np.abs(theta) + np.float32(0.5))
        e.set_rows_per_image(5)
        before = e.evaluate(3, 0, 4, 0.01).cpu().numpy()
        split = e.make_split(_fc(300, dims.F, 11), [g[:3] for g in gts] * 7 + [g[:3] for g in gts[:20]])
        seq = split.decode()
        split.score(seq)
        split.evaluate()
        after = e.evaluate(3, 0, 4, 0.01).cpu().numpy()
        assert np.array_equal(before.view(np.uint64), after.view(np.uint64)), (before, after)
        split.close()
        after2 = e.evaluate(3, 0, 4, 0.01).cpu().numpy()
        assert np.array_equal(before.view(np.uint64), after2.view(np.uint64))
    finally:
        e.close()


def test_split_decode_needs_no_noise_table():
    import nicnes
    dims = O.Dims(vocab_size=1023)
    theta = O.make_theta(dims, 5, 4.0, 0.1)
    fc = _fc(33, dims.F, 3)
    e = nicnes.Engine(vocab_size=1023, max_batch=64, max_members=2, noise_len=NOISE_LEN, noise_seed=7)
    try:
        e.set_theta(theta)
        split = e.make_split(fc)
        seq = split.decode().cpu().numpy()
        oseq, _, fragile = O.decode(dims, theta, fc)
        keep = ~np.asarray(fragile).reshape(33, -1).any(1)
        assert keep.sum() >= 30
        assert np.array_equal(seq[keep], oseq[keep])
        with pytest.raises(nicnes.NicnesError):                     # a decode-only split has nothing to score against
            split.evaluate()
    finally:
        e.close()
