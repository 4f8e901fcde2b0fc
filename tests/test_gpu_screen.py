"""The bf16-screened greedy decode ("bf16 screening"), on the GPU.

Chain == MFMA: a screened decode certifies a candidate's exact logit with one lane's fmaf chain instead of staging
an fp32 tile, which is only right if the chain reproduces the fp32 MFMA accumulator bit for bit. The test entry
(nicnes_test_logit_chain) lays the given rows of h out as the decode's lane scratch and computes every logit of one
member and sign both ways: by the MFMA tile path and by the very function the decode certifies with.

On against off: the fused shape forced with set_decode_split(1, 4), screening flipped with the setter on one engine;
tokens and fitness must be equal bit for bit in every case."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from oracle import oracle as O          # noqa: E402

NOISE_LEN = 1 << 23
SIGMA = 0.01


def _engine(vocab):
    import nicnes
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    e = nicnes.Engine(vocab_size=vocab, max_batch=32, max_members=4, noise_len=NOISE_LEN, noise_seed=11)
    e.set_noise_table(O.noise_table(NOISE_LEN, 123))
    return e


def _h_rows(seed):
    return np.random.Generator(np.random.PCG64(seed)).uniform(-1, 1, (32, 128)).astype(np.float32)


@pytest.mark.parametrize('vocab,gain,bias_std', [(9487, 1.0, 0.0), (9487, 4.0, 0.1), (999, 4.0, 0.1), (63, 4.0, 0.1)])
def test_fmaf_chain_equals_the_mfma_tile_bit_for_bit(vocab, gain, bias_std):
    e = _engine(vocab)
    try:
        dims = O.Dims(vocab_size=vocab)
        theta = O.make_theta(dims, 0, gain, bias_std)
        e.set_theta(theta)
        h = _h_rows(5)
        off = dims.offsets()
        (wo, ws), (bo, _) = off['logit.weight'], off['logit.bias']
        for sign in (0, 1):
            om, oc = e.test_logit_chain(7, 2, SIGMA, sign, h)
            om, oc = om.cpu().numpy(), oc.cpu().numpy()
            assert om.shape == (32, vocab + 1) and np.isfinite(om).all()
            assert np.array_equal(om.view(np.uint32), oc.view(np.uint32)), \
                '%d of %d logits differ' % ((om != oc).sum(), om.size)
            # and both are the member's logits: against fp64 on the perturbed theta, to fp32 chain rounding
            th = O.perturb(theta, e_table(), O.noise_index(11, 7, 2, NOISE_LEN, dims.D), SIGMA, +1 if sign == 0 else -1)
            W, b = th[wo: wo + ws[0] * ws[1]].reshape(ws).astype(np.float64), th[bo: bo + ws[0]].astype(np.float64)
            ref = h.astype(np.float64) @ W.T + b
            mag = np.abs(h).astype(np.float64) @ np.abs(W).T + np.abs(b)
            assert (np.abs(oc - ref) <= 129 * 2.0 ** -24 * mag).all()      # 128 fma roundings + the last
    finally:
        e.close()


_TABLE = []


def e_table():
    if not _TABLE:
        _TABLE.append(O.noise_table(NOISE_LEN, 123))
    return _TABLE[0]


def _evaluator(monkeypatch, vocab, B, P, theta, env=None, max_batch=None):
    """an engine on the fused shape with the bounded-lse decode pinned (the adaptive policy would leave the screened
    instantiation after a decode with exact passes), loaded with theta and a batch of B images"""
    import nicnes
    monkeypatch.setenv('NICNES_BOUNDED_LSE', '1')
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    e = nicnes.Engine(vocab_size=vocab, max_batch=max_batch or B, max_members=P, noise_len=NOISE_LEN, noise_seed=11)
    e.set_noise_table(e_table())
    e.set_theta(theta)
    keys, vals = nicnes.df_table_arrays({})
    e.set_df_table(keys, vals, np.log(4096.0))
    fc = np.random.Generator(np.random.PCG64(1234)).standard_normal((B, 2048)).astype(np.float32)
    gts = [np.asarray([[(7 * b + k) % min(60, vocab) + 1 for k in range(8)] + [0] * 8], np.int32) for b in range(B)]
    e.set_batch(fc, gts)
    e.set_decode_split(1, 4)
    assert e.decode_path(B, P) == 'fused'
    return e


def _on_off(e, P, sigma=SIGMA, it=5):
    """(fitness, seq) with screening off and on, and the screened run's counters"""
    out = []
    for on in (False, True):
        e.set_decode_screen(on)
        before = e.stats()
        fit, seq = e.evaluate(it, 0, P, sigma, return_seq=True)
        assert e.last_decode_bounded()
        out.append((fit.cpu().numpy(), seq.cpu().numpy()))
        after = e.stats()
    e.set_decode_screen(False)
    d = {k: after[k] - before[k] for k in after}
    ne = np.argwhere(out[0][1] != out[1][1])
    assert ne.size == 0, '%d tokens differ, first (member, sign, row, step) %s: off %s on %s' % (
        len(ne), ne[:4].tolist(), out[0][1][tuple(ne[:4].T)].tolist(), out[1][1][tuple(ne[:4].T)].tolist())
    assert np.array_equal(out[0][0], out[1][0])
    return out[1][1], d


@pytest.mark.parametrize('vocab,P,B,gain,bias_std', [
    (9487, 3, 40, 1.0, 0.0), (9487, 3, 40, 4.0, 0.1),       # rows padded to a slab, the last row group part empty
    (63, 2, 40, 1.0, 0.0), (63, 2, 40, 4.0, 0.1),           # one stage, partly valid
    (999, 2, 40, 1.0, 0.0), (999, 2, 40, 4.0, 0.1),         # last stage partly valid
    (9487, 2, 128, 1.0, 0.0), (9487, 2, 128, 4.0, 0.1)])
def test_screened_tokens_equal_the_fp32_loops(monkeypatch, vocab, P, B, gain, bias_std):
    e = _evaluator(monkeypatch, vocab, B, P, O.make_theta(O.Dims(vocab_size=vocab), 0, gain, bias_std))
    try:
        seq, d = _on_off(e, P)
        assert d['screen_candidates'] > 0                    # the screened kernel ran
        assert (seq != 0).any()
    finally:
        e.close()


def _logit_views(dims, theta):
    off = dims.offsets()
    (wo, ws), (bo, _) = off['logit.weight'], off['logit.bias']
    return theta[wo: wo + ws[0] * ws[1]].reshape(ws), theta[bo: bo + ws[0]]


def test_forced_tie_takes_the_lower_id(monkeypatch):
    dims = O.Dims()
    theta = O.make_theta(dims, 0, 4.0, 0.1).copy()
    W, b = _logit_views(dims, theta)
    lo, hi = 1234, 7001                                      # identical rows and bias, lifted to the top logit
    W[hi] = W[lo]
    b[lo] = b[hi] = 30.0
    e = _evaluator(monkeypatch, 9487, 40, 2, theta)
    try:
        seq, d = _on_off(e, 2, sigma=0.0)                    # sigma 0: the noise rows cannot split the tie
        assert (seq[:, :, :, 0] == lo).all() and not (seq == hi).any()
    finally:
        e.close()


def test_flat_logits_fall_back_to_the_exact_pass(monkeypatch):
    dims = O.Dims()
    theta = O.make_theta(dims, 0, 4.0, 0.1).copy()
    W, b = _logit_views(dims, theta)
    W[:] = W[17]
    b[:] = 0.25
    e = _evaluator(monkeypatch, 9487, 40, 2, theta)
    try:
        seq, d = _on_off(e, 2, sigma=0.0)                    # every id is a candidate
        assert d['screen_fallback_rows'] > 0
        assert (seq == 0).all()                              # the first id of the window: the end token
    finally:
        e.close()


def test_widened_eps_certifies_more_and_decodes_the_same(monkeypatch):
    theta = O.make_theta(O.Dims(), 0, 4.0, 0.1)
    res = []
    for scale in ('1', '32'):
        e = _evaluator(monkeypatch, 9487, 40, 2, theta, env={'NICNES_SCREEN_EPS_SCALE': scale})
        try:
            res.append(_on_off(e, 2))
        finally:
            e.close()
    assert np.array_equal(res[0][0], res[1][0])
    assert res[1][1]['screen_candidates'] > res[0][1]['screen_candidates']


def test_non_finite_theta_decodes_the_same(monkeypatch):
    dims = O.Dims()
    theta = O.make_theta(dims, 0, 4.0, 0.1).copy()
    W, b = _logit_views(dims, theta)
    W[4321, 5] = np.inf
    W[77, 100] = np.nan
    e = _evaluator(monkeypatch, 9487, 40, 2, theta)
    try:
        _on_off(e, 2)
    finally:
        e.close()
