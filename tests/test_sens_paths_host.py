"""Guards of tests/test_gpu_sens_paths.py's worlds (tests/sens_worlds.py), on the CPU: each world is what DESIGN.md
section 8's table says of it (alignment, K, the split of the vocabulary), its oracle tokens exercise the embedding
kernels (runs of several chunks, rows no token feeds), and the oracle's own summation-order noise is a small fraction
of the bar the GPU vector is held to. No GPU."""
import numpy as np
import pytest

from tests import sens_worlds as W
from tests.test_gpu_mutations import SENS_RTOL, _sens_close

NOISE_SHARE = 0.1      # of the bar: a condition on the inputs (the reference is sharp enough there), not a kernel tolerance


def _nsp(V):
    """nicnes_sens_run's split of p Wl over the vocabulary (TR_MIN = 32)"""
    for d in range(32, 1, -1):
        if V % d == 0 and V // d >= 32:
            return d
    return 1


@pytest.mark.parametrize('vocab', sorted(W.VOCAB_FACTS) + sorted(W.REFUSED_VOCABS))
def test_vocabulary_is_what_the_table_says(vocab):
    d = W.dims_of(vocab)
    offs = d.offsets()
    nsp = _nsp(d.V1)
    got = (d.V1 % 4, d.V1 // W.SPLIT + 1, nsp, d.V1 // nsp, offs['core.i2h.weight'][0] % 4, offs['core.h2h.weight'][0] % 4)
    assert got == (W.VOCAB_FACTS.get(vocab) or W.REFUSED_VOCABS[vocab])
    assert [name for name, _ in d.shapes()] == list(W.SEGMENTS)
    assert d.E == 128 and d.R == 128 and d.F == W.F


def test_expected_paths_follow_the_dispatcher_rules():
    """the table's expected bits, from the rules of nicnes_sens_run restated: rows <= 128, aligned i2h / h2h, K <= 96"""
    for name, (vocab, _, rows, want) in W.SHAPE_CASES.items():
        v1m4, K, _, _, oi, oh = W.VOCAB_FACTS[vocab]
        assert v1m4 == 0, name
        rule = dict(logit_fast=rows <= 128, bwd_fused=oi == 0 and oh == 0, gates_bsq=(K + 31) // 32 <= 3,
                    emb_two_pass=K <= 96)
        assert want == rule, name
        assert rows <= W.MAX_ROWS
    assert W.MAX_ROWS == 819 and W.L * W.MAX_ROWS == 4095            # npair of rows_max
    # the last group: all padding at 999 (its seed is zero), 28 words at 1027 (test_all_switches_at_once)
    assert W.dims_of(999).V1 % W.SPLIT == 0 and W.dims_of(1027).V1 % W.SPLIT == 28
    cleared = {tuple(sorted(k for k, v in c[3].items() if not v)) for c in W.SHAPE_CASES.values()}
    assert cleared == {(), ('logit_fast',), ('emb_two_pass', 'gates_bsq')}       # what a shape alone can clear
    for name, (vocab, _, rows, switches, want) in W.FORCED_CASES.items():
        assert set(switches) == {'bwd', 'scalar'} and vocab in W.VOCAB_FACTS
        assert want == W.paths(bwd_fused=False, logit_fast=rows <= 128), name


@pytest.mark.parametrize('vocab', sorted(W.REFUSED_VOCABS))
def test_no_handle_has_a_misaligned_theta(vocab):
    """A V1 that is no multiple of 4 would put core.i2h.weight and core.h2h.weight off 16-byte alignment (the backward
    bit cleared, scalar loads in every V-strided product, by shape alone): nicnes_create refuses it before touching
    the GPU, so those fallbacks are reached through NICNES_SENS_TILE_BWD / NICNES_SENS_TILE_SCALAR only
    (sens_worlds.FORCED_CASES). If the handle ever accepts such a vocabulary, it belongs in SHAPE_CASES."""
    import ctypes
    from nicnes import _lib
    v1m4, _, _, _, oi, oh = W.REFUSED_VOCABS[vocab]
    assert v1m4 != 0 and oi != 0 and oh != 0
    cfg = _lib.NicnesConfig(vocab, 128, 128, W.F, 16, 16, 8, 2, 1 << 23, 0)
    h = ctypes.c_void_p()
    assert _lib.lib().nicnes_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == _lib.ERR_UNSUPPORTED


def _long_runs_at_least(rows):
    """The oracle's runs of more than EMB_CH pairs beside BOS's (runs of one chunk only would leave sens_emb_part's
    chunk search and sens_emb_fin's sum over chunks to the BOS run alone): at least two from 128 rows on (counted: 2 to
    40), at least one at 33 .. 65 rows, where these thetas repeat one token only beyond 16 pairs."""
    return 2 if rows >= 128 else 1


@pytest.mark.parametrize('world', W.all_worlds(), ids=lambda w: '%s_%s_%s' % w)
def test_tokens_exercise_the_embedding_kernels(world):
    vocab, kind, rows = world
    d = W.dims_of(vocab)
    tok = W.oracle_tokens(vocab, kind, rows)
    assert tok.shape == (rows, W.L) and (tok[:, 0] == 0).all() and tok.min() >= 0 and tok.max() < d.V1
    ids, counts = np.unique(tok, return_counts=True)
    assert counts[ids == 0][0] >= rows                                # the BOS run
    if rows > W.EMB_CH:
        assert -(-int(counts[ids == 0][0]) // W.EMB_CH) >= 2          # ... of several chunks
    if rows >= 33:
        long_runs = int(((counts > W.EMB_CH) & (ids != 0)).sum())
        assert long_runs >= _long_runs_at_least(rows), long_runs
    # rows no token feeds: exact zeros in the vector (sens_zero_rows, in every partial row the segment sums)
    ref = W.reference(vocab, kind, rows)
    (o, n), = [(o, n) for name, o, n in W.segments(vocab) if name == 'embed.weight']
    emb = ref[o:o + n].reshape(d.V1, d.E)
    unfed = np.setdiff1d(np.arange(d.V1), ids)
    assert unfed.size >= d.V1 // 2 and not emb[unfed].any()
    assert all(emb[t].any() for t in ids)
    assert np.isfinite(ref).all() and ref.max() > 0


@pytest.mark.parametrize('world', [w for w in W.all_worlds() if w[2] >= 2], ids=lambda w: '%s_%s_%s' % w)
def test_reference_noise_is_a_small_share_of_the_bar(world):
    """The oracle on the rows in another order is the same sum mathematically; what differs is its own fp32
    summation-order noise, here as a share of the bar (measured 0.004 .. 0.021 over these worlds)."""
    vocab, kind, rows = world
    perm = np.random.Generator(np.random.PCG64(5)).permutation(rows)
    assert not np.array_equal(perm, np.arange(rows))
    ref, permuted = W.reference(vocab, kind, rows), W.reference(vocab, kind, rows, perm)
    ratios = W.segment_ratios(permuted, ref, vocab)
    print(world, {k: round(v, 4) for k, v in ratios.items()})
    assert max(ratios.values()) <= NOISE_SHARE, ratios
    assert _sens_close(permuted, ref)[0]


def test_segment_ratios_is_the_project_bar():
    """segment_ratios <= 1 everywhere exactly when tests/test_gpu_mutations.py's _sens_close holds"""
    vocab, kind, rows = 999, 'wc', 12
    ref = W.reference(vocab, kind, rows)
    segs = W.segments(vocab)
    assert segs[0][1] == 0 and segs[-1][1] + segs[-1][2] == ref.size
    assert all(a[1] + a[2] == b[1] for a, b in zip(segs, segs[1:]))
    for name, o, n in segs:
        for scale, ok_want in ((0.9, True), (1.1, False)):
            got = ref.astype(np.float64).copy()
            j = o + int(np.argmax(ref[o:o + n]))
            got[j] += scale * (SENS_RTOL * abs(float(ref[j])) + 1e-6 * float(ref.max()))
            ratios = W.segment_ratios(got, ref, vocab)
            assert (max(ratios.values()) <= 1.0) == ok_want == _sens_close(got, ref)[0], (name, scale)
            assert max(ratios, key=ratios.get) == name
