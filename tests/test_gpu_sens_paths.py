"""The SM-G-SUM sensitivity (nicnes_sum_sensitivity, csrc/sensitivity.hip) on every path nicnes_sens_run's dispatcher
can take: each fast kernel and its general fallback, reached by shape (rows above 128, a
vocabulary whose V1 is no multiple of 4 so that the i2h / h2h weights lose their 16-byte alignment, K above 96) and by
the NICNES_SENS_* switches, with Engine.sens_paths() confirming where the run went. Every vector is held to
tests/test_gpu_mutations.py's bar against oracle/sensitivity_ref.py, segment by segment (the print names the kernel
behind a miss); a switch must leave the segments it cannot feed bit-identical; the work buffers and the partial rows,
which persist between calls, must not leak from one path or batch size into the next. The worlds and their CPU guards:
tests/sens_worlds.py, tests/test_sens_paths_host.py."""
import contextlib

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from oracle import oracle as O                                   # noqa: E402
from tests import sens_worlds as W                               # noqa: E402
from tests.test_gpu_mutations import _sens_close                 # noqa: E402  (the project's bar, not a copy)

NOISE_LEN = 1 << 23
UNDERFLOW = 1e-3
_cache = {}


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)
    return a.view(np.uint32)


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    """every test starts with no NICNES_SENS_* switch set (env_on reads the environment on every run)"""
    for name in W.SWITCHES.values():
        monkeypatch.delenv(name, raising=False)


@contextlib.contextmanager
def _handle(vocab, kind, max_batch, es_parents=None):
    """a handle at F = 128 holding the first max_batch fc rows, theta = the world's (or parent 0 of es_parents)"""
    import nicnes
    if 'table' not in _cache:
        _cache['table'] = O.noise_table(NOISE_LEN, 123)
    d = W.dims_of(vocab)
    e = nicnes.Engine(vocab_size=vocab, fc_feat_size=W.F, max_batch=max_batch, max_members=2, noise_len=NOISE_LEN,
                      noise_seed=0)
    try:
        e.set_noise_table(_cache['table'])
        e.set_df_table(np.zeros(0, np.uint64), np.zeros(0), np.log(64.0))
        e.set_batch(W.fc_rows(max_batch), [np.zeros((1, d.T), np.int32)] * max_batch)
        if es_parents is None:
            e.set_theta(W.theta_of(vocab, kind))
        else:
            e.es_create(len(es_parents) + 1, 1)
            e.es_set_parents([W.theta_of(vocab, s) for s in es_parents])
            e.es_set_mutation_divide()
        yield e
    finally:
        e.close()


def _bits_of(p):
    return {k: p[k] for k in W.ALL_FAST}


def _check(e, vocab, kind, rows, want, label):
    """One world on handle e: the paths taken, the raw vector against the oracle segment by segment, the same bits
    and paths on a second call, the clamped vector = clamp_calc of the raw one bit for bit. Returns (raw, paths)."""
    from nicnes import mutations as MU
    raw = e.sum_sensitivity(rows).cpu().numpy()
    p = e.sens_paths()
    assert _bits_of(p) == want, (label, p)
    assert p['gemm_v4'] + p['gemm_scalar'] > 0
    again = e.sum_sensitivity(rows).cpu().numpy()
    assert np.array_equal(_bits(again), _bits(raw)), label
    assert e.sens_paths() == p, label
    clamped = e.sum_sensitivity(rows, UNDERFLOW).cpu().numpy()
    assert np.array_equal(_bits(clamped), _bits(MU.clamp_calc(torch.from_numpy(raw), UNDERFLOW).numpy())), label
    assert e.sens_paths() == p, label
    ref = W.reference(vocab, kind, rows)
    ratios = W.segment_ratios(raw, ref, vocab)
    print('%s: vocab %d rows %d %s worst error / bound per segment: %s' % (
        label, vocab, rows, {k: v for k, v in p.items() if not v or k.startswith('gemm')},
        ' '.join('%s %.3f' % (k, v) for k, v in ratios.items())))
    assert np.isfinite(raw).all()
    over = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not over, (label, p, over)
    assert _sens_close(raw, ref)[0], label
    return raw, p


def _differing(a, b, vocab, names):
    return [name for name, o, n in W.segments(vocab) if name in names and not np.array_equal(_bits(a[o:o + n]),
                                                                                              _bits(b[o:o + n]))]


# ---- reached by shape alone ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(W.SHAPE_CASES))
def test_shape_reaches_its_path(case):
    import nicnes
    vocab, kind, rows, want = W.SHAPE_CASES[case]
    with _handle(vocab, kind, rows) as e:
        with pytest.raises(nicnes.NicnesError, match='first'):    # no run yet: nothing to report
            e.sens_paths()
        _, p = _check(e, vocab, kind, rows, want, case)
        assert p['gemm_v4'] > p['gemm_scalar']                    # a handle's theta is aligned: 16-byte loads


@pytest.mark.parametrize('case', sorted(W.FORCED_CASES))
def test_what_a_misaligned_theta_would_run(case, monkeypatch):
    """No handle holds a theta whose i2h / h2h weights are off 16-byte alignment (nicnes_create refuses V1 % 4 != 0:
    tests/test_sens_paths_host.py), so the two fallbacks that guard against one, the tile kernel's gemms for dX / dH
    and scalar loads in every product, are forced together here: at one tile of rows, at a full logit slab and past
    it (three row tiles of the scalar kernel, the logit fallback as well), with both thetas."""
    vocab, kind, rows, switches, want = W.FORCED_CASES[case]
    for s in switches:
        monkeypatch.setenv(W.SWITCHES[s], '1')
    with _handle(vocab, kind, rows) as e:
        _, p = _check(e, vocab, kind, rows, want, case)
        assert p['gemm_v4'] == 0 and p['gemm_scalar'] > 0


# ---- the switches, on one handle -------------------------------------------------------------------------------------
# the segments a switch can feed; every other one must keep base's bits (NICNES_SENS_TILE_BWD changes the products
# dX and dH of the recurrence, which everything but the logit segments reads; NICNES_SENS_TILE_SCALAR every product)
FEEDS = {'logit': {'logit.weight'}, 'emb': {'embed.weight'},
         'gates': {'core.i2h.weight', 'core.h2h.weight', 'img_embed.weight'},
         'bwd': set(W.SEGMENTS) - {'logit.weight', 'logit.bias'}, 'scalar': set(W.SEGMENTS)}


@pytest.fixture(scope='module')
def base_handle():
    vocab, kind, rows, _ = W.SHAPE_CASES['base']
    with _handle(vocab, kind, rows) as e:
        yield {'e': e, 'base': None}


@pytest.mark.parametrize('switch', sorted(W.SWITCHES))
def test_one_switch_changes_one_path(base_handle, switch, monkeypatch):
    vocab, kind, rows, want = W.SHAPE_CASES['base']
    e = base_handle['e']
    if base_handle['base'] is None:
        base_handle['base'] = _check(e, vocab, kind, rows, want, 'base')
    base, bp = base_handle['base']
    assert bp['gemm_v4'] > 0
    monkeypatch.setenv(W.SWITCHES[switch], '1')
    bit = W.SWITCH_BIT[switch]
    got, p = _check(e, vocab, kind, rows, W.paths(**({bit: False} if bit else {})), 'sw_' + switch)
    if switch == 'scalar':
        assert p['gemm_v4'] == 0 and p['gemm_scalar'] == bp['gemm_v4'] + bp['gemm_scalar']
    elif switch == 'bwd':                                         # two gemms per cell (one at the image cell)
        assert p['gemm_v4'] + p['gemm_scalar'] == bp['gemm_v4'] + bp['gemm_scalar'] + 2 * W.L + 1
    else:
        assert (p['gemm_v4'], p['gemm_scalar']) == (bp['gemm_v4'], bp['gemm_scalar'])
    differ = _differing(got, base, vocab, set(W.SEGMENTS) - FEEDS[switch])
    assert not differ, (switch, differ)
    monkeypatch.delenv(W.SWITCHES[switch])
    back = e.sum_sensitivity(rows).cpu().numpy()                  # and the fast path again gives base's bits
    assert np.array_equal(_bits(back), _bits(base)) and e.sens_paths() == bp


@pytest.mark.parametrize('world', [(999, 'wc', 41), (1027, 'wc', 65)], ids=['sw_all', 'sw_all_last_group'])
def test_all_switches_at_once(world, monkeypatch):
    """Every fallback in one run. At vocabulary 999 the last of the K = 11 groups is all padding (V1 = 1000): its seed
    is zero, and with one seed per k range so is the last partial row of every fallback's square sums; a fallback that
    summed one partial row too few would pass there. At 1027 the last group holds 28 words."""
    vocab, kind, rows = world
    for name in W.SWITCHES.values():
        monkeypatch.setenv(name, '1')
    with _handle(vocab, kind, rows) as e:
        _, p = _check(e, vocab, kind, rows, {k: False for k in W.ALL_FAST}, 'sw_all')
        assert p['gemm_v4'] == 0 and p['gemm_scalar'] > 0


def test_forced_embedding_ranges_at_a_small_K(monkeypatch):
    """K = 2 under NICNES_SENS_EMB_KC: six of sens_emb_sq's EMB_KC = 8 ranges start past K and must write zeros"""
    vocab, kind, rows = 127, 'xavier', 12
    with _handle(vocab, kind, rows) as e:
        base, _ = _check(e, vocab, kind, rows, W.ALL_FAST, 'small_K_base')
        monkeypatch.setenv(W.SWITCHES['emb'], '1')
        got, _ = _check(e, vocab, kind, rows, W.paths(emb_two_pass=False), 'small_K_emb')
        assert not _differing(got, base, vocab, set(W.SEGMENTS) - FEEDS['emb'])


# ---- the buffers that persist between calls --------------------------------------------------------------------------
def test_buffers_reused_over_shrinking_and_growing_rows():
    """One handle called with rows 12, 129, 8, 128, 12: the work buffers grow once (12 -> 129) and are then reused by
    smaller batches, the logit path flips at 129 and back, and each segment sums another number of partial rows per
    path. Every call gives the bits of a fresh handle called once with that rows."""
    vocab, kind = 999, 'wc'
    fresh = {}
    for rows in sorted(set(W.REUSE_ROWS)):
        with _handle(vocab, kind, 129) as e:
            fresh[rows] = _check(e, vocab, kind, rows, W.paths(logit_fast=rows <= 128), 'fresh_%d' % rows)
    with _handle(vocab, kind, 129) as e:
        got = []
        for rows in W.REUSE_ROWS:
            raw = e.sum_sensitivity(rows).cpu().numpy()
            assert e.sens_paths() == fresh[rows][1], rows
            differ = _differing(raw, fresh[rows][0], vocab, set(W.SEGMENTS))
            assert not differ, (rows, differ)
            got.append(raw)
        assert np.array_equal(_bits(got[0]), _bits(got[-1]))


# ---- nic_es shares the work buffers -----------------------------------------------------------------------------------
def test_es_rows_on_the_logit_fallback():
    """nicnes_sensitivity_es shares the handle's work buffers: at 129 rows (the logit fallback; tests/test_gpu_es_safe.py
    runs 8 and 12) es_sensitivity([0, 2]) writes rows that are sum_sensitivity of that parent bit for bit (its
    test_rows pattern, three 'wc' parents), each within the bar, and sens_paths() reports the last slot's run."""
    import nicnes
    vocab, rows = W.ES_VOCAB, W.ES_ROWS
    want = W.paths(logit_fast=False)
    with _handle(vocab, None, rows, es_parents=W.ES_SEEDS) as e:
        with pytest.raises(nicnes.NicnesError, match='first'):
            e.sens_paths()
        e.es_sensitivity([0, 2], rows, UNDERFLOW)
        p_es = e.sens_paths()
        assert _bits_of(p_es) == want
        got = {s: e.es_sensitivity_row(s).cpu().numpy() for s in (0, 2)}
        assert not np.array_equal(got[0], got[2])
        with pytest.raises(nicnes.NicnesError, match='invalid'):
            e.es_sensitivity_row(1)
        for s in (0, 2):
            e.es_load_theta(s)
            assert np.array_equal(_bits(e.sum_sensitivity(rows, UNDERFLOW)), _bits(got[s])), s
            assert e.sens_paths() == p_es
            _check(e, vocab, W.ES_SEEDS[s], rows, want, 'es_parent_%d' % s)
        e.es_sensitivity([0, 2], rows, UNDERFLOW)
        assert all(np.array_equal(_bits(e.es_sensitivity_row(s)), _bits(got[s])) for s in (0, 2))


# ---- the rows limit ----------------------------------------------------------------------------------------------------
def test_rows_limit_is_refused_by_name():
    """5 * rows <= 4096 (the embedding kernels' pair list): rows = 820 is refused with the limit named, at both
    entries, before nicnes_sens_run is entered (sens_paths() still reports the run before); the handle then gives the
    bits it gave before, and rows = 819, the largest, meets the bar."""
    import nicnes
    vocab, kind = 127, 'xavier'
    with _handle(vocab, kind, W.MAX_ROWS + 1) as e:
        raw, p = _check(e, vocab, kind, 12, W.ALL_FAST, 'limit_rows_12')
        with pytest.raises(nicnes.NicnesError, match=r'not supported.*rows <= 819'):
            e.sum_sensitivity(W.MAX_ROWS + 1)
        assert e.sens_paths() == p                                # no run was started
        e.es_create(2, 1)
        e.es_set_parents([W.theta_of(vocab, kind)])
        e.es_set_mutation_divide()
        with pytest.raises(nicnes.NicnesError, match=r'not supported.*rows <= 819'):
            e.es_sensitivity([0], W.MAX_ROWS + 1, UNDERFLOW)
        assert e.sens_paths() == p
        assert np.array_equal(_bits(e.sum_sensitivity(12)), _bits(raw))
        _check(e, vocab, kind, W.MAX_ROWS, W.paths(logit_fast=False), 'limit_rows_819')
        assert np.array_equal(_bits(e.sum_sensitivity(12)), _bits(raw))
