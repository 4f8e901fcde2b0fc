"""nic_es on the coop decode path (nicnes_set_decode_es, nicnes_decode_coop_es_kernel): the offspring of several base
thetas decoded by S = 2 or 4 workgroups per pair and slab in one persistent launch, against the fused ES evaluate of the
same handle (bit for bit) and the oracle, on the world of tests/test_gpu_es.py (its parents, seeds, PARENT_OF, table)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from oracle import cider_ref as CR      # noqa: E402
from tests import test_gpu_es as E      # noqa: E402  (the world only: nothing of it is modified)

GEN, SIGMA, PARENT_OF, FRAGILE_CAP = E.GEN, E.SIGMA, E.PARENT_OF, E.FRAGILE_CAP
_oracle = {}


def _oracle_offspring(B, mode):
    """The oracle's tokens and fragile rows of the five pairs, computed once per (B, mode) and never modified."""
    if (B, mode) not in _oracle:
        _oracle[B, mode] = E._oracle_offspring(B, mode, PARENT_OF)
    return _oracle[B, mode]


def _loaded_engine(B, mode, **kw):
    import nicnes
    fc, gts, df, n = E._workload(B)
    e = E._engine(B, **kw)
    keys, vals = nicnes.df_table_arrays(df)
    e.set_df_table(keys, vals, np.log(float(n)))
    e.set_batch(fc, gts)
    e.es_set_parents(E._world()[1])
    e.es_set_mutation(mode)
    return e


def _bits(t, dtype):
    return t.cpu().numpy().view(dtype)


@pytest.mark.parametrize('B', [24, 130], ids=['B24_one_partial_slab', 'B130_two_slabs'])
@pytest.mark.parametrize('mode', E.MODES)
def test_coop_equals_fused_and_oracle(monkeypatch, mode, B):
    """('coop', S) for S = 2, 4: tokens and greedy fitness bit-identical to the fused ES evaluate of the same handle, the
    oracle's on non-fragile rows; the slices (0, 2) + (2, 3) equal (0, 5) (pair_begin > 0: parent_of shifts with the
    members); no hand-off timed out; es_decode_path names the path taken."""
    fc, gts, df, n = E._workload(B)
    oseq, frag = _oracle_offspring(B, mode)
    assert frag.mean() <= FRAGILE_CAP, 'too many fragile rows (%.3f): change the seed, not the cap' % frag.mean()
    monkeypatch.setenv('NICNES_BOUNDED_LSE', '1')          # the pair-bounded instantiations, whatever ran before
    e = _loaded_engine(B, mode)
    try:
        e.set_decode_screen(False)
        assert e.es_decode_path(B, 5) == 'fused'           # the default mode
        fit, seq = e.es_evaluate(GEN, 0, 5, SIGMA, PARENT_OF, return_seq=True)
        fit, seq = fit.cpu().numpy(), seq.cpu().numpy()
        for S in (2, 4):
            e.es_set_decode('coop', S)
            assert e.es_decode_path(B, 5) == 'coop' and e.es_decode_path(B, 2) == 'coop'
            fc_, sc_ = e.es_evaluate(GEN, 0, 5, SIGMA, PARENT_OF, return_seq=True)
            assert np.array_equal(_bits(sc_, np.uint32), seq.view(np.uint32)), S
            assert np.array_equal(_bits(fc_, np.uint64), fit.view(np.uint64)), S
            E._check_against_oracle(sc_.cpu().numpy(), fc_.cpu().numpy(), oseq, frag, CR.CiderDOracle(df, n), gts)
            fa, sa = e.es_evaluate(GEN, 0, 2, SIGMA, PARENT_OF[:2], return_seq=True)
            fb, sb = e.es_evaluate(GEN, 2, 3, SIGMA, PARENT_OF[2:], return_seq=True)
            assert np.array_equal(np.concatenate([sa.cpu().numpy(), sb.cpu().numpy()]), seq), S
            assert np.array_equal(np.concatenate([_bits(fa, np.uint64), _bits(fb, np.uint64)]), fit.view(np.uint64)), S
        assert e.stats()['coop_timeouts'] == 0
        e.es_set_decode('fused')
        assert e.es_decode_path(B, 5) == 'fused'
        f2, s2 = e.es_evaluate(GEN, 0, 5, SIGMA, PARENT_OF, return_seq=True)
        assert np.array_equal(s2.cpu().numpy(), seq) and np.array_equal(_bits(f2, np.uint64), fit.view(np.uint64))
    finally:
        e.close()


@pytest.mark.parametrize('B', [24, 130], ids=['B24_one_partial_slab', 'B130_two_slabs'])
@pytest.mark.parametrize('mode', E.MODES)
def test_logprob_criterion(mode, B):
    """greedy_logprob on the coop path (the exact exp-sum instantiations): the tokens of the fused evaluate, log-probs
    within the project's 1e-5 of its up to each row's end token, fitness within 1e-6 relative."""
    e = _loaded_engine(B, mode)
    try:
        e.set_fitness_mode('greedy_logprob')
        f0, s0, l0 = (t.cpu().numpy() for t in e.es_evaluate(GEN, 0, 5, SIGMA, PARENT_OF, return_seq=True, return_lp=True))
        ended = np.cumsum(np.cumsum(s0 == 0, axis=-1), axis=-1) > 1        # after a row's end token
        for S in (2, 4):
            e.es_set_decode('coop', S)
            f, s, lp = (t.cpu().numpy() for t in e.es_evaluate(GEN, 0, 5, SIGMA, PARENT_OF, return_seq=True,
                                                               return_lp=True))
            assert np.array_equal(s, s0), S
            err = np.abs(lp - l0)[~ended].max()
            print('B %d %s S %d: max |lp - lp_fused| %.3g, max rel fitness %.3g'
                  % (B, mode, S, err, (np.abs(f - f0) / np.maximum(1.0, np.abs(f0))).max()))
            assert err <= 1e-5, (S, err)
            assert (np.abs(f - f0) <= 1e-6 * np.maximum(1.0, np.abs(f0))).all(), (S, f, f0)
        assert e.stats()['coop_timeouts'] == 0
    finally:
        e.close()


def test_member_batches():
    """A pair on per-member batch 1 sees that batch's images, as on the fused path."""
    B = 24
    fc, gts, df, n = E._workload(B)
    e = _loaded_engine(B, 'plain')
    try:
        e.set_batches([(fc, gts), (fc[::-1].copy(), gts[::-1])])
        f0, s0 = e.es_evaluate(GEN, 0, 2, SIGMA, [1, 1], return_seq=True, member_batch=[0, 1])
        for S in (2, 4):
            e.es_set_decode('coop', S)
            f, s = e.es_evaluate(GEN, 0, 2, SIGMA, [1, 1], return_seq=True, member_batch=[0, 1])
            assert not np.array_equal(s.cpu().numpy()[0], s.cpu().numpy()[1])
            assert np.array_equal(s.cpu().numpy(), s0.cpu().numpy()) and np.array_equal(_bits(f, np.uint64), _bits(f0, np.uint64))
            f1, s1 = e.es_evaluate(GEN, 1, 1, SIGMA, [1], return_seq=True, member_batch=[1])
            assert np.array_equal(s1.cpu().numpy()[0], s.cpu().numpy()[1])
        assert e.stats()['coop_timeouts'] == 0
    finally:
        e.close()


def test_auto_rule_and_refusals():
    """'auto' follows the handle's own shape rule (coop at an 8-GPU share of mscoco_es.json, fused at the whole
    generation, on a 256-CU device) and nicnes_set_decode_coop(0); a coop S whose grid cannot be resident at once is
    refused before anything is launched."""
    import nicnes
    B = 8
    occ, socc = ctypes.c_int(), ctypes.c_int()
    e0 = nicnes.Engine(max_batch=8, max_members=1, noise_len=E.NOISE_LEN, noise_seed=E.SEED)
    assert e0.L.nicnes_decode_occupancy(ctypes.byref(occ), ctypes.byref(socc)) == 0
    e0.close()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    unfit = occ.value * n_cu // 4 + 1                    # pairs whose count x 1 slab x 4 workgroups exceed occupancy x CUs
    e = _loaded_engine(B, 'plain', members=max(500, unfit))
    try:
        def want(Bq, count):                              # from the nic_nes rule of the same handle, not a literal
            return 'coop' if e.decode_path(Bq, count) == 'coop' else 'fused'
        e.es_set_decode('auto')
        assert e.es_decode_path(256, 63) == want(256, 63)
        assert e.es_decode_path(256, 500) == want(256, 500)
        if n_cu == 256:
            assert want(256, 63) == 'coop' and want(256, 500) == 'fused'
        e.set_decode_coop(0)
        assert e.es_decode_path(256, 63) == 'fused'
        e.set_decode_coop(1)
        e.es_set_decode('coop', 4)
        before = e.stats()
        with pytest.raises(nicnes.NicnesError, match='occupancy x CUs'):
            e.es_evaluate(GEN, 0, unfit, SIGMA, [0] * unfit)
        with pytest.raises(nicnes.NicnesError, match='occupancy x CUs'):
            e.es_decode_path(B, unfit)
        assert e.es_decode_path(B, unfit - 1) == 'coop'
        with pytest.raises(nicnes.NicnesError):
            e.es_set_decode('coop', 3)
        torch.cuda.synchronize()
        assert e.stats() == before                        # nothing ran
        e.es_set_decode('fused')
        e.es_evaluate(GEN, 0, 1, SIGMA, [0])
        torch.cuda.synchronize()
    finally:
        e.close()
