"""CPU: the host restatement of the teacher-forced cross-entropy (tests/xent_ref.py) and the experiment spec's side of
the 'xent' fitness.

The restatement against tests/golden/xent.npz (scripts/make_golden_xent.py: the imported reference's img_embed, embed,
core and logit driven teacher-forced, F.log_softmax(...).gather): the bar on every counted lp_s is 2 x the largest
difference measured when the fixture was made. That measurement: 5.72e-06 over the 373 counted targets of 59 label rows
x 5 candidates (theta and two members of both signs; torch 2.x CPU against oracle.gemv chains and the oracle's fp64
exp-sum), so the bar is 1.144e-05 -- the order of the 5e-6 tests/test_wide_host.py holds the oracle's own log-probs to
against the same reference. The value is stored in the fixture ('measured_max_diff') and asserted to be the one quoted
here."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import xent_ref as X

MEASURED = 5.72e-06
BAR = 2 * MEASURED


@pytest.fixture(scope='module')
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, 'xent.npz'))
    V, E, R, F, T = (int(v) for v in z['dims'])
    d = O.Dims(vocab_size=V, E=E, R=R, F=F, T=T)
    theta = O.make_theta(d, int(z['theta_seed']), float(z['gain']), float(z['bias_std']))
    fc = np.random.Generator(np.random.PCG64(int(z['fc_seed']))).standard_normal((int(z['B']), F)).astype(np.float32)
    table = O.noise_table(int(z['noise_len']), int(z['table_seed']))
    cands = [theta]
    for m in z['members']:
        idx = O.noise_index(int(z['noise_seed']), int(z['iteration']), int(m), int(z['noise_len']), d.D)
        cands += [O.perturb(theta, table, idx, float(z['sigma']), sign) for sign in (+1, -1)]
    return dict(z=z, d=d, fc=fc, cands=cands)


def test_fixture_shape_and_measurement(golden):
    z = golden['z']
    lab = z['labels']
    assert lab.shape == (59, 16) and z['logprobs'].shape == (5, 59, 17)
    assert sorted(set((lab > 0).sum(1))) == [0, 1, 5, 16]
    assert sorted(set(np.bincount(z['row_img']))) == [1, 2, 3, 4, 5, 6, 7]
    assert abs(float(z['measured_max_diff']) - MEASURED) <= 0.005e-06, float(z['measured_max_diff'])
    assert str(z['torch_version']) and str(z['numpy_version'])


def test_restatement_against_the_reference(golden):
    z, d = golden['z'], golden['d']
    lab = z['labels']
    mask = X.counted(lab)
    worst = 0.0
    for th, ref in zip(golden['cands'], z['logprobs']):
        lp, lp_sum, n_tok = X.forced(d, th, golden['fc'][z['row_img']], lab)
        assert np.array_equal(n_tok, mask.sum(1))                       # n_tok exact
        assert np.array_equal(lp != 0, mask & (lp != 0)) and np.array_equal(ref != 0, mask & (ref != 0))
        worst = max(worst, float(np.abs(lp.astype(np.float64) - ref)[mask].max()))
        resum = np.zeros(lab.shape[0])
        for s in range(lp.shape[1]):
            resum = np.where(mask[:, s], resum + lp[:, s].astype(np.float64), resum)
        assert np.array_equal(lp_sum, resum)
    print('largest |xent_ref - reference| %.3g (bar %.3g)' % (worst, BAR))
    assert worst <= BAR


def test_mask_rules_on_hand_made_rows():
    d = O.Dims(vocab_size=67, F=128)
    theta = O.make_theta(d, 0, 4.0, 0.1)
    lab = np.zeros((3, 16), np.int32)
    lab[1] = np.arange(1, 17)                    # 16 words
    lab[2, :3] = (5, 6, 7)
    fc = np.random.Generator(np.random.PCG64(5)).standard_normal((3, 128)).astype(np.float32)
    lp, lp_sum, n_tok = X.forced(d, theta, fc, lab)
    assert n_tok.tolist() == [1, 17, 4]          # an empty row: one target (the end token); 16 words: 17
    assert (lp[0, 1:] == 0).all() and lp[0, 0] < 0
    assert (lp[1] < 0).all()
    assert (lp[2, :4] < 0).all() and (lp[2, 4:] == 0).all()
    assert X.counted(lab).sum(1).tolist() == [1, 17, 4]
    assert X.loss_of(lp_sum, n_tok) == pytest.approx(-lp_sum.sum() / 22, rel=1e-15)
    # a row's log-probs do not depend on the rows beside it
    one, _, _ = X.forced(d, theta, fc[2:], lab[2:])
    assert np.array_equal(one[0], lp[2])


def test_a_greedy_decodes_tokens_fed_back_give_the_oracle_decodes_log_probs():
    d = O.Dims(vocab_size=67, F=128)
    theta = O.make_theta(d, 0, 4.0, 0.1)
    fc = np.random.Generator(np.random.PCG64(1)).standard_normal((8, 128)).astype(np.float32)
    seq, lp, fragile = O.decode(d, theta, fc)
    mine, _, n_tok = X.forced(d, theta, fc, seq)
    mask = X.counted(seq)[:, :d.T]
    assert (seq > 0).any() and np.array_equal(n_tok, (seq > 0).sum(1) + 1)
    assert np.array_equal(mine[:, :d.T][mask], lp[mask])                # the same chains: bit for bit


def _exp(fitness='xent', mo=None, algorithm='nic_nes'):
    return {'algorithm': algorithm, 'nb_offspring': 4, 'config': {'noise_stdev': 0.01, 'batch_size': 8},
            'policy_options': {'net': 'fc_caption', 'fitness': fitness, 'model_options': dict(mo or {})}}


def test_spec_accepts_xent_and_refuses_what_the_engine_refuses():
    from nicnes import config as C
    from nicnes.engine import Engine
    s = C.ExperimentSpec(_exp())
    assert s.fitness == 'xent' and 'xent' in C.XENT_FITNESS and 'xent' not in C.FITNESS
    assert Engine.FITNESS_MODES['xent'] == 8 == Engine.XENT_MODE
    for mo in ({'rnn_size': 256}, {'input_encoding_size': 384}, {'layer_n': True}, {'safe_mutations': 'SM-G-SUM'},
               {'safe_mutations': 'SM-VECTOR'}, {'safe_mutations': 'SM-PROPORTIONAL'}):
        with pytest.raises(C.NotSupported, match='xent'):
            C.ExperimentSpec(_exp(mo=mo))
    with pytest.raises(C.NotSupported):
        C.ExperimentSpec(_exp('xent2'))
    C.ExperimentSpec(_exp('greedy', {'rnn_size': 256}))                  # what was accepted stays accepted


def test_es_spec_keeps_refusing_xent():
    from nicnes import config as C
    from nicnes import es
    exp = _exp(algorithm='nic_es')
    exp.update({'population_size': 4, 'num_elites': 1, 'num_elite_cands': 1})
    with pytest.raises(C.NotSupported, match='xent'):
        es.ESExperimentSpec(exp)
    exp['policy_options']['fitness'] = 'greedy'
    assert es.ESExperimentSpec(exp).fitness == 'greedy'
