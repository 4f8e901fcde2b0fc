"""CPU: models wider than 128 units (rnn_size / input_encoding_size in 128, 256, 384, 512), the host side.

* The C oracle against tests/golden/decode_wide.npz (FCModel._sample of the imported reference at (E, R) = (256, 256),
  (128, 384), (512, 128), scripts/make_golden.py): tokens equal on every row that is not fragile, at most 5 % of a case's
  rows fragile (the cap of tests/test_gpu_dims.py), log-probs of theta itself to 1e-5. This is what lets the GPU tests of
  tests/test_gpu_wide.py compare against the oracle. Counts here: no row of the 3 x 5 x 16 is fragile.
* ExperimentSpec / ESExperimentSpec refuse what the engine refuses at wide dims: a sampled fitness, SM-G-SUM, nic_es.
* engine_kwargs, param_shapes and the state-dict round trip (through a .pth read with weights_only=True) at wide dims."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import oracle as O

torch = pytest.importorskip('torch')

import os  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'decode_wide.npz')
MARGIN = 1e-5          # reference top-1 / top-2 log-prob margin below which a step is a near-tie (tests/test_oracle_golden.py)
FRAGILE_CAP = 0.05


def wide_cases():
    """The fixture's cases: (name, dims, theta, fc, [(theta of the rollout, reference seq, margins, log-probs or None)])."""
    z = np.load(GOLDEN)
    out = []
    for name in z['cases']:
        def g(k, name=name):
            return z['%s/%s' % (name, k)]
        V, E, R, F, T = [int(x) for x in g('dims')]
        d = O.Dims(vocab_size=V, E=E, R=R, F=F, T=T)
        theta = O.make_theta(d, int(g('theta_seed')), float(g('gain')), float(g('bias_std')))
        fc = np.random.Generator(np.random.PCG64(int(g('fc_seed')))).standard_normal((int(g('B')), F)).astype(np.float32)
        table = O.noise_table(int(g('noise_len')), int(g('table_seed')))
        rolls = [(theta, g('seq'), g('margins'), g('logprobs'))]
        i = 0
        for m in g('members'):
            idx = O.noise_index(int(g('noise_seed')), int(g('iteration')), int(m), int(g('noise_len')), d.D)
            for sign in (+1, -1):
                rolls.append((O.perturb(theta, table, idx, float(g('sigma')), sign), g('member_seq')[i],
                              g('member_margins')[i], None))
                i += 1
        out.append((str(name), d, theta, fc, rolls))
    return out


def test_oracle_equals_the_reference_fixture_at_wide_dims():
    cases = wide_cases()
    assert [(c[1].E, c[1].R) for c in cases] == [(256, 256), (128, 384), (512, 128)]
    for name, d, theta, fc, rolls in cases:
        assert (d.V1, d.F) == (68, 128) and len(rolls) == 5
        n_frag = n_rows = 0
        for th, rseq, mar, rlp in rolls:
            seq, lp, fr = O.decode(d, th, fc)
            frag = fr.any(1) | (mar < MARGIN).any(1)
            n_frag += int(frag.sum())
            n_rows += frag.size
            assert np.array_equal(seq[~frag], rseq[~frag]), name
            if rlp is not None:                    # theta itself: the reference's seq_logprobs
                keep = np.concatenate([np.ones((len(rseq), 1), bool), rseq[:, :-1] > 0], 1) & ~frag[:, None]
                assert np.abs(lp[keep] - rlp[keep]).max() <= 1e-5, name
            assert np.unique(rseq).size >= 12, name          # not one id over and over
        assert n_frag <= FRAGILE_CAP * n_rows, 'too many fragile rows in %s (%d of %d): re-seed the case' % (
            name, n_frag, n_rows)


# ------------------------------------------------------------------------------------------------ spec refusals
NES = {'algorithm': 'nic_nes', 'nb_offspring': 4,
       'config': {'noise_stdev': 0.01, 'batch_size': 8, 'l2coeff': 1e-3},
       'policy_options': {'net': 'fc_caption', 'fitness': 'greedy', 'model_options': {}},
       'optimizer_options': {'type': 'adam', 'args': {'stepsize': 1e-3}}}
ES = {'algorithm': 'nic_es', 'dataset': 'mscoco', 'nb_offspring': 8, 'population_size': 4, 'num_elites': 1,
      'num_elite_cands': 1, 'selection': 'uniform',
      'config': {'noise_stdev': 0.005, 'batch_size': 8},
      'policy_options': {'net': 'fc_caption', 'fitness': 'greedy', 'model_options': {}}}


def _exp(base, fitness='greedy', **mo):
    e = copy.deepcopy(base)
    e['policy_options']['fitness'] = fitness
    e['policy_options']['model_options'] = dict(mo)
    return e


WIDTHS = [dict(rnn_size=256), dict(input_encoding_size=384), dict(rnn_size=512, input_encoding_size=256)]


@pytest.mark.parametrize('w', WIDTHS, ids=lambda w: '_'.join('%s%d' % (k[0], v) for k, v in w.items()))
def test_specs_refuse_what_the_engine_refuses_at_wide_dims(w):
    from nicnes.config import ExperimentSpec, NotSupported, GREEDY_FITNESS, SAMPLED_FITNESS
    from nicnes.es import ESExperimentSpec
    for f in GREEDY_FITNESS:                       # the greedy modes and the materialised mutations stay
        for m in ('', 'SM-PROPORTIONAL'):
            s = ExperimentSpec(_exp(NES, f, safe_mutations=m, **w))
            assert s.fitness == f and s.mutation == m
    ExperimentSpec(_exp(NES, safe_mutations='SM-VECTOR', safe_mutation_vector='v.pth', **w))
    for f in SAMPLED_FITNESS:
        with pytest.raises(NotSupported, match='wider than 128'):
            ExperimentSpec(_exp(NES, f, **w))
    with pytest.raises(NotSupported, match='SM-G-SUM'):
        ExperimentSpec(_exp(NES, safe_mutations='SM-G-SUM', safe_mutation_underflow=0.01, **w))
    for m in ('', 'SM-PROPORTIONAL'):
        with pytest.raises(NotSupported, match='nic_es'):
            ESExperimentSpec(_exp(ES, safe_mutations=m, **w))


def test_specs_at_the_default_widths_are_as_before():
    from nicnes.config import ExperimentSpec
    from nicnes.es import ESExperimentSpec
    for mo in (dict(), dict(rnn_size=128, input_encoding_size=128)):
        assert ExperimentSpec(_exp(NES, 'sample', **mo)).fitness == 'sample'
        assert ExperimentSpec(_exp(NES, safe_mutations='SM-G-SUM', safe_mutation_underflow=0.01, **mo)).mutation == 'SM-G-SUM'
        assert ESExperimentSpec(_exp(ES, **mo)).n_pairs == 4


# ------------------------------------------------------------------------------------------------ state dict
def test_engine_kwargs_and_param_shapes_at_wide_dims():
    from nicnes.config import ExperimentSpec
    from nicnes import nes as N
    s = ExperimentSpec(_exp(NES, rnn_size=384, input_encoding_size=256, fc_feat_size=128), vocab_size=67)
    kw = s.engine_kwargs(max_members=4, noise_len=1 << 21)
    assert (kw['rnn_size'], kw['input_encoding_size'], kw['fc_feat_size'], kw['vocab_size']) == (384, 256, 128, 67)
    d = O.Dims(vocab_size=67, E=256, R=384, F=128)
    eng = SimpleNamespace(cfg=SimpleNamespace(vocab_size=67, input_encoding_size=256, rnn_size=384, fc_feat_size=128))
    shapes = N.param_shapes(eng)
    assert [(k, tuple(v)) for k, v in shapes.items()] == [(k, tuple(v)) for k, v in d.shapes()]
    assert sum(int(np.prod(v)) for v in shapes.values()) == d.D


def test_wide_state_dict_round_trips_through_a_pth(tmp_path):
    from nicnes import nes as N
    d = O.Dims(vocab_size=67, E=512, R=256, F=128)
    eng = SimpleNamespace(cfg=SimpleNamespace(vocab_size=67, input_encoding_size=512, rnn_size=256, fc_feat_size=128))
    shapes = N.param_shapes(eng)
    theta = torch.from_numpy(O.make_theta(d, 3, 4.0, 0.1))
    sd = N.state_dict_from_vector(theta, shapes)
    assert sd['core.h2h.weight'].shape == (5 * 256, 256) and sd['core.i2h.weight'].shape == (5 * 256, 512)
    off = d.offsets()['core.i2h.weight'][0]
    assert torch.equal(sd['core.i2h.weight'].reshape(-1), theta[off: off + 5 * 256 * 512])
    path = str(tmp_path / 'wide.pth')
    torch.save(sd, path)
    back = N.vector_from_state_dict(torch.load(path, weights_only=True), shapes)
    assert back.dtype == torch.float32 and torch.equal(back, theta)
    narrow = N.param_shapes(SimpleNamespace(cfg=SimpleNamespace(vocab_size=67, input_encoding_size=128, rnn_size=256,
                                                                 fc_feat_size=128)))
    with pytest.raises(ValueError, match='shape'):
        N.vector_from_state_dict(sd, narrow)
