"""CPU: layer_n models (LSTMCore with nn.LayerNorm on i2h(x), h2h(h) and next_c), the host side.

* tests/ln_ref.py with the normalisation switched off is the C oracle's decode bit for bit, tokens and log-probs: that
  pins the restatement the GPU tests of tests/test_gpu_layernorm.py compare against.
* ln_ref against tests/golden/decode_layernorm.npz (FCModel._sample of the imported reference with layer_n=True at
  (E, R) = (128, 128) and (256, 256), without and with affine; scripts/make_golden_ln.py): tokens equal on every row
  that is not excluded. A row is excluded when it is fragile or its stored reference margin at a live step is below
  MARGIN. MARGIN is measured, not chosen: 4 x the largest |log-prob of ln_ref - log-prob of the reference| over the
  live steps of theta itself in the fixture. That largest difference is 1.1205673e-05 (case e256_r256; the other three
  cases 3.8e-06, 4.1e-06, 5.1e-06), so MARGIN = 4.49e-05; the factor 4 covers the perturbed members, whose errors are of
  the same kind. At most 5 % of a case's rows may be excluded (FRAGILE_CAP of tests/test_wide_host.py). Counts here: no
  row of the 4 x 5 x 16 is excluded (the smallest stored live margin is 4.94e-05, a member of e128_r128).
* The statistics on edge rows: a constant row, a row of mean 1e4 with unit spread, N = 128 and N = 2,560.
* ExperimentSpec accepts layer_n and refuses with it what the engine refuses; ESExperimentSpec keeps refusing it; the
  parameter layout with and without the affine tail; the state-dict round trip under the fixture's names."""
import copy
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import oracle as O

from tests import ln_ref as L

torch = pytest.importorskip('torch')

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'decode_layernorm.npz')
LP_DIFF = 1.1205673e-05        # measured: see the header
MARGIN = 4.49e-05              # 4 x LP_DIFF
FRAGILE_CAP = 0.05


def live_steps(seq):
    return np.concatenate([np.ones((len(seq), 1), bool), seq[:, :-1] > 0], 1)


def ln_cases():
    """The fixture's cases: (name, dims, affine, theta, fc, [(theta of the rollout, seq, margins, log-probs or None)])"""
    z = np.load(GOLDEN)
    out = []
    for name in z['cases']:
        def g(k, name=name):
            return z['%s/%s' % (name, k)]
        V, E, R, F, T = [int(x) for x in g('dims')]
        d = O.Dims(vocab_size=V, E=E, R=R, F=F, T=T)
        theta = O.make_theta(d, int(g('theta_seed')), float(g('gain')), float(g('bias_std')))
        if int(g('affine')):
            theta = np.concatenate([theta, L.make_tail(R, int(g('tail_seed')), float(g('tail_scale')))])
        assert theta.size == int(g('D'))
        fc = np.random.Generator(np.random.PCG64(int(g('fc_seed')))).standard_normal((int(g('B')), F)).astype(np.float32)
        table = O.noise_table(int(g('noise_len')), int(g('table_seed')))
        rolls = [(theta, g('seq'), g('margins'), g('logprobs'))]
        i = 0
        for m in g('members'):
            idx = O.noise_index(int(g('noise_seed')), int(g('iteration')), int(m), int(g('noise_len')), theta.size)
            for sign in (+1, -1):
                rolls.append((O.perturb(theta, table, idx, float(g('sigma')), sign), g('member_seq')[i],
                              g('member_margins')[i], None))
                i += 1
        out.append((str(name), d, bool(int(g('affine'))), theta, fc, rolls))
    return out


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize('E,R,V,F,B', [(128, 128, 67, 128, 16), (256, 128, 67, 256, 6), (128, 256, 11, 128, 6)])
def test_ln_ref_without_the_normalisation_is_the_oracle_bit_for_bit(E, R, V, F, B):
    d = O.Dims(vocab_size=V, E=E, R=R, F=F)
    theta = O.make_theta(d, 5, 4.0, 0.1)
    fc = np.random.Generator(np.random.PCG64(77)).standard_normal((B, F)).astype(np.float32)
    seq, lp, fr = L.Model(d, theta, layer_n=False).decode(fc)
    oseq, olp, ofr = O.decode(d, theta, fc)
    assert np.array_equal(seq, oseq)
    assert np.array_equal(lp.view(np.uint32), olp.view(np.uint32))
    assert np.array_equal(fr, ofr)
    assert np.unique(seq).size >= 4


def test_ln_ref_equals_the_reference_fixture():
    cases = ln_cases()
    assert [(c[1].E, c[1].R, c[2]) for c in cases] == [(128, 128, False), (256, 256, False), (128, 128, True),
                                                       (256, 256, True)]
    assert list(np.load(GOLDEN)['ln_names']) == L.LN_NAMES
    worst = 0.0
    for name, d, affine, theta, fc, rolls in cases:
        assert (d.V1, d.F) == (68, 128) and len(rolls) == 5
        n_ex = n_rows = 0
        for th, rseq, mar, rlp in rolls:
            seq, lp, fr = L.Model(d, th).decode(fc)
            live = live_steps(rseq)
            ex = fr.any(1) | ((mar < MARGIN) & live).any(1)
            n_ex += int(ex.sum())
            n_rows += ex.size
            assert np.array_equal(seq[~ex], rseq[~ex]), name
            if rlp is not None:                    # theta itself: the reference's seq_logprobs
                diff = float(np.abs(lp - rlp)[live].max())
                print('%s: largest |lp - reference lp| over the live steps of theta %.7e' % (name, diff))
                worst = max(worst, diff)
                assert not ex.any(), name          # theta itself excludes none
            assert np.unique(rseq).size >= 12, name
        print('%s: %d of %d rows excluded' % (name, n_ex, n_rows))
        assert n_ex <= FRAGILE_CAP * n_rows, 'too many excluded rows in %s (%d of %d): re-seed the case' % (
            name, n_ex, n_rows)
    # the threshold in the header is the measured one
    assert worst <= LP_DIFF * (1 + 1e-6) and 4 * worst <= MARGIN


# ------------------------------------------------------------------------------------------------ statistics
def _norm64(a):
    a = a.astype(np.float64)
    return (a - a.mean(1, keepdims=True)) / np.sqrt(a.var(1, keepdims=True) + 1e-5)


@pytest.mark.parametrize('N', [128, 2560])
def test_statistics_on_edge_rows(N):
    rng = np.random.Generator(np.random.PCG64(N))
    # a constant row: var = 0, y = 0 exactly (every d is a - mean with mean == a when N is a power of two times
    # the value's exactness; here 0.75 sums exactly)
    const = np.full((3, N), 0.75, np.float32)
    y = L.layer_norm(const)
    assert np.array_equal(y, np.zeros_like(y))
    g, b = rng.standard_normal(N).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    assert np.array_equal(L.layer_norm(const, g, b), np.broadcast_to(b, (3, N)))      # 0 * gamma + beta
    # unit spread: fp32 rounding of N sequential adds and the division
    x = rng.standard_normal((4, N)).astype(np.float32)
    assert np.abs(L.layer_norm(x) - _norm64(x)).max() <= 1e-5
    # mean 1e4 with unit spread. A lane's running sum reaches N / 2 * 1e4 <= 1.28e7 < 2^24, so every one of its N / 2
    # adds rounds by at most half an ulp <= 0.5, about 0.29 rms; as a random walk a lane sum is off by about
    # 0.29 sqrt(N / 2) ~ 10, the mean by about 14.6 / N ~ 0.006 at N = 2,560 (far less at 128), and y = d / ~1 by the
    # same: 0.05 is some nine of those. The centred second pass then sees the spread itself (its error is second order
    # in the mean's), where E[x^2] - mean^2 at 1e8 with an ulp of 8 would leave nothing of a variance of 1: the
    # normalised row's own spread within 2 % of 1
    big = (x + np.float32(1e4)).astype(np.float32)
    yb = L.layer_norm(big)
    ref = _norm64(big)
    assert np.abs(yb - ref).max() <= 0.05
    assert np.abs(yb.astype(np.float64).std(1) - 1.0).max() <= 0.02
    # the order of a lane's sum: half hh owns units with ((u >> 2) & 1) == hh, ascending
    a = rng.standard_normal((1, N)).astype(np.float32)
    for half in (0, 1):
        s = np.float32(0)
        for u in range(N):
            if ((u >> 2) & 1) == half:
                s = np.float32(s + a[0, u])
        assert L.lane_sum(a, half)[0] == s


# ------------------------------------------------------------------------------------------------ spec and layout
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


@pytest.mark.parametrize('mo', [dict(layer_n=True), dict(layer_n=True, layer_n_affine=True),
                                dict(layer_n=True, layer_n_affine=True, rnn_size=256, input_encoding_size=384)],
                         ids=['ln', 'ln_affine', 'ln_affine_wide'])
def test_spec_accepts_layer_n_and_refuses_what_the_engine_refuses(mo):
    from nicnes.config import ExperimentSpec, NotSupported, GREEDY_FITNESS, SAMPLED_FITNESS
    from nicnes.es import ESExperimentSpec
    for f in GREEDY_FITNESS:
        for m in ('', 'SM-PROPORTIONAL'):
            s = ExperimentSpec(_exp(NES, f, safe_mutations=m, **mo))
            assert s.fitness == f and s.mutation == m
    ExperimentSpec(_exp(NES, safe_mutations='SM-VECTOR', safe_mutation_vector='v.pth', **mo))
    kw = ExperimentSpec(_exp(NES, **mo)).engine_kwargs(max_members=4)
    assert kw['layer_n'] is True and kw['layer_n_affine'] is bool(mo.get('layer_n_affine'))
    for f in SAMPLED_FITNESS:
        with pytest.raises(NotSupported, match='layer_n|wider than 128'):
            ExperimentSpec(_exp(NES, f, **mo))
    with pytest.raises(NotSupported, match='SM-G-SUM'):
        ExperimentSpec(_exp(NES, safe_mutations='SM-G-SUM', safe_mutation_underflow=0.01, **mo))
    with pytest.raises(NotSupported):
        ESExperimentSpec(_exp(ES, **mo))


def test_vbn_still_raises_and_affine_alone_is_ignored():
    from nicnes.config import ExperimentSpec, NotSupported
    for mo in (dict(vbn=True), dict(vbn_e=True), dict(vbn_e=True, layer_n=True)):
        with pytest.raises(NotSupported, match='batch norm'):
            ExperimentSpec(_exp(NES, **mo))
    e = _exp(NES)
    e['policy_options']['vbn'] = True
    with pytest.raises(NotSupported, match='batch norm'):
        ExperimentSpec(e)
    kw = ExperimentSpec(_exp(NES, layer_n_affine=True)).engine_kwargs(max_members=4)     # as the reference ignores it
    assert kw['layer_n'] is False and kw['layer_n_affine'] is False
    assert ExperimentSpec(_exp(NES, 'sample', layer_n_affine=True)).fitness == 'sample'


@pytest.mark.parametrize('E,R', [(128, 128), (256, 512)])
def test_param_layout_with_and_without_the_tail(E, R):
    from nicnes import _lib
    Lb = _lib.lib()
    d = O.Dims(vocab_size=67, E=E, R=R, F=128)
    nine = [o for o, _ in d.offsets().values()]

    def cfg(ln, aff):
        return _lib.NicnesConfig(67, E, R, 128, 16, 8, 64, 4, 1 << 21, 0, ln, aff)
    off, off7 = (ctypes.c_int64 * 10)(), (ctypes.c_int64 * 7)()
    for ln, aff in ((0, 0), (1, 0), (0, 1)):                  # no tail: affine without layer_n is ignored
        c = cfg(ln, aff)
        assert Lb.nicnes_param_count(ctypes.byref(c)) == d.D
        assert Lb.nicnes_param_offsets(ctypes.byref(c), off) == 0 and list(off) == nine + [d.D]
        assert Lb.nicnes_param_offsets_ln(ctypes.byref(c), off7) == _lib.ERR_INVALID
    c = cfg(1, 1)
    assert Lb.nicnes_param_count(ctypes.byref(c)) == d.D + 22 * R
    assert Lb.nicnes_param_offsets(ctypes.byref(c), off) == 0 and list(off) == nine + [d.D + 22 * R]
    assert Lb.nicnes_param_offsets_ln(ctypes.byref(c), off7) == 0
    assert list(off7) == L.tail_offsets(d)
    assert list(off7) == [d.D, d.D + 5 * R, d.D + 10 * R, d.D + 15 * R, d.D + 20 * R, d.D + 21 * R, d.D + 22 * R]
    assert Lb.nicnes_param_offsets_ln(None, off7) == _lib.ERR_INVALID
    # positional construction without the new fields leaves them zero
    old = _lib.NicnesConfig(67, E, R, 128, 16, 8, 64, 4, 1 << 21, 0)
    assert (old.layer_n, old.layer_n_affine) == (0, 0)


def test_synthetic_fresh_theta_has_a_neutral_tail():
    import nicnes.synthetic as S
    d9 = S.Dims(67, 128, 256, 128)
    da = S.Dims(67, 128, 256, 128, layer_n=True, layer_n_affine=True)
    assert S.Dims(67, 128, 256, 128, layer_n=False, layer_n_affine=True).D == d9.D      # ignored without layer_n
    assert da.D == d9.D + 22 * 256 and [n for n, _ in da.shapes()][9:] == L.LN_NAMES
    th = S.init_theta(da, 3)
    assert np.array_equal(th[:d9.D], S.init_theta(d9, 3))
    assert np.array_equal(th[d9.D:], L.make_tail(256))                                  # weight 1, bias 0


def test_ln_state_dict_round_trips_through_a_pth(tmp_path):
    from nicnes import nes as N
    d = O.Dims(vocab_size=67, E=128, R=256, F=128)
    cfg = SimpleNamespace(vocab_size=67, input_encoding_size=128, rnn_size=256, fc_feat_size=128, layer_n=1,
                          layer_n_affine=1)
    shapes = N.param_shapes(SimpleNamespace(cfg=cfg))
    names = list(np.load(GOLDEN)['ln_names'])
    assert list(shapes)[:9] == [n for n, _ in d.shapes()] and list(shapes)[9:] == names == N.LN_PARAM_NAMES
    theta = torch.from_numpy(np.concatenate([O.make_theta(d, 3, 4.0, 0.1), L.make_tail(256, 9, 0.1)]))
    assert sum(int(np.prod(v)) for v in shapes.values()) == theta.numel()
    sd = N.state_dict_from_vector(theta, shapes)
    to = L.tail_offsets(d)
    for i, n in enumerate(names):
        assert torch.equal(sd[n], theta[to[i]:to[i + 1]]), n
    assert sd['core.c_ln.weight'].shape == (256,) and sd['core.i2h_ln.bias'].shape == (1280,)
    path = str(tmp_path / 'ln.pth')
    torch.save(sd, path)
    back = N.vector_from_state_dict(torch.load(path, weights_only=True), shapes)
    assert back.dtype == torch.float32 and torch.equal(back, theta)
    # a checkpoint without the tail does not load into an affine engine, and says why
    nine = {k: v for k, v in sd.items() if k not in names}
    with pytest.raises(KeyError, match='layer_n_affine'):
        N.vector_from_state_dict(nine, shapes)
    # without affine the shapes are the nine
    cfg0 = SimpleNamespace(vocab_size=67, input_encoding_size=128, rnn_size=256, fc_feat_size=128, layer_n=1,
                           layer_n_affine=0)
    assert list(N.param_shapes(SimpleNamespace(cfg=cfg0))) == [n for n, _ in d.shapes()]
