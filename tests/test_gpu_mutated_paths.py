"""GPU: the mutated decode (nicnes_set_mutation 'divide' / 'scale') on every path the dispatcher of evaluate_impl can
send it down, against the CPU oracle (O.perturb(..., mutation) + O.decode / O.decode_sample, oracle/cider_ref.py).

Who forms delta' = fp32(sigma z) / s or * s: on the fused greedy path (G = 4, S = 1, no coop, not sampled, no
NICNES_MUT_FULL) the engine materialises it only from logit.weight on, and nicnes_decode_img_mut_kernel /
nicnes_decode_steps_mut_kernel form the image projection's and the embedding rows' part themselves from the
sigma-scaled table at head_idx[member] and the vector (MutHead: "the head path"); on every other path the whole row
is materialised into dbuf and the plain kernels read it through didx. What is crossed here: the head path over two
slabs, over 2 and 4 streams (head_idx shifted per part), with per-member batches, with the exact lse (log-probs, the
greedy_*prob criteria, the batch-exit pass), NICNES_MUT_FULL=1, the materialised rows through fused64, split G = 4 and
G = 2 and coop S = 2 and S = 4, a member_begin other than 0, a change of sigma between evaluates, evaluate_theta under a
mutation, and the sampled modes ('sample' at two rows per image, 'self_critical', 'sc_loss').

The small world: vocab_size 255 (V1 = 256: four full logit stages, coop fits at S = 2 and 4), F = 384 (nK = 3),
seq_length 16, B = 160 (two slabs, the second with 32 valid rows), two batches, members 3..7 of iteration 3 (2 streams:
2 + 3 members, 4 streams: 1, 1, 1, 2), theta the 'wc' kind of tests/test_gpu_dims.py, the mutation vectors of its
_mutation_vector. One case runs once at the default dims (vocabulary 9487, F = 2048: off_log_w at its production size).

Tolerances are the suite's own: tokens equal up to a step the oracle marks fragile (_compare_tokens / _rows_agree),
CIDEr-D fitness (greedy, sample, self_critical) 1e-9 relative to the restatement on the GPU's own tokens, log-probs
1e-5 absolute, the log-prob criteria (greedy_*prob, sc_loss: fp32 elementwise on log-probs) 1e-6 relative on the GPU's
own log-probs and 1e-5 on the oracle's as tests/test_gpu_parity.py and tests/test_gpu_sample.py hold them, GPU against
GPU bit for bit.

Counts of the oracle (CPU), each asserted (test_input_conditions, test_sampled_modes, test_head_path_exact_lse,
test_head_path_default_dims), of the 1600 (member, sign, row) rows of a greedy world, 'divide' / 'scale':
  fragile rows (cap 5 %)                      0 / 0 at sigma, at 2 sigma and on the second batch
  head sensitivity: rows whose tokens change when the image-projection and embedding entries of delta' carry the plain
  fp32(sigma z) instead (bar 10 %)            800 / 1227; slab 0: 644 / 978, slab 1: 156 / 249; per member, of 320:
                                              154 167 156 169 154 / 247 248 242 242 248 (bar: 4 of the 5 members)
  rows that differ between the two batches    320 of 320 for every member, both modes (bar: half)
  rows that differ between sigma and 2 sigma  1560 / 916 (bar 10 %)
  distinct ids                                161 / 125 of 256; no row of these worlds ends before T
  sampled world (3 members, 1920 rows)        1899 / 1902 rows compare through their last step (bar: half)
  second theta of test 4 (END_BIAS)           every rollout ends before T, at steps 7..12 / 7..8; 82 / 50 ids, no
                                              fragile row
  default dims (2 members, 640 rows)          0 fragile rows; 159 of the 160 rows of member 1, sign +, are
                                              head-sensitive"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from oracle import oracle as O                                  # noqa: E402
from oracle import cider_ref as CR                              # noqa: E402
from tests import test_gpu_dims as D                            # noqa: E402  (helpers only: nothing of it is modified)
from tests.test_gpu_parity import _compare_tokens               # noqa: E402
from tests.test_gpu_sample import _rows_agree                   # noqa: E402

NOISE_LEN, SEED, FRAGILE_CAP = D.NOISE_LEN, D.SEED, D.FRAGILE_CAP
DIMS = O.Dims(vocab_size=255, F=384, T=16)
B, T = 160, 16
SLAB = 128                   # rows of a fused slab: rows 128..159 are slab 1 (blockIdx.z == 1)
IT, M0, P = 3, 3, 5          # members 3..7 of iteration 3
SIGMA = 0.01
MEMBER_BATCH = [1, 0, 1, 1, 0]
MODES = ['divide', 'scale']
FC_SEEDS = (260, 261)
P_SAMPLED, RPI = 3, 2
# on logit.bias[0], test 4's second theta: raised in steps of 1.0 on the CPU until every rollout of the oracle ended
# before T (at 4.0 none does; at 5.0 they end at steps 7 to 12, 82 / 50 distinct ids)
END_BIAS = 5.0
CRITERIA = ['greedy_logprob', 'greedy_expprob', 'greedy_linprob', 'greedy_avgprob']

_cache = {}


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _base():
    """theta, the two batches with their references, the one df table (batch 0's) and its scorer."""
    if 'base' not in _cache:
        import nicnes.synthetic as S
        theta = O.make_theta(DIMS, 0, *D.THETAS['wc'])
        fcs, gts = [], []
        df = n = None
        for j, seed in enumerate(FC_SEEDS):
            fc = np.random.Generator(np.random.PCG64(seed)).standard_normal((B, DIMS.F)).astype(np.float32)
            base, _, _ = O.decode(DIMS, theta, fc)
            g, df_j, n_j = S.build_references(base, DIMS.vocab_size, seed=11 + j, df_sets=64, T=T)
            if j == 0:
                df, n = df_j, n_j
            fcs.append(fc)
            gts.append(g)
        _ro(theta, *fcs)
        _cache['base'] = dict(theta=theta, fcs=fcs, gts=gts, df=df, n=n, scorer=CR.CiderDOracle(df, n))
    return _cache['base']


def _vector(mode):
    key = ('vec', mode)
    if key not in _cache:
        _cache[key] = _ro(np.ascontiguousarray(D._mutation_vector(mode, _base()['theta']), np.float32))[0]
    return _cache[key]


def _theta(end_bias=0.0):
    """theta; end_bias > 0: with logit.bias[0] raised, so that whole rollouts end before T."""
    key = ('theta', float(end_bias))
    if key not in _cache:
        th = _base()['theta'].copy()
        th[DIMS.offsets()['logit.bias'][0]] += np.float32(end_bias)
        _cache[key] = _ro(th)[0]
    return _cache[key]


def _delta(member, sigma, mode, head_plain=False, dims=DIMS, vec=None):
    """delta' of a member; head_plain: the mutation only from logit.weight on, the image projection's and the embedding
    rows' entries left as the plain fp32(sigma z) (what a head kernel that ignored the vector would read)."""
    table = D._table()
    idx = D._idx(dims, member, IT)
    vec = _vector(mode) if vec is None else vec
    d = O.member_delta(table, idx, sigma, dims.D, (mode, vec))
    if head_plain:
        j0 = dims.offsets()['logit.weight'][0]
        d = d.copy()
        d[:j0] = O.member_delta(table, idx, sigma, dims.D)[:j0]
    return d


def _greedy(mode, sigma=SIGMA, batch=0, head_plain=False, end_bias=0.0):
    """The oracle's tokens, log-probs and fragile flags [P, 2, B, T] of members M0 .. M0 + P - 1 on a batch; computed
    once, read-only."""
    key = ('greedy', mode, float(sigma), batch, head_plain, float(end_bias))
    if key not in _cache:
        w, theta = _base(), _theta(end_bias)
        oseq = np.zeros((P, 2, B, T), np.int32)
        olp = np.zeros((P, 2, B, T), np.float32)
        ofr = np.zeros((P, 2, B, T), np.uint8)
        for k in range(P):
            d = _delta(M0 + k, sigma, mode, head_plain)
            for s in range(2):
                th = (theta + d) if s == 0 else (theta - d)
                oseq[k, s], olp[k, s], ofr[k, s] = O.decode(DIMS, th, w['fcs'][batch])
        _cache[key] = _ro(oseq, olp, ofr)
    return _cache[key]


def _oracle_scores(mode, sigma, batch, k, s):
    """CIDEr-D row scores of the oracle's own tokens of one rollout (the restatement is run once per rollout; a GPU
    rollout whose tokens equal the oracle's on every row is scored by it)."""
    key = ('scores', mode, float(sigma), batch, k, s)
    if key not in _cache:
        w = _base()
        _cache[key] = CR.rollout_fitness(w['scorer'], _greedy(mode, sigma, batch)[0][k, s], w['gts'][batch])
    return _cache[key]


def _restated(seq_ks, mode, sigma, batch, k, s):
    """(fitness, row scores) of the CIDEr-D restatement on the GPU's own tokens seq_ks [B, T]."""
    if np.array_equal(seq_ks, _greedy(mode, sigma, batch)[0][k, s]):
        return _oracle_scores(mode, sigma, batch, k, s)
    w = _base()
    return CR.rollout_fitness(w['scorer'], seq_ks, w['gts'][batch])


def _check_greedy(fit, seq, mode, sigma=SIGMA, batches=None, tag=''):
    """tokens of every member and sign against the oracle up to a fragile step, fitness against the restatement on the
    GPU's tokens; batches: each member's batch (None: batch 0)."""
    assert seq.shape == (P, 2, B, T) and fit.shape == (P, 2)
    for k in range(P):
        b = batches[k] if batches is not None else 0
        oseq, _, ofr = _greedy(mode, sigma, b)
        for s in range(2):
            assert _compare_tokens(seq[k, s], oseq[k, s], ofr[k, s]) == 0, (tag, k, s)
            f_ref, _ = _restated(seq[k, s], mode, sigma, b, k, s)
            assert D._close(fit[k, s], f_ref), (tag, k, s, fit[k, s], f_ref)
    assert fit.max() > 0.0


def _diff_rows(a, b):
    """[.., B] rows whose tokens differ"""
    return (a != b).any(-1)


def input_counts(mode):
    """The conditions on the inputs, from the oracle alone (no GPU): a dict of the counts the module's docstring
    records. Asserted by test_input_conditions."""
    oseq, _, ofr = _greedy(mode)
    frag = ofr.any(-1)
    out = {'rows': int(frag.size), 'fragile': int(frag.sum())}
    for name, kw in (('2sigma', dict(sigma=2 * SIGMA)), ('batch1', dict(batch=1))):
        out['fragile_' + name] = int(_greedy(mode, **kw)[2].any(-1).sum())
    head = _diff_rows(oseq, _greedy(mode, head_plain=True)[0])           # [P, 2, B]
    out['head_rows'] = int(head.sum())
    out['head_slab0'] = int(head[..., :SLAB].sum())
    out['head_slab1'] = int(head[..., SLAB:].sum())
    out['head_per_member'] = [int(head[k].sum()) for k in range(P)]
    other = _diff_rows(oseq, _greedy(mode, batch=1)[0])
    out['batch_rows_per_member'] = [int(other[k].sum()) for k in range(P)]
    out['sigma_rows'] = int(_diff_rows(oseq, _greedy(mode, sigma=2 * SIGMA)[0]).sum())
    out['distinct_ids'] = int(np.unique(oseq).size)
    return out


# ---------------------------------------------------------------------------------------- engines
@pytest.fixture(scope='module')
def engines():
    """'head': the engine as it runs by default; 'full': one created under NICNES_MUT_FULL=1 (read at create). Both pin
    the pair-bounded lse as tests/test_gpu_dims.py does: greedy-only decodes run the PAIRS instantiations, log-prob
    decodes the exact ones."""
    import nicnes
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    made = {}

    def get(kind):
        if kind not in made:
            mp = pytest.MonkeyPatch()
            mp.setenv('NICNES_BOUNDED_LSE', '1')
            mp.delenv('NICNES_MUT_FULL', raising=False)
            if kind == 'full':
                mp.setenv('NICNES_MUT_FULL', '1')
            try:
                e = nicnes.Engine(vocab_size=DIMS.vocab_size, fc_feat_size=DIMS.F, seq_length=T, max_batch=B,
                                  max_members=8, noise_len=NOISE_LEN, noise_seed=SEED)
            finally:
                mp.undo()
            e.set_noise_table(D._table())
            assert e.D == DIMS.D
            w = _base()
            D._load(e, w['theta'].copy(), w['fcs'][0], w['gts'][0], w['df'], w['n'])
            made[kind] = e
        return made[kind]
    yield get
    for e in made.values():
        e.close()


def _reset(e):
    w = _base()
    D._reset(e)
    e.set_theta(w['theta'].copy())              # (copies: torch warns about read-only arrays)
    e.set_decode_streams(0)
    e.set_rows_per_image(1)
    e.set_batch(w['fcs'][0], w['gts'][0])


def _no_faults(e):
    st = e.stats()
    assert st['coop_timeouts'] == 0 and st['sample_slot_timeouts'] == 0 and st['queue_timeouts'] == 0, st


def _head_setting(e, mode, streams=0):
    e.set_decode_split(1, 4)
    e.set_decode_coop(0)
    e.set_decode_streams(streams)
    e.set_mutation(mode, _vector(mode).copy())
    assert e.decode_path(B, P) == 'fused' and e.decode_shape(B, P) == (4, 2, 1)


def _evaluate(e, sigma=SIGMA, **kw):
    out = e.evaluate(IT, M0, P, sigma, return_seq=True, **kw)
    return tuple(x.cpu().numpy() for x in out)


def _head_output(engines, mode):
    """(fitness, tokens) of the head path on one stream: what test 1 checks against the oracle and tests 2, 3 and 8
    compare with bit for bit. Run once per mode."""
    key = ('gpu_head', mode)
    if key not in _cache:
        e = engines('head')
        try:
            _head_setting(e, mode)
            _cache[key] = _ro(*_evaluate(e))
        finally:
            _reset(e)
    return _cache[key]


def _same_bits(got, want, tag):
    assert np.array_equal(got[1], want[1]), tag
    assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)), tag


# ---------------------------------------------------------------------------------------- 0. the inputs
@pytest.mark.parametrize('mode', MODES)
def test_input_conditions(mode):
    """What makes the tests below bite, from the oracle alone: few fragile rows in every greedy world; the tokens
    depend on the head part of delta' (a decode whose image-projection and embedding entries carry the plain
    fp32(sigma z) differs in >= 10 % of the rows, in both slabs and for >= 4 of the 5 members: a head kernel that
    dropped the vector fails); the two batches decode differently; sigma and 2 sigma decode differently."""
    c = input_counts(mode)
    print(mode, c)
    rows = c['rows']
    assert rows == P * 2 * B
    for key in ('fragile', 'fragile_2sigma', 'fragile_batch1'):
        assert c[key] <= FRAGILE_CAP * rows, (key, c)
    assert 10 * c['head_rows'] >= rows, c
    assert c['head_slab0'] > 0 and c['head_slab1'] > 0, c
    assert sum(1 for v in c['head_per_member'] if v > 0) >= 4, c
    assert all(2 * v >= 2 * B for v in c['batch_rows_per_member']), c
    assert 10 * c['sigma_rows'] >= rows, c
    assert c['distinct_ids'] >= 20, c


# ---------------------------------------------------------------------------------------- 1. head path, two slabs
@pytest.mark.parametrize('mode', MODES)
def test_head_path_two_slabs(engines, mode):
    """(1, 4), coop off, one stream, member_begin 3: the head kernels over dim3(1, members, 2) with the lane's fc row in
    slab 1. Tokens and fitness of 5 members x 2 signs against the oracle; noise_vectors = O.member_delta bit for bit;
    grad_partial = the fp64 member-order sum rounded once."""
    e = engines('head')
    fit, seq = _head_output(engines, mode)
    _check_greedy(fit, seq, mode, tag='head')
    try:
        e.set_mutation(mode, _vector(mode).copy())
        idx = [int(i) for i in e.noise_indices(IT, M0, P).cpu().numpy()]
        assert idx == [D._idx(DIMS, M0 + k, IT) for k in range(P)]
        dv = e.noise_vectors(IT, M0, P, SIGMA).cpu().numpy()
        w_np = np.linspace(-0.5, 0.5, P).astype(np.float32)
        acc = np.zeros(DIMS.D, np.float64)
        for k in range(P):
            want = _delta(M0 + k, SIGMA, mode)
            assert np.array_equal(dv[k].view(np.uint32), want.view(np.uint32)), k
            assert not np.array_equal(want, _delta(M0 + k, SIGMA, mode, head_plain=True))
            acc += np.float64(w_np[k]) * want.astype(np.float64)
        g = e.grad_partial(IT, M0, P, torch.from_numpy(w_np).to(e.device), SIGMA).cpu().numpy()
        assert np.array_equal(g.view(np.uint32), acc.astype(np.float32).view(np.uint32))
        _no_faults(e)
    finally:
        _reset(e)


# ---------------------------------------------------------------------------------------- 2. head path over streams
@pytest.mark.parametrize('streams', [2, 4])
@pytest.mark.parametrize('mode', MODES)
def test_head_path_over_streams(engines, mode, streams):
    """nicnes_decode_shift's head_idx += m0: the members in 2 + 3 and in 1, 1, 1, 2 parts. The same bits as one stream;
    two streams also against the oracle itself."""
    e = engines('head')
    want = _head_output(engines, mode)
    try:
        _head_setting(e, mode, streams)
        got = _evaluate(e)
        if streams == 2:
            _check_greedy(got[0], got[1], mode, tag='2 streams')
        _same_bits(got, want, streams)
        _no_faults(e)
    finally:
        _reset(e)


# ---------------------------------------------------------------------------------------- 3. NICNES_MUT_FULL=1
@pytest.mark.parametrize('streams', [1, 2])
@pytest.mark.parametrize('mode', MODES)
def test_mut_full_engine(engines, mode, streams):
    """An engine created under NICNES_MUT_FULL=1 materialises every row and runs the plain fused kernels on the same
    shape: the oracle's tokens, and the head path's tokens and fitness bit for bit."""
    e = engines('full')
    want = _head_output(engines, mode)
    try:
        _head_setting(e, mode, streams)
        got = _evaluate(e)
        _check_greedy(got[0], got[1], mode, tag='full')
        _same_bits(got, want, streams)
        _no_faults(e)
    finally:
        _reset(e)


# ---------------------------------------------------------------------------------------- 4. exact lse on the head path
def _check_logprobs(seq, lp, mode, tag='', end_bias=0.0):
    oseq, olp, ofr = _greedy(mode, end_bias=end_bias)
    assert lp.shape == (P, 2, B, T) and np.isfinite(lp).all() and (lp <= 0).all()
    for k in range(P):
        for s in range(2):
            assert _compare_tokens(seq[k, s], oseq[k, s], ofr[k, s]) == 0, (tag, k, s)
            keep = ~ofr[k, s].any(-1)
            m = np.concatenate([np.ones((B, 1), bool), oseq[k, s][:, :-1] > 0], 1) & keep[:, None]
            err = np.abs(lp[k, s][m] - olp[k, s][m]).max()
            assert err <= 1e-5, (tag, k, s, err)
            if keep.all():                                 # steps after the rollout's last finishing one read 0
                ends = np.where((oseq[k, s] == 0).any(1), (oseq[k, s] == 0).argmax(1) + 1, T)
                assert (lp[k, s][:, ends.max():] == 0).all(), (tag, k, s)


@pytest.mark.parametrize('mode', MODES)
def test_head_path_exact_lse(engines, mode):
    """return_lp selects nicnes_decode_steps_mut_kernel<false> and, with two slabs, no_exit and the batch-exit pass:
    tokens and log-probs against the oracle, 0 after a rollout's last finishing step; on one and two streams."""
    e = engines('head')
    want = _head_output(engines, mode)
    try:
        first = None
        for streams in (1, 2):
            _head_setting(e, mode, streams)
            fit, seq, lp = _evaluate(e, return_lp=True)
            _same_bits((fit, seq), want, streams)
            _check_logprobs(seq, lp, mode, streams)
            if first is None:
                first = lp
            assert np.array_equal(lp.view(np.uint32), first.view(np.uint32)), streams
        # every rollout of this world has rows that run to T, so the zeros above are checked on no step. A second theta
        # whose rollouts all end before T, each at its own step: the batch-exit pass zeroes what the slabs, which ran
        # to T (no_exit), wrote after it
        oseq, _, ofr = _greedy(mode, end_bias=END_BIAS)
        ends = np.where((oseq == 0).any(-1), (oseq == 0).argmax(-1) + 1, T).max(-1)          # [P, 2]
        assert (ends < T).all() and np.unique(ends).size >= 2 and not ofr.any(), ends
        assert np.unique(oseq).size >= 20
        e.set_theta(_theta(END_BIAS).copy())
        for streams in (1, 2):
            _head_setting(e, mode, streams)
            _, seq, lp = _evaluate(e, return_lp=True)
            _check_logprobs(seq, lp, mode, ('ending theta', streams), END_BIAS)
        _no_faults(e)
    finally:
        _reset(e)


@pytest.mark.parametrize('crit', CRITERIA)
def test_head_path_logprob_criteria(engines, crit):
    """The greedy_*prob criteria ('divide') run the exact-lse head kernels into the engine's own log-prob buffer:
    fitness against oracle/cider_ref.py's criterion on the GPU's log-probs (1e-6) and on the oracle's tokens and
    log-probs (1e-5), the bounds of tests/test_gpu_parity.py::test_fitness_criteria_match_oracle."""
    mode = 'divide'
    e = engines('head')
    oseq, olp, ofr = _greedy(mode)
    try:
        _head_setting(e, mode)
        e.set_fitness_mode(crit)
        fit, seq, lp = _evaluate(e, return_lp=True)
        fit_own = e.evaluate(IT, M0, P, SIGMA).cpu().numpy()
        assert np.array_equal(fit_own.view(np.uint64), fit.view(np.uint64))      # the engine's buffer == the caller's
        _check_logprobs(seq, lp, mode, crit)
        worst = [0.0, 0.0]
        for k in range(P):
            for s in range(2):
                _, scores = _restated(seq[k, s], mode, SIGMA, 0, k, s)
                f_own = CR.criterion_fitness(crit, lp[k, s], seq[k, s], scores)
                worst[0] = max(worst[0], abs(fit[k, s] - f_own) / max(1.0, abs(f_own)))
                assert abs(fit[k, s] - f_own) <= 1e-6 * max(1.0, abs(f_own)), (k, s, fit[k, s], f_own)
                if not ofr[k, s].any():
                    f_ora = CR.criterion_fitness(crit, olp[k, s], oseq[k, s], scores)
                    worst[1] = max(worst[1], abs(fit[k, s] - f_ora) / max(1.0, abs(f_ora)))
                    assert abs(fit[k, s] - f_ora) <= 1e-5 * max(1.0, abs(f_ora)), (k, s, fit[k, s], f_ora)
        print(crit, 'worst relative error: own log-probs %.3g, oracle log-probs %.3g' % tuple(worst))
        assert np.abs(fit).max() > 0.0
        _no_faults(e)
    finally:
        _reset(e)


# ---------------------------------------------------------------------------------------- 5. materialised paths
# name: (S, G, coop), the path nicnes_decode_path reports, slabs of B = 160
MATERIALISED = {'fused64': (1, 2, 1, 'fused', 3), 'split_G4': (4, 4, 0, 'split', 2), 'split_G2': (4, 2, 0, 'split', 3),
                'coop_S2': (2, 4, 1, 'coop', 2), 'coop_S4': (4, 4, 1, 'coop', 2)}


@pytest.mark.parametrize('path', list(MATERIALISED))
@pytest.mark.parametrize('mode', MODES)
def test_materialised_paths(engines, mode, path):
    """The whole delta' row in dbuf, read through didx by the plain kernels: the 64-row fused kernel, the split path at
    G = 4 and G = 2 (two streams by default: didx shifted) and the coop kernels at S = 2 and S = 4."""
    S, G, coop, want_path, slabs = MATERIALISED[path]
    e = engines('head')
    try:
        e.set_decode_split(S, G)
        e.set_decode_coop(coop)
        e.set_mutation(mode, _vector(mode).copy())
        assert e.decode_path(B, P) == want_path, (path, e.decode_path(B, P))
        assert e.decode_shape(B, P) == (G, slabs, S), (path, e.decode_shape(B, P))
        fit, seq = _evaluate(e)
        _check_greedy(fit, seq, mode, tag=path)
        _same_bits((fit, seq), _head_output(engines, mode), path)
        _no_faults(e)
    finally:
        _reset(e)


# ---------------------------------------------------------------------------------------- 6. per-member batches
@pytest.mark.parametrize('path', ['head_1_stream', 'head_2_streams', 'coop_S2'])
@pytest.mark.parametrize('mode', MODES)
def test_per_member_batches(engines, mode, path):
    """set_batches of two batches, member_batch = [1, 0, 1, 1, 0]: p.member_batch[c.member] inside
    nicnes_decode_img_mut_kernel (shifted with the members on two streams), and the coop kernels on materialised rows.
    Every member against the oracle decode of its own batch, scored against its own batch's references."""
    w = _base()
    e = engines('head')
    try:
        e.set_batches(list(zip(w['fcs'], w['gts'])))
        if path == 'coop_S2':
            e.set_decode_split(2, 4)
            e.set_decode_coop(1)
            e.set_mutation(mode, _vector(mode).copy())
            assert e.decode_path(B, P) == 'coop'
        else:
            _head_setting(e, mode, 2 if path == 'head_2_streams' else 1)
        fit, seq = _evaluate(e, member_batch=MEMBER_BATCH)
        _check_greedy(fit, seq, mode, batches=MEMBER_BATCH, tag=path)
        _no_faults(e)
    finally:
        _reset(e)


# ---------------------------------------------------------------------------------------- 7. sigma sequence
@pytest.mark.parametrize('kind', ['head', 'full'])
@pytest.mark.parametrize('mode', MODES)
def test_sigma_sequence(engines, mode, kind):
    """sigma, 2 sigma, sigma on one engine: the head kernels read the table scaled by ensure_noise_scaled, the
    materialised part is scaled in nicnes_launch_mutate; a stale scaled table would make the halves of one delta'
    disagree. Each evaluate matches its oracle world and the third equals the first bit for bit; the same on the
    NICNES_MUT_FULL=1 engine."""
    e = engines(kind)
    try:
        _head_setting(e, mode)
        runs = []
        for sigma in (SIGMA, 2 * SIGMA, SIGMA):
            fit, seq = _evaluate(e, sigma)
            _check_greedy(fit, seq, mode, sigma, tag=(kind, sigma))
            runs.append((fit, seq))
        _same_bits(runs[2], runs[0], kind)
        _same_bits(runs[0], _head_output(engines, mode), kind)
        assert not np.array_equal(runs[1][1], runs[0][1])
        dv = e.noise_vectors(IT, M0, 1, 2 * SIGMA).cpu().numpy()
        assert np.array_equal(dv[0].view(np.uint32), _delta(M0, 2 * SIGMA, mode).view(np.uint32))
        _same_bits(_evaluate(e), runs[0], (kind, 'after noise_vectors at 2 sigma'))
        _no_faults(e)
    finally:
        _reset(e)


# ---------------------------------------------------------------------------------------- 8. theta itself
@pytest.mark.parametrize('mode', MODES)
def test_theta_itself_under_a_mutation(engines, mode):
    """evaluate_theta ignores the mutation: tokens, log-probs and fitness are the same bits with the mutation set and
    after set_mutation('plain'), on the fused and the screened fused setting (without log-probs the screened loop really
    runs: its counters move); they are the oracle's decode of theta; a mutated evaluate right after still gives test
    1's bits."""
    w = _base()
    e = engines('head')
    want = _head_output(engines, mode)
    base, _, base_fr = O.decode(DIMS, w['theta'], w['fcs'][0])
    try:
        for screen in (0, 1):
            e.set_decode_split(1, 4)
            e.set_decode_coop(1)
            e.set_decode_screen(screen)
            got = {}
            for mut in (mode, 'plain', mode):
                e.set_mutation(*((mut, _vector(mut).copy()) if mut != 'plain' else ('plain',)))
                before = e.stats()
                f0, s0 = e.evaluate_theta(0, return_seq=True)
                after = e.stats()
                moved = (after['screen_candidates'] + after['screen_fallback_rows']
                         - before['screen_candidates'] - before['screen_fallback_rows'])
                assert (moved > 0) == bool(screen), (screen, mut, moved)
                f1, s1, l1 = e.evaluate_theta(0, return_seq=True, return_lp=True)
                out = [x.cpu().numpy() for x in (f0, s0, f1, s1, l1)]
                assert out[1].shape == (B, T)
                if not got:
                    got = out
                    assert _compare_tokens(out[1], base, base_fr) == 0
                    f_ref, _ = CR.rollout_fitness(w['scorer'], out[1], w['gts'][0])
                    assert D._close(out[0][0], f_ref), (out[0], f_ref)
                for a, b in zip(out, got):
                    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (screen, mut)
            # the mutation is set again: the members' decode (never screened under a mutation) is test 1's
            e.set_decode_coop(0)
            _same_bits(_evaluate(e), want, screen)
        _no_faults(e)
    finally:
        _reset(e)


# ---------------------------------------------------------------------------------------- 9. sampled modes
def _sampled_world(mode):
    """Three members, two rows per image (320 rows, three slabs): the engine's own draws restated by O.sample_draws and
    the oracle's sampled decode of theta +- delta'."""
    key = ('sampled', mode)
    if key not in _cache:
        w = _base()
        rows = B * RPI
        u = O.sample_draws(SEED, IT, M0, P_SAMPLED, rows, T)
        fc_rows = np.repeat(w['fcs'][0], RPI, 0)
        oseq = np.zeros((P_SAMPLED, 2, rows, T), np.int32)
        ofr = np.zeros((P_SAMPLED, 2, rows, T), bool)
        for k in range(P_SAMPLED):
            d = _delta(M0 + k, SIGMA, mode)
            for s in range(2):
                th = (w['theta'] + d) if s == 0 else (w['theta'] - d)
                sq, _, fr = O.decode_sample(DIMS, th, fc_rows, u[k, s])
                oseq[k, s], ofr[k, s] = sq, fr != 0
        _cache[key] = _ro(u, oseq, ofr)
    return _cache[key]


@pytest.mark.parametrize('mode', MODES)
def test_sampled_modes(engines, mode):
    """The sampled pass materialises the whole row (its kernels take no MutHead). 'sample' at two rows per image:
    tokens against O.decode_sample up to the first fragile draw, fitness against the restatement on the GPU's rows.
    'self_critical' / 'sc_loss': their greedy baseline pass goes down the head path (dbuf written from off[3] on), the
    sampled pass of the same call rewrites the whole row: the same sampled rows, fitness = the restatement built from
    the greedy baseline's and the sampled rows' scores. 'sample' over two streams (1 + 2 members) gives the bits of one
    stream: nicnes_decode_shift moves the draws with the members (it did not: the second part drew with the first
    members' uniforms). The greedy head path afterwards still gives test 1's bits."""
    w = _base()
    e = engines('head')
    u, oseq, ofr = _sampled_world(mode)
    whole = int((~ofr.any(-1)).sum())
    print(mode, 'sampled rows compared through their last step: %d of %d' % (whole, ofr[..., 0].size))
    assert 2 * whole >= ofr[..., 0].size, whole
    assert np.unique(oseq).size >= 20
    want = _head_output(engines, mode)
    n, rows = P_SAMPLED, B * RPI
    out = {}
    try:
        _head_setting(e, mode)
        e.set_rows_per_image(RPI)
        e.set_sample_draws(u)
        for fm in ('greedy', 'sample', 'self_critical', 'sc_loss'):
            e.set_fitness_mode(fm)
            out[fm] = tuple(x.cpu().numpy() for x in e.evaluate(IT, M0, n, SIGMA, return_seq=True,
                                                               return_lp=(fm == 'sc_loss')))
        # the members in 1 + 2 parts on two streams: every part reads its own members' draws and delta' rows
        e.set_decode_streams(2)
        e.set_fitness_mode('sample')
        out['sample_2_streams'] = tuple(x.cpu().numpy() for x in e.evaluate(IT, M0, n, SIGMA, return_seq=True))
        e.set_decode_streams(1)
        e.set_fitness_mode('greedy')
        e.set_sample_draws(None)
        e.set_rows_per_image(1)
        _same_bits(_evaluate(e), want, 'greedy after the sampled modes')
        _no_faults(e)
    finally:
        _reset(e)
    fg, sg = out['greedy']
    fs, ss = out['sample']
    fsc, ssc = out['self_critical']
    fl, sl, lpl = out['sc_loss']
    assert sg.shape == (n, 2, B, T) and ss.shape == (n, 2, rows, T)
    _same_bits((fg, sg), (want[0][:n], want[1][:n]), 'greedy baseline')
    assert np.array_equal(ss, ssc) and np.array_equal(ss, sl)              # the same draws, the same samples
    _same_bits(out['sample_2_streams'], (fs, ss), 'sample on two streams')
    assert np.allclose(fsc, fs - fg, rtol=0, atol=1e-9), (fsc, fs - fg)
    for k in range(n):
        for s in range(2):
            _rows_agree(ss[k, s], oseq[k, s], ofr[k, s])
            f_s, sc_s = CR.rollout_fitness(w['scorer'], ss[k, s], w['gts'][0], RPI)
            assert D._close(fs[k, s], f_s), (k, s, fs[k, s], f_s)
            _, sc_g = _restated(sg[k, s], mode, SIGMA, 0, k, s)
            reward = np.asarray(sc_s) - np.repeat(np.asarray(sc_g), RPI)
            assert D._close(fsc[k, s], 100.0 * reward.mean()), (k, s, fsc[k, s], 100.0 * reward.mean())
            f_l = CR.criterion_fitness('sc_loss', lpl[k, s], sl[k, s], reward)
            assert abs(fl[k, s] - f_l) <= 1e-6 * max(1.0, abs(f_l)), (k, s, fl[k, s], f_l)
    assert fs.max() > 0.0


# ---------------------------------------------------------------------------------------- 10. default dims, once
def test_head_path_default_dims():
    """Engine()'s default vocabulary and F ('scale', B = 160, members 1 and 2, two streams): the one case where
    off_log_w, and with it the head / materialised split of a row and the 4 * off_log_w buffer range of the head
    kernels, has its production size."""
    import nicnes
    import nicnes.synthetic as S
    dims, table = O.Dims(), D._table()
    theta = O.make_theta(dims, 0, *D.THETAS['wc'])
    fc = np.random.Generator(np.random.PCG64(FC_SEEDS[0])).standard_normal((B, dims.F)).astype(np.float32)
    base, _, _ = O.decode(dims, theta, fc)
    gts, df, n = S.build_references(base, dims.vocab_size, seed=11, df_sets=64, T=T)
    scorer = CR.CiderDOracle(df, n)
    vec = D._mutation_vector('scale', theta)
    m0, cnt = 1, 2
    mp = pytest.MonkeyPatch()
    mp.setenv('NICNES_BOUNDED_LSE', '1')
    mp.delenv('NICNES_MUT_FULL', raising=False)
    try:
        e = nicnes.Engine(max_batch=B, max_members=8, noise_len=NOISE_LEN, noise_seed=SEED)
    finally:
        mp.undo()
    try:
        e.set_noise_table(table)
        D._load(e, theta, fc, gts, df, n)
        e.set_decode_split(1, 4)
        e.set_decode_coop(0)
        e.set_decode_streams(2)
        e.set_mutation('scale', vec)
        assert e.decode_path(B, cnt) == 'fused'
        fit, seq = e.evaluate(IT, m0, cnt, SIGMA, return_seq=True)
        fit, seq = fit.cpu().numpy(), seq.cpu().numpy()
        cut = head = 0
        for k in range(cnt):
            d = _delta(m0 + k, SIGMA, 'scale', dims=dims, vec=vec)
            d_plain = _delta(m0 + k, SIGMA, 'scale', True, dims=dims, vec=vec)
            for s in range(2):
                oseq, _, fr = O.decode(dims, (theta + d) if s == 0 else (theta - d), fc)
                if k == 0 and s == 0:       # the head part matters here too
                    head = int(_diff_rows(oseq, O.decode(dims, theta + d_plain, fc)[0]).sum())
                assert _compare_tokens(seq[k, s], oseq, fr) == 0, (k, s)
                cut += int(fr.any(1).sum())
                f_ref, _ = CR.rollout_fitness(scorer, seq[k, s], gts)
                assert D._close(fit[k, s], f_ref), (k, s, fit[k, s], f_ref)
        print('default dims: fragile rows %d of %d, head-sensitive rows of member 1 sign + %d of %d'
              % (cut, cnt * 2 * B, head, B))
        assert cut <= FRAGILE_CAP * cnt * 2 * B, cut
        assert 10 * head >= B, head
        _no_faults(e)
    finally:
        e.close()
