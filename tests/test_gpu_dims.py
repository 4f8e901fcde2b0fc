"""GPU: every decode path, the sampled, mutated, theta-itself and ES decodes, the update kernels and the sensitivity away
from the default fc_feat_size = 2048, seq_length = 16 and vocabulary, at the edges include/nicnes.h promises
(F any multiple of 128, seq_length 1..16, V1 = vocab_size + 1 in 8..16384 with V1 % 4 == 0), against the CPU oracle.

What each dimension reaches in the kernels: F sets nK = F / 128, the trip count of the hand-pipelined image-projection
loops (nK = 1 has no steady state, odd nK ends on the other buffer) and moves every later tensor offset inside theta;
seq_length bounds every step loop and is the row stride of the token, log-prob and draw arrays; V1 sets
nst = ceil(V1 / 64) logit stages, which the split path divides over S workgroups (empty ranges when nst < S, where the
coop path must refuse) and whose last stage may be 4 to 64 columns wide.

The cases (B and T are the test shapes):
  a  V1 8      F 128   T 16  B 40    one stage 8 columns wide, nK = 1, D % 64 = 8
  b  V1 8      F 128   T 1   B 40    one logit step: every `t < T` guard at its edge
  c  V1 60     F 128   T 7   B 130   one stage with a 60-column tail, two slabs with a 2-row tail, rows ending before T
  d  V1 68     F 384   T 16  B 40    two stages, the second 4 columns wide, odd nK = 3, D % 64 = 4
  e  V1 128    F 640   T 16  B 40    two full stages: coop fits at S = 2 and not at S = 4, nK = 5
  f  V1 9488   F 128   T 7   B 40    the workload's vocabulary with nK = 1
  g  V1 9488   F 384   T 1   B 130   the same with T = 1 over two slabs
  h  V1 9488   F 4096  T 16  B 40    nK = 32: fc and img_w byte offsets beyond the default's
  i  V1 16384  F 128   T 3   B 40    the largest vocabulary (nst = 256); id 16383 from a decode into the scorer's keys
  j  V1 16380  F 256   T 3   B 40    a 60-column tail at the largest stage count

Tolerances are the suite's own: tokens bit-exact up to a step the oracle marks fragile, CIDEr-D fitness 1e-9 relative,
log-probs 1e-5 absolute (tests/test_gpu_parity.py), the sensitivity bar of tests/test_gpu_mutations.py; everything else
bit for bit. The update ratio is an fp64 sum of at most 4.4 M non-negative terms in another order than numpy's:
n * 2^-53 = 5e-10 bounds its relative error, checked at 1e-9.

Counts of the oracle (CPU): none of the 240 (780 in cases c and g) (member, sign, row) rows of a greedy world, either
theta kind, is marked fragile (cap: 5 %), nor any row of the mutated and ES worlds; the sampled worlds compare 160, 160
and 141 of their 160 rows through the last step (cases b, d, i; bar: half). Distinct ids over a greedy world: a 7 of 8,
b 8 of 8, d 43, e 83, f 200, g 243, h 265, i 161, j 190 (xavier: a 7, d 34, f 196); case c ends 345 of 780 rows before T."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from oracle import oracle as O                                  # noqa: E402
from oracle import cider_ref as CR                              # noqa: E402
from tests import es_ref as R                                   # noqa: E402
from tests import test_gpu_es as E                              # noqa: E402  (helpers only: nothing of it is modified)
from tests.test_gpu_eval_theta import PATHS                     # noqa: E402
from tests.test_gpu_mutations import _sens_close                # noqa: E402
from tests.test_gpu_parity import _compare_tokens               # noqa: E402
from tests.test_gpu_sample import _rows_agree                   # noqa: E402

NOISE_LEN = 1 << 23          # D reaches 4.41 M at V = 16383
SEED = 7
SIGMA = 0.01
IT = 3
P = 3                        # members of the greedy worlds (odd)
FRAGILE_CAP = 0.05           # share of (member, sign, row) rows the oracle's fragile flag may cut short

CASES = {
    'a': dict(vocab=7, F=128, T=16, B=40),
    'b': dict(vocab=7, F=128, T=1, B=40, fc_seed=240),
    'c': dict(vocab=59, F=128, T=7, B=130),
    'd': dict(vocab=67, F=384, T=16, B=40),
    'e': dict(vocab=127, F=640, T=16, B=40),
    'f': dict(vocab=9487, F=128, T=7, B=40),
    'g': dict(vocab=9487, F=384, T=1, B=130),
    'h': dict(vocab=9487, F=4096, T=16, B=40),
    'i': dict(vocab=16383, F=128, T=3, B=40),
    'j': dict(vocab=16379, F=256, T=3, B=40),
}
THETAS = {'wc': (4.0, 0.1), 'xavier': (1.0, 0.0)}
GREEDY_WORLDS = [(c, 'wc') for c in CASES] + [(c, 'xavier') for c in ('a', 'd', 'f')]
# case i: logit.bias[16383] raised in steps of 0.1 on the CPU until every rollout of the oracle held id 16383 in several
# of its rows (6 to 13 of 40 at 0.5, 161 distinct ids left; at 1.0 nearly every token is 16383); asserted in the test
TOP_ID_BIAS = 0.5

# name: (S, G, coop, screen) as nicnes_set_decode_split / _coop / _screen take them
GREEDY_PATHS = {'fused': (1, 4, 1, 0), 'fused_screened': (1, 4, 1, 1), 'fused64': (1, 2, 1, 0), 'split_G4': (4, 4, 0, 0),
                'split_G2': (4, 2, 0, 0), 'coop_S4': (4, 4, 1, 0), 'coop_S2': (2, 4, 1, 0)}

_cache = {}


def _dims(case):
    c = CASES[case]
    return O.Dims(vocab_size=c['vocab'], F=c['F'], T=c['T'])


def _table():
    if 'table' not in _cache:
        _cache['table'] = O.noise_table(NOISE_LEN, 123)
    return _cache['table']


def _theta(case, kind='wc'):
    dims = _dims(case)
    theta = O.make_theta(dims, 0, *THETAS[kind])
    if case == 'i':
        theta[dims.offsets()['logit.bias'][0] + dims.vocab_size] += np.float32(TOP_ID_BIAS)
    return theta


def _fc(case):
    c = CASES[case]
    # seed 100 + B; case b: 240, since with 140 the one step of its 240 rows takes only 6 of the 8 ids (with 240: all 8)
    seed = c.get('fc_seed', 100 + c['B'])
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((c['B'], c['F'])).astype(np.float32)


def _idx(dims, member, iteration=IT):
    return O.noise_index(SEED, iteration, member, NOISE_LEN, dims.D)


def _references(dims, theta, fc, seed):
    import nicnes.synthetic as S
    base, _, _ = O.decode(dims, theta, fc)
    gts, df, n = S.build_references(base, dims.vocab_size, seed=seed, df_sets=64, T=dims.T)
    return base, gts, df, n


def _world(case, kind='wc'):
    """The oracle's side of a greedy world, computed once and never modified: theta, the batch, its references, and the
    tokens / log-probs / fragile flags of P members x 2 signs."""
    key = ('world', case, kind)
    if key not in _cache:
        dims, theta, fc, table = _dims(case), _theta(case, kind), _fc(case), _table()
        base, gts, df, n = _references(dims, theta, fc, 11)
        B = fc.shape[0]
        oseq = np.zeros((P, 2, B, dims.T), np.int32)
        olp = np.zeros((P, 2, B, dims.T), np.float32)
        ofr = np.zeros((P, 2, B, dims.T), np.uint8)
        for k in range(P):
            for s, sign in enumerate((+1, -1)):
                oseq[k, s], olp[k, s], ofr[k, s] = O.decode(dims, O.perturb(theta, table, _idx(dims, k), SIGMA, sign), fc)
        for a in (base, oseq, olp, ofr):
            a.setflags(write=False)
        _cache[key] = dict(dims=dims, theta=theta, fc=fc, base=base, gts=gts, df=df, n=n, oseq=oseq, olp=olp, ofr=ofr,
                           scorer=CR.CiderDOracle(df, n))
    return _cache[key]


def _coverage(case, oseq):
    """What keeps a decode that only ever emits one id from passing: the distinct ids the oracle's tokens take over the
    case (case c instead: the rows that end before T)."""
    if case == 'c':
        return int((oseq == 0).any(-1).sum()), 40
    return int(np.unique(oseq).size), min(CASES[case]['vocab'], 20)


# ---------------------------------------------------------------------------------------- engines
@pytest.fixture(scope='module')
def engines():
    """One small engine per dimension case, made at its first use and kept for the module. The pair-bounded lse is pinned
    as tests/test_gpu_screen.py pins it (read at create): greedy-only decodes then always run the PAIRS instantiations,
    which the screened loop needs; the log-prob passes take the exact ones."""
    import nicnes
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    made = {}

    def get(case):
        if case not in made:
            c = CASES[case]
            mp = pytest.MonkeyPatch()
            mp.setenv('NICNES_BOUNDED_LSE', '1')
            try:
                e = nicnes.Engine(vocab_size=c['vocab'], fc_feat_size=c['F'], seq_length=c['T'], max_batch=c['B'],
                                  max_members=4, noise_len=NOISE_LEN, noise_seed=SEED)
            finally:
                mp.undo()
            e.set_noise_table(_table())
            assert e.D == _dims(case).D
            made[case] = e
        return made[case]
    yield get
    for e in made.values():
        e.close()


def _load(e, theta, fc, gts, df, n):
    import nicnes
    e.set_theta(theta)
    keys, vals = nicnes.df_table_arrays(df)
    e.set_df_table(keys, vals, np.log(float(n)))
    e.set_batch(fc, gts)


def _reset(e):
    e.set_fitness_mode('greedy')
    e.set_sample_draws(None)
    e.set_mutation('plain')
    e.set_decode_split(0, 0)
    e.set_decode_coop(1)
    e.set_decode_screen('auto')


def _no_faults(e):
    st = e.stats()
    assert st['coop_timeouts'] == 0 and st['sample_slot_timeouts'] == 0, st


def _expected_path(dims, S, G, coop):
    """nicnes_decode_path for the few workgroups of these tests: coop needs 128-row slabs, S = 2 or 4 and no empty logit
    range (nst >= S); the split path takes the shapes it refuses."""
    nst = (dims.V1 + 63) // 64
    if S == 1:
        return 'fused'
    return 'coop' if (coop and G == 4 and nst >= S) else 'split'


def _close(got, want, rel=1e-9):
    return abs(got - want) <= rel * max(1.0, abs(want))


# ---------------------------------------------------------------------------------------- 1. greedy parity
@pytest.mark.parametrize('case,kind', GREEDY_WORLDS, ids=['%s_%s' % w for w in GREEDY_WORLDS])
def test_greedy_parity_on_every_path(engines, case, kind):
    """Tokens of every member and sign equal the oracle's on every decode path, and tokens and greedy fitness are the
    same bits on all of them; the fitness equals the CIDEr-D oracle's; the log-prob pass (exact lse) matches the oracle's
    log-probs on the positions a criterion counts, in a [.., T] array whose steps after the batch's exit are 0."""
    w = _world(case, kind)
    dims, B, T = w['dims'], CASES[case]['B'], CASES[case]['T']
    oseq, olp, ofr = w['oseq'], w['olp'], w['ofr']
    frag_rows = ofr.any(-1)
    assert frag_rows.mean() <= FRAGILE_CAP, 'too many fragile rows (%d of %d): change the fc seed, not the cap' % (
        frag_rows.sum(), frag_rows.size)
    got, need = _coverage(case, oseq)
    assert got >= need, (got, need)
    if case == 'i':                                        # the top id travels from the decode into the scorer's keys
        assert all((oseq[:, s] == dims.vocab_size).any() for s in range(2))
    nst = (dims.V1 + 63) // 64
    if kind == 'wc' and case in ('d', 'j'):                # ids of the narrow last stage are decoded (8 and 13 tokens)
        assert (oseq >= 64 * (nst - 1)).any()
    e = engines(case)
    _load(e, w['theta'], w['fc'], w['gts'], w['df'], w['n'])
    assert [int(i) for i in e.noise_indices(IT, 0, P).cpu().numpy()] == [_idx(dims, k) for k in range(P)]
    first = None
    try:
        for name, (S, G, coop, screen) in GREEDY_PATHS.items():
            e.set_decode_split(S, G)
            e.set_decode_coop(coop)
            e.set_decode_screen(screen)
            want_path = _expected_path(dims, S, G, coop)
            assert e.decode_path(B, P) == want_path, (name, e.decode_path(B, P), nst)
            before = e.stats()
            fit, seq = e.evaluate(IT, 0, P, SIGMA, return_seq=True)
            assert seq.shape == (P, 2, B, T) and seq.is_contiguous()
            fit, seq = fit.cpu().numpy(), seq.cpu().numpy()
            after = e.stats()
            screened = (after['screen_candidates'] + after['screen_fallback_rows']
                        - before['screen_candidates'] - before['screen_fallback_rows'])
            assert (screened > 0) == (name == 'fused_screened'), (name, before, after)
            if first is None:
                first = (fit, seq)
                for k in range(P):
                    for s in range(2):
                        assert _compare_tokens(seq[k, s], oseq[k, s], ofr[k, s]) == 0, (name, k, s)
                        f_ref, _ = CR.rollout_fitness(w['scorer'], seq[k, s], w['gts'])
                        assert _close(fit[k, s], f_ref), (name, k, s, fit[k, s], f_ref)
                assert fit.max() > 0.0
            else:
                assert np.array_equal(seq, first[1]), name
                assert np.array_equal(fit.view(np.uint64), first[0].view(np.uint64)), name
            # the log-prob pass: the exact-lse instantiations of the same path
            _, seq_l, lp = e.evaluate(IT, 0, P, SIGMA, return_seq=True, return_lp=True)
            assert lp.shape == (P, 2, B, T) and lp.is_contiguous()
            seq_l, lp = seq_l.cpu().numpy(), lp.cpu().numpy()
            assert np.array_equal(seq_l, first[1]), name
            assert np.isfinite(lp).all() and (lp <= 0).all(), name
            for k in range(P):
                for s in range(2):
                    keep = ~frag_rows[k, s]
                    m = np.concatenate([np.ones((B, 1), bool), oseq[k, s][:, :-1] > 0], 1) & keep[:, None]
                    assert np.abs(lp[k, s][m] - olp[k, s][m]).max() <= 1e-5, (name, k, s)
                    if keep.all():                         # steps after the batch's last finishing one stay 0
                        ends = np.where((oseq[k, s] == 0).any(1), (oseq[k, s] == 0).argmax(1) + 1, T)
                        assert (lp[k, s][:, ends.max():] == 0).all(), (name, k, s)
        _no_faults(e)
    finally:
        _reset(e)


# ---------------------------------------------------------------------------------------- 2. sampled decode
@pytest.mark.parametrize('case', ['b', 'd', 'i'])
def test_sampled_decode(engines, case):
    """mode 'sample' with given draws u [P, 2, B, T]: tokens equal the oracle's up to the first fragile draw (the one
    place the draws' row stride T is pinned), fitness = the CIDEr-D oracle's on the GPU's own rows."""
    w = _world(case)
    dims, B, T, table = w['dims'], CASES[case]['B'], CASES[case]['T'], _table()
    n_members = 2
    u = np.random.Generator(np.random.PCG64(5)).random((n_members, 2, B, T))
    e = engines(case)
    _load(e, w['theta'], w['fc'], w['gts'], w['df'], w['n'])
    try:
        e.set_fitness_mode('sample')
        e.set_sample_draws(u)
        fit, seq = e.evaluate(IT, 0, n_members, SIGMA, return_seq=True)
        assert seq.shape == (n_members, 2, B, T)
        fit, seq = fit.cpu().numpy(), seq.cpu().numpy()
        whole, ids = 0, set()
        for k in range(n_members):
            for s, sign in enumerate((+1, -1)):
                oseq, _, ofr = O.decode_sample(dims, O.perturb(w['theta'], table, _idx(dims, k), SIGMA, sign), w['fc'],
                                               u[k, s])
                _rows_agree(seq[k, s], oseq, ofr != 0)
                whole += int((~(ofr != 0).any(1)).sum())
                ids |= set(np.unique(oseq).tolist())
                f_ref, _ = CR.rollout_fitness(w['scorer'], seq[k, s], w['gts'])
                assert _close(fit[k, s], f_ref), (k, s, fit[k, s], f_ref)
        assert 2 * whole >= n_members * 2 * B, 'only %d of %d rows compared through their last step' % (
            whole, n_members * 2 * B)
        assert len(ids) >= min(CASES[case]['vocab'], 20), len(ids)
        _no_faults(e)
    finally:
        _reset(e)


# ---------------------------------------------------------------------------------------- 3. mutated decode
def _mutation_vector(mode, theta):
    if mode == 'scale':
        return np.abs(theta)
    return (0.5 + np.random.Generator(np.random.PCG64(3)).random(theta.size)).astype(np.float32)


def _mutated_world(case, mode):
    key = ('mut', case, mode)
    if key not in _cache:
        w = _world(case)
        dims, table = w['dims'], _table()
        vec = _mutation_vector(mode, w['theta'])
        out = []
        for k in range(2):
            for sign in (+1, -1):
                seq, _, fr = O.decode(dims, O.perturb(w['theta'], table, _idx(dims, k), SIGMA, sign, (mode, vec)), w['fc'])
                out.append((seq, fr))
        _cache[key] = (vec, out)
    return _cache[key]


MUTATED = [(c, m, sh) for c in ('d', 'h') for m in ('scale', 'divide') for sh in ((1, 4), (4, 2))] + [('a', 'scale', (1, 4))]


@pytest.mark.parametrize('case,mode,shape', MUTATED, ids=['%s_%s_S%dG%d' % (c, m, sh[0], sh[1]) for c, m, sh in MUTATED])
def test_mutated_decode(engines, case, mode, shape):
    """theta +- delta' on the fused path (which forms the image projection's and the embedding rows' delta' itself:
    nicnes_decode_img_mut_kernel, here at nK = 3, 32 and 1) and on the split path (materialised rows)."""
    w = _world(case)
    dims, table = w['dims'], _table()
    vec, ora = _mutated_world(case, mode)
    e = engines(case)
    _load(e, w['theta'], w['fc'], w['gts'], w['df'], w['n'])
    try:
        e.set_decode_split(*shape)
        e.set_decode_coop(0)
        e.set_mutation(mode, vec)
        assert e.decode_path(CASES[case]['B'], 2) == ('fused' if shape[0] == 1 else 'split')
        fit, seq = e.evaluate(IT, 0, 2, SIGMA, return_seq=True)
        fit, seq = fit.cpu().numpy(), seq.cpu().numpy()
        dv = e.noise_vectors(IT, 0, 2, SIGMA).cpu().numpy()
        cut = 0
        for k in range(2):
            want = O.member_delta(table, _idx(dims, k), SIGMA, dims.D, (mode, vec))
            assert np.array_equal(dv[k].view(np.uint32), want.view(np.uint32)), k
            assert not np.array_equal(want, O.member_delta(table, _idx(dims, k), SIGMA, dims.D))
            for s in range(2):
                oseq, fr = ora[2 * k + s]
                assert _compare_tokens(seq[k, s], oseq, fr) == 0, (k, s)
                cut += int(fr.any(1).sum())
                f_ref, _ = CR.rollout_fitness(w['scorer'], seq[k, s], w['gts'])
                assert _close(fit[k, s], f_ref), (k, s, fit[k, s], f_ref)
        assert cut <= FRAGILE_CAP * 4 * CASES[case]['B'], cut
        _no_faults(e)
    finally:
        _reset(e)


# ---------------------------------------------------------------------------------------- 4. theta itself
@pytest.mark.parametrize('case', ['b', 'c', 'i'])
def test_theta_itself_and_the_resident_split(engines, case):
    """evaluate_theta's rows equal the sign-+ rows of a sigma = 0 member on every decode shape (tokens and greedy fitness
    bit for bit); a resident split's one-call decode gives the same rows over [0, B) and over the odd inner range
    [1, B - 2); Split.evaluate's CIDEr row scores equal Split.score's of the same tokens."""
    w = _world(case)
    dims, B, T = w['dims'], CASES[case]['B'], CASES[case]['T']
    e = engines(case)
    _load(e, w['theta'], w['fc'], w['gts'], w['df'], w['n'])
    sp = e.make_split(w['fc'], w['gts'])
    try:
        ref = None
        for path, (S, G, coop) in PATHS.items():
            e.set_decode_split(S, G)
            e.set_decode_coop(coop)
            f2, seq2 = e.evaluate(0, 0, 1, 0.0, return_seq=True)
            f1, seq1 = e.evaluate_theta(0, return_seq=True)
            assert seq1.shape == (B, T)
            f2, f1, seq2, seq1 = f2.cpu().numpy(), f1.cpu().numpy(), seq2.cpu().numpy(), seq1.cpu().numpy()
            assert np.array_equal(seq1, seq2[0, 0]) and np.array_equal(seq2[0, 0], seq2[0, 1]), path
            assert f1[0] == f2[0, 0] == f2[0, 1], (path, f1, f2)
            if ref is None:
                ref = (f1, seq1)
                fr = O.decode(dims, w['theta'], w['fc'])[2]
                assert _compare_tokens(seq1, w['base'], fr) == 0
                f_ref, _ = CR.rollout_fitness(w['scorer'], seq1, w['gts'])
                assert _close(f1[0], f_ref), (f1, f_ref)
            assert np.array_equal(seq1, ref[1]) and f1[0] == ref[0][0], path
            for first, count in ((0, B), (1, B - 3)):
                rows = sp.decode(first, count)
                assert rows.shape == (count, T)
                assert np.array_equal(rows.cpu().numpy(), seq1[first:first + count]), (path, first, count)
            (res, totals, cider), seq_e = sp.evaluate(detail=True, return_seq=True)
            assert np.array_equal(seq_e.cpu().numpy(), seq1), path
            res_s, totals_s, cider_s = sp.score(seq_e, detail=True)
            assert np.array_equal(cider.view(np.uint64), cider_s.view(np.uint64)) and np.array_equal(totals, totals_s)
            assert res == res_s and cider.shape == (B,)
        _no_faults(e)
    finally:
        sp.close()
        _reset(e)


# ---------------------------------------------------------------------------------------- 5. nic_es
ES_GEN, ES_PARENT_OF = 9, [1, 0, 1]


def _es_world(mode):
    """Case d's dims: two parents with planted exact zeros, the three pairs' offspring and their oracle decodes."""
    key = ('es', mode)
    if key not in _cache:
        dims, table, fc = _dims('d'), _table(), _fc('d')
        if 'es_parents' not in _cache:
            parents = []
            for s in (4, 11):
                th = O.make_theta(dims, s, 4.0, 0.1)
                th[:dims.E * dims.F:7] = 0.0
                assert R.mean_off_boundary(th), 'seed %d puts mean|theta| on a rounding boundary: change the seed' % s
                parents.append(th)
            _cache['es_parents'] = parents, _references(dims, parents[0], fc, 3)[1:]
        parents, (gts, df, n) = _cache['es_parents']
        off = {}
        oseq = np.zeros((3, 2, fc.shape[0], dims.T), np.int32)
        frag = np.zeros((3, 2, fc.shape[0]), bool)
        for k, p in enumerate(ES_PARENT_OF):
            for sign in (0, 1):
                off[k, sign] = R.offspring(parents[p], table, _idx(dims, k, ES_GEN), SIGMA, sign, mode)
                oseq[k, sign], _, fr = O.decode(dims, off[k, sign], fc)
                frag[k, sign] = fr.any(axis=1)
        _cache[key] = dict(dims=dims, fc=fc, parents=parents, gts=gts, df=df, n=n, off=off, oseq=oseq, frag=frag)
    return _cache[key]


@pytest.mark.parametrize('mode', E.MODES)
def test_es_generation(engines, mode):
    """es_evaluate on the fused path and on coop S = 2 (nst = 2: it just fits) against the oracle decode of every
    offspring; es_offspring is fp32(parent +- delta') bit for bit; after es_select and es_advance the new parent rows
    are those offspring bit for bit (Dp, D rounded up to 64, differs from D here: D % 64 = 4)."""
    w = _es_world(mode)
    dims, B = w['dims'], CASES['d']['B']
    assert dims.D % 64 == 4
    assert w['frag'].mean() <= FRAGILE_CAP, w['frag'].sum()
    assert np.unique(w['oseq']).size >= 20
    e = engines('d')
    _load(e, w['parents'][0], w['fc'], w['gts'], w['df'], w['n'])
    scorer = CR.CiderDOracle(w['df'], w['n'])
    try:
        e.es_create(4, 1)
        e.es_set_parents(w['parents'])
        e.es_set_mutation(mode)
        e.set_decode_screen(False)
        for (k, sign), want in w['off'].items():
            got = e.es_offspring(ES_GEN, k, sign, SIGMA, ES_PARENT_OF[k]).cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (k, sign)
        assert e.es_decode_path(B, 3) == 'fused'
        fit, seq = e.es_evaluate(ES_GEN, 0, 3, SIGMA, ES_PARENT_OF, return_seq=True)
        assert seq.shape == (3, 2, B, dims.T)
        fit_np, seq = fit.cpu().numpy(), seq.cpu().numpy()
        E._check_against_oracle(seq, fit_np, w['oseq'], w['frag'], scorer, w['gts'])
        e.es_set_decode('coop', 2)
        assert e.es_decode_path(B, 3) == 'coop'
        fit_c, seq_c = e.es_evaluate(ES_GEN, 0, 3, SIGMA, ES_PARENT_OF, return_seq=True)
        assert np.array_equal(seq_c.cpu().numpy(), seq)
        assert np.array_equal(fit_c.cpu().numpy().view(np.uint64), fit_np.view(np.uint64))
        e.es_set_decode('fused')
        order = e.es_select(fit, 3)
        assert np.array_equal(order.cpu().numpy(), R.select(fit_np, 3))
        e.es_advance(ES_GEN, SIGMA, ES_PARENT_OF, order)
        for i, o in enumerate(order.cpu().numpy()):
            row = e.es_row(i).cpu().numpy()
            assert row.shape == (dims.D,)
            assert np.array_equal(row.view(np.uint32), w['off'][int(o) >> 1, int(o) & 1].view(np.uint32)), (i, o)
        _no_faults(e)
    finally:
        e.es_set_decode('fused')
        e.es_free()
        _reset(e)


# ---------------------------------------------------------------------------------------- 6. update kernels
@pytest.mark.parametrize('case', ['a', 'd'])
def test_update_kernels_on_an_unaligned_D(case):
    """D is no multiple of 64 (nor of 256: the update kernels' last workgroup is partial): the weighted noise sum, whole
    and in 64-aligned ranges with a short last one, plain and scaled, equals the fp64 member-order sum rounded once;
    three Adam and three SGD steps over the whole of D equal the oracle optimizers bit for bit."""
    import nicnes
    dims, table = _dims(case), _table()
    D, n_members = dims.D, 5
    assert D % 64 in (4, 8) and D % 256 != 0
    theta = _theta(case)
    e = nicnes.Engine(vocab_size=dims.vocab_size, fc_feat_size=dims.F, seq_length=dims.T, max_batch=8,
                      max_members=n_members, noise_len=NOISE_LEN, noise_seed=SEED)
    try:
        assert e.D == D
        e.set_noise_table(table)
        e.set_theta(theta)
        rng = np.random.Generator(np.random.PCG64(1))
        w_np = (rng.random(n_members) - 0.5).astype(np.float32)
        w_t = torch.from_numpy(w_np).to(e.device)
        idx = [_idx(dims, k, 9) for k in range(n_members)]
        cuts = [0, 64 * (D // 192), 64 * (D // 96), 64 * (D // 64), D]       # the last range holds D % 64 entries
        assert cuts[-1] - cuts[-2] == D % 64 and all(c % 64 == 0 for c in cuts[:-1])
        for mut in (None, ('scale', np.abs(theta))):
            e.set_mutation(*(mut or ('plain',)))
            acc = np.zeros(D, np.float64)
            for k in range(n_members):
                acc += np.float64(w_np[k]) * O.member_delta(table, idx[k], SIGMA, D, mut).astype(np.float64)
            want = acc.astype(np.float32)
            g = e.grad_partial(9, 0, n_members, w_t, SIGMA).cpu().numpy()
            assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), mut and mut[0]
            out = torch.full((D,), float('nan'), dtype=torch.float32, device=e.device)
            for j0, j1 in zip(cuts[:-1], cuts[1:]):
                e.grad_partial_range(9, 0, n_members, w_t, SIGMA, j0, j1, out)
            assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), mut and mut[0]
        e.set_mutation('plain')
        l2, step, pop = 1e-3, 1e-3, 5
        gsums = [np.random.Generator(np.random.PCG64(20 + k)).standard_normal(D).astype(np.float32) for k in range(3)]
        for kind in ('adam', 'sgd'):
            e.set_theta(theta)
            e.set_adam_state(np.zeros(D), np.zeros(D), 0)
            ora = O.AdamOracle(theta.copy(), step) if kind == 'adam' else O.SGDOracle(theta.copy(), step, 0.9)
            for k in range(3):
                gs = torch.from_numpy(gsums[k]).to(e.device)
                ratio = e.adam_step(gs, pop, l2, step) if kind == 'adam' else e.sgd_step(gs, pop, l2, step, 0.9)
                old = np.asarray(ora.theta, np.float64)
                r_ora, th_ref = O.master_update(ora, gsums[k] / np.float32(2 * pop), l2)
                # |step| / |theta_old| in fp64 from the oracle's own state and expressions: the ratio the oracle returns
                # takes |theta_old| in fp32 at its first step (theta is an fp32 array until then), 1e-7 off by itself
                if kind == 'adam':
                    a = ora.stepsize * np.sqrt(1 - ora.beta2 ** ora.t) / (1 - ora.beta1 ** ora.t)
                    st = -a * ora.m / (np.sqrt(ora.v) + ora.epsilon)
                else:
                    st = -ora.stepsize * ora.v
                r_ref = np.linalg.norm(st) / np.linalg.norm(old)
                assert abs(r_ref - r_ora) <= (1e-6 if k == 0 else 1e-12) * r_ora, (kind, k, r_ref, r_ora)
                t64, t32 = e.theta()
                assert np.array_equal(t64.cpu().numpy().view(np.uint64), th_ref.view(np.uint64)), (kind, k)
                assert np.array_equal(t32.cpu().numpy(), th_ref.astype(np.float32)), (kind, k)
                m, v, t = e.adam_state()
                if kind == 'adam':
                    assert np.array_equal(m.cpu().numpy().view(np.uint64), ora.m.view(np.uint64)), (kind, k)
                assert np.array_equal(v.cpu().numpy().view(np.uint64), ora.v.view(np.uint64)), (kind, k)
                assert t == k + 1
                assert abs(ratio - r_ref) <= 1e-9 * r_ref, (kind, k, ratio, r_ref)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------- 7. sensitivity
def _sens_reference(F):
    key = ('sens', F)
    if key not in _cache:
        from oracle import sensitivity_ref as SR
        dims = O.Dims(F=F)
        theta = O.make_theta(dims, 3, 4.0, 0.1)
        fc = np.random.Generator(np.random.PCG64(78)).standard_normal((12, F)).astype(np.float32)
        _cache[key] = theta, fc, SR.sum_sensitivity((dims.V1, dims.E, dims.R, F), theta, fc, 12).numpy()
    return _cache[key]


@pytest.mark.parametrize('F,T', [(128, 16), (384, 16), (128, 3)], ids=['F128', 'F384', 'F128_seq_length3'])
def test_sensitivity_off_the_default_F(F, T):
    """nicnes_sum_sensitivity takes F as a parameter and has its own forward length 5: the vector matches the autograd
    restatement at F = 128 and 384, does not depend on the handle's seq_length, and is the same bits when repeated."""
    import nicnes
    theta, fc, ref = _sens_reference(F)
    e = nicnes.Engine(fc_feat_size=F, seq_length=T, max_batch=12, max_members=2, noise_len=NOISE_LEN, noise_seed=0)
    try:
        e.set_noise_table(_table())
        e.set_theta(theta)
        e.set_df_table(np.zeros(0, np.uint64), np.zeros(0), np.log(64.0))
        e.set_batch(fc, [np.zeros((1, T), np.int32)] * 12)
        raw = e.sum_sensitivity(12).cpu().numpy()
        assert np.array_equal(e.sum_sensitivity(12).cpu().numpy().view(np.uint32), raw.view(np.uint32))
    finally:
        e.close()
    ok, worst = _sens_close(raw, ref)
    assert ok, worst


# ---------------------------------------------------------------------------------------- 8. the limits
@pytest.mark.parametrize('kw', [dict(fc_feat_size=192), dict(fc_feat_size=0), dict(vocab_size=8), dict(vocab_size=6),
                                dict(vocab_size=16387), dict(seq_length=0), dict(seq_length=17)],
                         ids=['F192', 'F0', 'V1_9', 'V1_7', 'V1_16388', 'T0', 'T17'])
def test_create_refuses_what_the_header_excludes(kw):
    import nicnes
    with pytest.raises(nicnes.NicnesError, match='nicnes_create failed: not supported'):
        nicnes.Engine(max_batch=8, max_members=1, noise_len=NOISE_LEN, **kw)


@pytest.mark.parametrize('kw', [dict(vocab_size=7, fc_feat_size=128, seq_length=1),
                                dict(vocab_size=16383, fc_feat_size=128, seq_length=1)], ids=['smallest', 'V1_16384'])
def test_create_accepts_the_edges(kw):
    import nicnes
    e = nicnes.Engine(max_batch=8, max_members=1, noise_len=NOISE_LEN, **kw)
    try:
        d = O.Dims(vocab_size=kw['vocab_size'], F=kw['fc_feat_size'], T=kw['seq_length'])
        assert e.D == d.D and e.offsets[:9] == [d.offsets()[name][0] for name, _ in d.shapes()]
    finally:
        e.close()
