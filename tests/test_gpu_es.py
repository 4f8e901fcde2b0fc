"""nic_es on the GPU (nicnes_es_*, nicnes.es): offspring over several base thetas decoded in one launch, the device-side
selection and the next parents' materialisation, checked against the host restatement tests/es_ref.py and the oracle."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from oracle import oracle as O          # noqa: E402
from oracle import cider_ref as CR      # noqa: E402
from tests import es_ref as R           # noqa: E402

NOISE_LEN = 1 << 23
SIGMA = 0.01
SEED, GEN = 6, 9
PARENT_OF = [2, 0, 2, 1, 0]            # 5 pairs over 3 parents: slot 0 and the last slot, a parent shared by two pairs
MODES = ['plain', 'scale']
FRAGILE_CAP = 0.10                     # a test may leave at most this share of its (offspring, row) pairs unchecked

_cache = {}


def _world():
    """dims, the noise table and three parents with distinct seeds and planted exact zeros (shared, never modified)."""
    if not _cache:
        dims = O.Dims()
        parents = []
        for s in (4, 11, 23):
            th = O.make_theta(dims, s, 4.0, 0.1)
            th[:dims.E * dims.F:7] = 0.0                 # exact zeros: SM-PROPORTIONAL's mean replacement
            th[dims.D - 5 * dims.R + 3] = -0.0
            assert R.mean_off_boundary(th), 'seed %d puts mean|theta| on a rounding boundary: change the seed' % s
            parents.append(th)
        _cache.update(dims=dims, parents=parents, table=O.noise_table(NOISE_LEN, 123))
    return _cache['dims'], _cache['parents'], _cache['table']


def _engine(B, members=5, max_parents=6, max_elites=2):
    import nicnes
    e = nicnes.Engine(max_batch=B, max_members=members, noise_len=NOISE_LEN, noise_seed=SEED)
    e.set_noise_table(_world()[2])
    e.es_create(max_parents, max_elites)
    return e


def _idx(pair, gen=GEN):
    dims, _, table = _world()
    return O.noise_index(SEED, gen, pair, table.size, dims.D)


@pytest.mark.parametrize('mode', MODES)
def test_offspring_bits(mode):
    """es_offspring equals the numpy formula bit for bit, both signs of every pair; the parents' statistics are the
    fp64 mean rounded once and the exact-zero count."""
    dims, parents, table = _world()
    e = _engine(8)
    try:
        e.es_set_parents(parents)
        e.es_set_mutation(mode)
        for p, th in enumerate(parents):
            mean, zeros = e.es_row_stats(p)
            assert mean == R.parent_mean(th) and zeros == int((th == 0).sum())
            assert np.array_equal(e.es_row(p).cpu().numpy(), th)
        for k, p in enumerate(PARENT_OF):
            for sign in (0, 1):
                got = e.es_offspring(GEN, k, sign, SIGMA, p).cpu().numpy()
                want = R.offspring(parents[p], table, _idx(k), SIGMA, sign, mode)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (k, sign)
        if mode == 'scale':
            plain = R.offspring(parents[2], table, _idx(0), SIGMA, 0, 'plain')
            assert not np.array_equal(plain, R.offspring(parents[2], table, _idx(0), SIGMA, 0, 'scale'))
        with pytest.raises(Exception):
            e.es_offspring(GEN, 0, 0, SIGMA, 3)          # beyond the parent count
    finally:
        e.close()


def _workload(B):
    import nicnes.synthetic as S
    dims, parents, _ = _world()
    key = ('wl', B)
    if key not in _cache:
        fc = np.random.Generator(np.random.PCG64(31 + B)).standard_normal((B, dims.F)).astype(np.float32)
        base, _, _ = O.decode(dims, parents[0], fc)
        gts, df, n = S.build_references(base, dims.vocab_size, seed=3, n_refs=5, df_sets=128)
        _cache[key] = (fc, gts, df, n)
    return _cache[key]


def _oracle_offspring(B, mode, parent_of, gen=GEN, sigma=SIGMA, parents=None):
    """(tokens [pairs, 2, B, T], fragile rows [pairs, 2, B]) of every offspring, on the CPU."""
    dims, base_parents, table = _world()
    parents = parents or base_parents
    fc = _workload(B)[0]
    seqs = np.zeros((len(parent_of), 2, B, dims.T), np.int32)
    frag = np.zeros((len(parent_of), 2, B), bool)
    for k, p in enumerate(parent_of):
        for sign in (0, 1):
            th = R.offspring(parents[p], table, _idx(k, gen), sigma, sign, mode)
            seqs[k, sign], _, fr = O.decode(dims, th, fc)
            frag[k, sign] = fr.any(axis=1)
    return seqs, frag


def _check_against_oracle(seq, fit, oseq, frag, scorer, gts):
    ok = frag | (seq == oseq).all(axis=-1)
    assert ok.all(), np.argwhere(~ok)[:5]
    for k in range(seq.shape[0]):
        for s in range(2):
            if not frag[k, s].any():
                f_ref = CR.rollout_fitness(scorer, oseq[k, s], gts)[0]
                assert abs(fit[k, s] - f_ref) <= 1e-9 * max(1.0, f_ref), (k, s, fit[k, s], f_ref)


@pytest.mark.parametrize('B', [24, 130], ids=['B24_one_partial_slab', 'B130_two_slabs'])
@pytest.mark.parametrize('mode', MODES)
def test_decode_matches_oracle(monkeypatch, mode, B):
    """Every offspring's tokens and fitness against the oracle; screen off and screen forced on agree bit for bit; the
    slices (0, 2) + (2, 3) equal (0, 5) bit for bit (the second has pair_begin > 0), and so does the decode cut into two
    member ranges on two streams."""
    import nicnes
    dims, parents, _ = _world()
    fc, gts, df, n = _workload(B)
    oseq, frag = _oracle_offspring(B, mode, PARENT_OF)
    assert frag.mean() <= FRAGILE_CAP, 'too many fragile rows (%.3f): change the seed, not the cap' % frag.mean()
    # the bounded lse pinned, as tests/test_gpu_screen.py does: under the adaptive policy a decode of this peaked theta
    # that needed exact passes makes the next decodes sum the exp exactly, and those do not screen
    monkeypatch.setenv('NICNES_BOUNDED_LSE', '1')
    e = _engine(B)
    try:
        keys, vals = nicnes.df_table_arrays(df)
        e.set_df_table(keys, vals, np.log(float(n)))
        e.set_batch(fc, gts)
        e.es_set_parents(parents)
        e.es_set_mutation(mode)
        e.set_decode_screen(False)
        fit, seq = e.es_evaluate(GEN, 0, 5, SIGMA, PARENT_OF, return_seq=True)
        fit, seq = fit.cpu().numpy(), seq.cpu().numpy()
        _check_against_oracle(seq, fit, oseq, frag, CR.CiderDOracle(df, n), gts)
        fa, sa = e.es_evaluate(GEN, 0, 2, SIGMA, PARENT_OF[:2], return_seq=True)
        fb, sb = e.es_evaluate(GEN, 2, 3, SIGMA, PARENT_OF[2:], return_seq=True)
        assert np.array_equal(np.concatenate([sa.cpu().numpy(), sb.cpu().numpy()]), seq)
        assert np.array_equal(np.concatenate([fa.cpu().numpy(), fb.cpu().numpy()]).view(np.uint64), fit.view(np.uint64))
        e.set_decode_streams(2)                           # the pairs in two member ranges: parent_of shifts with them
        f2, s2 = e.es_evaluate(GEN, 0, 5, SIGMA, PARENT_OF, return_seq=True)
        assert np.array_equal(s2.cpu().numpy(), seq)
        assert np.array_equal(f2.cpu().numpy().view(np.uint64), fit.view(np.uint64))
        e.set_decode_streams(0)
        before = e.stats()['screen_candidates']
        e.set_decode_screen(True)
        fs, ss = e.es_evaluate(GEN, 0, 5, SIGMA, PARENT_OF, return_seq=True)
        assert e.stats()['screen_candidates'] > before, 'the screened kernels did not run'
        assert np.array_equal(ss.cpu().numpy(), seq)
        assert np.array_equal(fs.cpu().numpy().view(np.uint64), fit.view(np.uint64))
        assert e.stats()['coop_timeouts'] == 0
    finally:
        e.close()


def test_logprob_criterion_and_member_batches():
    """A greedy_* criterion (log-probs written by the fused path) and per-member batches through es_evaluate: pairs on
    batch 1 see its images."""
    import nicnes
    dims, parents, _ = _world()
    B = 24
    fc, gts, df, n = _workload(B)
    e = _engine(B)
    try:
        keys, vals = nicnes.df_table_arrays(df)
        e.set_df_table(keys, vals, np.log(float(n)))
        e.es_set_parents(parents)
        e.set_batches([(fc, gts), (fc[::-1].copy(), gts[::-1])])
        f, s = e.es_evaluate(GEN, 0, 2, SIGMA, [1, 1], return_seq=True, member_batch=[0, 1])
        s = s.cpu().numpy()
        assert not np.array_equal(s[0], s[1])
        f1, s1 = e.es_evaluate(GEN, 1, 1, SIGMA, [1], return_seq=True, member_batch=[1])
        assert np.array_equal(s1.cpu().numpy()[0], s[1])
        e.set_batch(fc, gts)
        e.set_fitness_mode('greedy_logprob')
        fl, sl, lp = e.es_evaluate(GEN, 0, 2, SIGMA, [1, 1], return_seq=True, return_lp=True)
        assert np.array_equal(sl.cpu().numpy()[0], s[0])
        assert np.isfinite(fl.cpu().numpy()).all() and (lp.cpu().numpy() <= 0).all()
    finally:
        e.close()


def _select_cases():
    rng = np.random.Generator(np.random.PCG64(99))
    out = {}
    out[2] = np.array([1.0, 1.0])
    out[7] = np.array([0.5, np.nan, -0.0, 0.0, 3.0, 0.5, -np.inf])
    for n in (2048, 2050):
        f = np.round(rng.standard_normal(n), 1)                       # many ties
        f[rng.integers(0, n, 9)] = np.nan
        f[rng.integers(0, n, 9)] = -0.0
        f[rng.integers(0, n, 9)] = 0.0
        f[n - 1] = np.nanmax(f) + 1.0                                 # the winner is the last entry (n = 2050: chunk 2)
        out[n] = f
    return out


def test_select_against_numpy():
    import nicnes
    cases = _select_cases()
    e = nicnes.Engine(vocab_size=63, max_batch=1, max_members=1025, noise_len=1 << 20, noise_seed=SEED)
    try:
        e.es_create(1, 1)
        for n, f in cases.items():
            ft = torch.from_numpy(f).to(e.device)
            for n_keep in sorted({1, n, min(n, 5)}):
                got = e.es_select(ft, n_keep).cpu().numpy()
                assert np.array_equal(got, R.select(f, n_keep)), (n, n_keep)
            with pytest.raises(nicnes.NicnesError):
                e.es_select(ft, n + 1)
            with pytest.raises(nicnes.NicnesError):
                e.es_select(ft, 0)
    finally:
        e.close()
    want = R.select(cases[7], 7)                                      # the hand-worked order of the 7-entry case
    assert list(want) == [4, 0, 5, 2, 3, 6, 1]


@pytest.mark.parametrize('mode', MODES)
def test_advance(mode):
    """The next table is [elite rows] + [numpy offspring of the selected ids], bit for bit: a parent selected through
    two pairs and both signs of one pair; the offspring are formed from the OLD parents although their rows are being
    replaced (the table is double-buffered); the statistics follow; a second advance goes back into the first table."""
    dims, parents, table = _world()
    e = _engine(8, max_parents=6, max_elites=2)
    try:
        e.es_set_parents(parents)
        e.es_set_mutation(mode)
        e.es_set_elite(0, 1)                              # elite 0 = parent 1, elite 1 = parent 0
        e.es_set_elite(1, 0)
        fit = np.array([[9.0, 8.0], [1.0, 2.0], [7.0, 0.0], [3.0, 6.5], [np.nan, 0.5]])
        ft = torch.from_numpy(fit).to(e.device)
        order = e.es_select(ft, 4)
        assert list(order.cpu().numpy()) == [0, 1, 4, 7]  # both signs of pair 0; parent 2 through pairs 0 and 2
        e.es_advance(GEN, SIGMA, PARENT_OF, order, n_front=2)
        want = [parents[1], parents[0]] + [R.offspring(parents[PARENT_OF[i >> 1]], table, _idx(i >> 1), SIGMA, i & 1, mode)
                                            for i in (0, 1, 4, 7)]
        for r, th in enumerate(want):
            assert np.array_equal(e.es_row(r).cpu().numpy().view(np.uint32), th.view(np.uint32)), r
            mean, zeros = e.es_row_stats(r)
            assert mean == R.parent_mean(th) and zeros == int((th == 0).sum()), r
        assert np.array_equal(e.es_row(0, 'elites').cpu().numpy(), parents[1])
        # the new rows are parents now: 6 of them, and the next generation perturbs them
        got = e.es_offspring(GEN + 1, 3, 1, SIGMA, 5).cpu().numpy()
        assert np.array_equal(got, R.offspring(want[5], table, _idx(3, GEN + 1), SIGMA, 1, mode))
        po2 = [5, 5, 0]
        order2 = e.es_select(torch.tensor([[1.0, 5.0], [4.0, 2.0], [3.0, 0.0]], dtype=torch.float64, device=e.device), 3)
        e.es_advance(GEN + 1, SIGMA, po2, order2, n_front=0)
        want2 = [R.offspring(want[po2[i >> 1]], table, _idx(i >> 1, GEN + 1), SIGMA, i & 1, mode) for i in (1, 2, 4)]
        for r, th in enumerate(want2):
            assert np.array_equal(e.es_row(r).cpu().numpy().view(np.uint32), th.view(np.uint32)), r
        with pytest.raises(Exception):
            e.es_advance(GEN + 2, SIGMA, [3], order2[:1], n_front=0)       # parent 3 of 3 parents
    finally:
        e.close()


def test_refusals():
    import nicnes
    dims, parents, _ = _world()
    B = 8
    fc, gts, df, n = _workload(B)
    e = _engine(B)
    try:
        keys, vals = nicnes.df_table_arrays(df)
        e.set_df_table(keys, vals, np.log(float(n)))
        e.set_batch(fc, gts)
        e.es_set_parents(parents)
        for shape in ((2, 4), (1, 2), (4, 2)):
            e.set_decode_split(*shape)
            with pytest.raises(nicnes.NicnesError, match='not supported'):
                e.es_evaluate(GEN, 0, 1, SIGMA, [0])
        e.set_decode_split(1, 4)
        e.es_evaluate(GEN, 0, 1, SIGMA, [0])
        e.set_decode_split(0, 0)
        for fm in ('sample', 'self_critical', 'sc_loss'):
            e.set_fitness_mode(fm)
            with pytest.raises(nicnes.NicnesError, match='not supported'):
                e.es_evaluate(GEN, 0, 1, SIGMA, [0])
        e.set_fitness_mode('greedy')
        with pytest.raises(nicnes.NicnesError, match='not supported'):
            e.es_set_mutation('divide')
        with pytest.raises(nicnes.NicnesError):
            e.es_evaluate(GEN, 0, 1, SIGMA, [3])                          # beyond the parent count
        e.es_evaluate(GEN, 0, 1, SIGMA, [2])
        torch.cuda.synchronize()
    finally:
        e.close()


ES_EXP = {
    'algorithm': 'nic_es', 'dataset': 'mscoco', 'nb_offspring': 8, 'population_size': 6, 'num_elites': 2,
    'num_elite_cands': 2, 'selection': 'tournament', 'tournament_size': 2,
    'config': {'noise_stdev': 0.01, 'batch_size': 16, 'patience': 1, 'stdev_divisor': 2.0, 'bs_multiplier': 1.0,
               'snapshot_freq': 0, 'num_val_items': 40},
    'policy_options': {'net': 'fc_caption', 'fitness': 'greedy',
                       'model_options': {'safe_mutations': 'SM-PROPORTIONAL', 'rnn_size': 128, 'input_encoding_size': 128}},
}


def test_three_generations_match_replay(tmp_path):
    """A 3-generation EngineESMaster run against tests/es_ref.Replay fed the engine's own fitness and validation
    scores: the same parents bit for bit, the same podium, the same schedule state; every offspring's fitness is the
    oracle's."""
    import nicnes
    import nicnes.synthetic as S
    from nicnes.es import ESExperimentSpec, EngineESMaster
    from nicnes.validation import Validator
    dims, _, table = _world()
    spec = ESExperimentSpec(ES_EXP)
    B = 16
    fc, gts, df, n = _workload(B)
    start = [O.make_theta(dims, 40 + i, 4.0, 0.1) for i in range(6)]
    vfc = np.random.Generator(np.random.PCG64(77)).standard_normal((40, dims.F)).astype(np.float32)
    vbase, _, _ = O.decode(dims, start[0], vfc)
    vgts, _, _ = S.build_references(vbase, dims.vocab_size, seed=5, n_refs=5, df_sets=40)
    e = nicnes.Engine(**spec.engine_kwargs(noise_len=NOISE_LEN, noise_seed=SEED, max_batch=B))
    try:
        e.set_noise_table(table)
        keys, vals = nicnes.df_table_arrays(df)
        e.set_df_table(keys, vals, np.log(float(n)))
        val = Validator(e, R.FakeLoader(vfc, vgts), 'val', 40)
        m = EngineESMaster(spec, e, validator=val, seed=3, thetas=start)
        rep = R.Replay(spec, start, table, SEED, dims, seed=3, mode='scale')
        scorer = CR.CiderDOracle(df, n)
        checked = total = 0
        for g in range(1, 4):
            m.step((fc, gts))
            last = m.last
            parent_of, child, sigma = rep.generation(last['fitness'], [sc for _, sc, _ in last['validated']])
            assert last['generation'] == g and np.array_equal(last['parent_of'], parent_of)
            assert sigma == last['sigma']
            for k in range(spec.n_pairs):
                for s in range(2):
                    oseq, _, fr = O.decode(dims, child(k, s), fc)
                    total += B
                    if not fr.any():
                        checked += B
                        f_ref = CR.rollout_fitness(scorer, oseq, gts)[0]
                        assert abs(last['fitness'][k, s] - f_ref) <= 1e-9 * max(1.0, f_ref), (g, k, s)
            assert m.n_parents == len(rep.parents)
            for r, th in enumerate(rep.parents):
                assert np.array_equal(e.es_row(r).cpu().numpy().view(np.uint32), th.view(np.uint32)), (g, r)
            for r, th in enumerate(rep.elites):
                assert np.array_equal(e.es_row(r, 'elites').cpu().numpy().view(np.uint32), th.view(np.uint32)), (g, r)
            assert m.podium.best_elites() == rep.podium.best_elites()
            assert m.sched.to_dict() == rep.sched.to_dict()
            assert m.cands == rep.cands
        assert checked >= (1.0 - FRAGILE_CAP) * total, 'too many fragile rollouts: change the seeds, not the cap'
        # run() drives the same step; the snapshot holds the rows in the reference's layout
        m.log_dir = str(tmp_path)
        stats = m.run([(fc, gts), (fc, gts)], generations=1)
        assert len(stats) == 4 and stats[-1]['iter'] == 4 and m.sched.iteration == 4
        snap = m.save_snapshot()
        assert [i for i, _ in snap['parents']] == list(range(m.n_parents)) and len(snap['best_elites']) == 2
        from nicnes.nes import param_shapes, vector_from_state_dict
        for kind, table, rows in (('parents', 'parents', range(m.n_parents)), ('elites_to_evaluate', 'parents', m.cands)):
            for (i, path), row in zip(snap[kind], rows):
                assert path.endswith('0_%d_%s_params.pth' % (i, 'parent' if kind == 'parents' else 'elite'))
                vec = vector_from_state_dict(torch.load(path, weights_only=True), param_shapes(e)).numpy()
                assert np.array_equal(vec, e.es_row(row, table).cpu().numpy())
        path, score = snap['best_elites'][0]
        assert path.endswith('best_elite/0_0_elite.pth') and score == m.podium.best_elites()[0][1]
        val.close()
    finally:
        e.close()
