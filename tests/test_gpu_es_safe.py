"""nic_es's safe mutations on the GPU (SM-G-SUM, SM-VECTOR: nicnes_set_mutation_divide_es, nicnes_sensitivity_es,
nicnes_set_sensitivity_es): one sensitivity per parent, every pair's delta' divided by its own parent's.

The engine's sensitivity agrees with the restatement oracle/sensitivity_ref.py only to fp32 rounding, so offspring bits are
always checked against the formula (tests/es_safe_ref.py) evaluated with the engine's own read-back row; the row itself is
checked apart, against Engine.sum_sensitivity bit for bit and against the oracle at tests/test_gpu_mutations.py's bar.
The world (parents, noise table, batches, pairs) is tests/test_gpu_es.py's; underflow 1e-3 (at mscoco_nes.json's 0.1 this
theta clamps nearly the whole vector to 1 and the division would hardly be exercised): tests/test_es_safe_host.py guards
that the workloads leave few rows fragile."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from oracle import oracle as O          # noqa: E402
from oracle import cider_ref as CR      # noqa: E402
from tests import es_ref as R           # noqa: E402
from tests import es_safe_ref as SRF    # noqa: E402
from tests import test_gpu_es as E      # noqa: E402  (the world only: nothing of it is modified)

GEN, SIGMA, PARENT_OF, FRAGILE_CAP, SEED, NOISE_LEN = E.GEN, E.SIGMA, E.PARENT_OF, E.FRAGILE_CAP, E.SEED, E.NOISE_LEN
UNDERFLOW = 1e-3
_small = {}


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _loaded(B, **kw):
    """tests/test_gpu_es.py's engine with its batch of B images, its df table and its three parents, in divide mode."""
    import nicnes
    fc, gts, df, n = E._workload(B)
    e = E._engine(B, **kw)
    keys, vals = nicnes.df_table_arrays(df)
    e.set_df_table(keys, vals, np.log(float(n)))
    e.set_batch(fc, gts)
    e.es_set_parents(E._world()[1])
    e.es_set_mutation_divide()
    return e


def _rows(e, slots):
    return {p: e.es_sensitivity_row(p).cpu().numpy() for p in slots}


def _want(parents, s, k, sign, p, gen=GEN, sigma=SIGMA, dims=None):
    dims = dims or E._world()[0]
    table = E._world()[2]
    return SRF.offspring(parents[p], table, O.noise_index(SEED, gen, k, table.size, dims.D), sigma, sign, 'divide', s)


def _small_world():
    """Vocabulary 999 (K = 11 groups, the last all padding), the sensitivity suite's own small shape: rows = 12."""
    if not _small:
        dims = O.Dims(vocab_size=999)
        fc = np.random.Generator(np.random.PCG64(78)).standard_normal((12, dims.F)).astype(np.float32)
        _small.update(dims=dims, fc=fc, parents=[O.make_theta(dims, s, 4.0, 0.1) for s in (3, 11, 23)])
    return _small['dims'], _small['parents'], _small['fc']


@pytest.mark.parametrize('shape', ['default_rows8', 'vocab999_rows12'])
def test_rows(shape):
    """es_sensitivity([0, 2]): row p is Engine.sum_sensitivity of parent p bit for bit (the same kernels on the same
    inputs), the oracle's within the project's bar, identical on a second call; slot 1, not named, stays invalid."""
    import nicnes
    if shape == 'default_rows8':
        dims, parents, _ = E._world()
        rows, fc = 8, E._workload(24)[0]
        e = _loaded(24)
    else:
        dims, parents, fc = _small_world()
        rows = 12
        e = nicnes.Engine(vocab_size=999, max_batch=rows, max_members=2, noise_len=NOISE_LEN, noise_seed=SEED)
        e.set_noise_table(E._world()[2])
        e.set_df_table(np.zeros(0, np.uint64), np.zeros(0), np.log(64.0))
        e.set_batch(fc, [np.zeros((1, dims.T), np.int32)] * rows)
        e.es_create(6, 2)
        e.es_set_parents(parents)
        e.es_set_mutation_divide()
    try:
        e.es_sensitivity([0, 2], rows, UNDERFLOW)
        got = _rows(e, (0, 2))
        for p in (0, 2):
            e.es_load_theta(p)
            assert np.array_equal(_bits(e.sum_sensitivity(rows, UNDERFLOW)), _bits(got[p])), p
            assert got[p].min() >= 1.0 and got[p].max() > 1.0
        assert not np.array_equal(got[0], got[2])
        with pytest.raises(nicnes.NicnesError, match='invalid'):
            e.es_sensitivity_row(1)
        with pytest.raises(nicnes.NicnesError, match='no valid sensitivity'):
            e.es_offspring(GEN, 3, 0, SIGMA, 1)
        e.es_offspring(GEN, 0, 0, SIGMA, 2)
        e.es_sensitivity([0, 2], rows, UNDERFLOW)
        again = _rows(e, (0, 2))
        assert all(np.array_equal(_bits(again[p]), _bits(got[p])) for p in (0, 2))
    finally:
        e.close()
    for p in (0, 2):
        ok, worst = SRF.sens_close(got[p], SRF.oracle_sensitivity(dims, parents[p], fc[:rows], UNDERFLOW))
        print('parent %d: worst error / bound %.3g' % (p, worst))
        assert ok, (p, worst)


def test_offspring_bits():
    """es_offspring = fp32(theta_p +- fp32(fp32(sigma z) / s_p)) with the read-back row, bit for bit, for every pair and
    sign: per-parent rows, then a shared vector (every parent uses it), then back to 'scale' and 'plain' on the handle."""
    dims, parents, table = E._world()
    e = _loaded(24)
    try:
        e.es_sensitivity([0, 1, 2], 8, UNDERFLOW)
        s = _rows(e, (0, 1, 2))
        for k, p in enumerate(PARENT_OF):
            for sign in (0, 1):
                got = e.es_offspring(GEN, k, sign, SIGMA, p)
                assert np.array_equal(_bits(got), _bits(_want(parents, s[p], k, sign, p))), (k, sign)
        assert not np.array_equal(_want(parents, s[2], 0, 0, 2), R.offspring(parents[2], table, E._idx(0), SIGMA, 0, 'plain'))
        rng = np.random.Generator(np.random.PCG64(17))
        vec = rng.uniform(1.0, 50.0, dims.D).astype(np.float32)
        planted = vec.copy()
        planted[::5] = 1.0
        planted[dims.D - 3:] = 1.0
        for v in (vec, planted):
            e.es_set_sensitivity(v)
            for p in (0, 1, 2):
                assert np.array_equal(_bits(e.es_sensitivity_row(p)), _bits(v))
            for k, p in enumerate(PARENT_OF):
                for sign in (0, 1):
                    got = e.es_offspring(GEN, k, sign, SIGMA, p)
                    assert np.array_equal(_bits(got), _bits(_want(parents, v, k, sign, p))), (k, sign)
        one = np.flatnonzero(planted == 1.0)
        got, plain = e.es_offspring(GEN, 1, 1, SIGMA, 0).cpu().numpy(), R.offspring(parents[0], table, E._idx(1), SIGMA, 1, 'plain')
        assert np.array_equal(got[one], plain[one]) and not np.array_equal(got, plain)
        for mode in ('scale', 'plain'):
            e.es_set_mutation(mode)
            for k, p in enumerate(PARENT_OF):
                got = e.es_offspring(GEN, k, k & 1, SIGMA, p)
                assert np.array_equal(_bits(got), _bits(R.offspring(parents[p], table, E._idx(k), SIGMA, k & 1, mode))), (mode, k)
        e.es_set_mutation_divide()                        # the shared vector is still there
        assert np.array_equal(_bits(e.es_offspring(GEN, 0, 0, SIGMA, 2)), _bits(_want(parents, planted, 0, 0, 2)))
    finally:
        e.close()


@pytest.mark.parametrize('B,rows', [(24, 8), (130, 16)], ids=['B24_one_partial_slab', 'B130_two_slabs'])
def test_decode_matches_oracle(monkeypatch, B, rows):
    """Tokens and fitness of every offspring against the oracle's decode of the bit-exact offspring (formed with the
    engine's own rows); screen off = screen forced on, the slices (0, 2) + (2, 3) = (0, 5), and the coop path, bit for
    bit."""
    dims, parents, _ = E._world()
    fc, gts, df, n = E._workload(B)
    monkeypatch.setenv('NICNES_BOUNDED_LSE', '1')         # as tests/test_gpu_es.py pins it
    e = _loaded(B)
    try:
        e.es_sensitivity(sorted(set(PARENT_OF)), rows, UNDERFLOW)
        s = _rows(e, (0, 1, 2))
        e.set_decode_screen(False)
        fit, seq = e.es_evaluate(GEN, 0, 5, SIGMA, PARENT_OF, return_seq=True)
        fit, seq = fit.cpu().numpy(), seq.cpu().numpy()
        oseq = np.zeros((5, 2, B, dims.T), np.int32)
        frag = np.zeros((5, 2, B), bool)
        for k, p in enumerate(PARENT_OF):
            for sign in (0, 1):
                oseq[k, sign], _, fr = O.decode(dims, _want(parents, s[p], k, sign, p), fc)
                frag[k, sign] = fr.any(axis=1)
        print('fragile share %.4f' % frag.mean())
        assert frag.mean() <= FRAGILE_CAP, 'too many fragile rows (%.3f): change the seed, not the cap' % frag.mean()
        E._check_against_oracle(seq, fit, oseq, frag, CR.CiderDOracle(df, n), gts)
        fa, sa = e.es_evaluate(GEN, 0, 2, SIGMA, PARENT_OF[:2], return_seq=True)
        fb, sb = e.es_evaluate(GEN, 2, 3, SIGMA, PARENT_OF[2:], return_seq=True)
        assert np.array_equal(np.concatenate([sa.cpu().numpy(), sb.cpu().numpy()]), seq)
        assert np.array_equal(np.concatenate([_bits(fa), _bits(fb)]), _bits(fit))
        before = e.stats()['screen_candidates']
        e.set_decode_screen(True)
        fs, ss = e.es_evaluate(GEN, 0, 5, SIGMA, PARENT_OF, return_seq=True)
        assert e.stats()['screen_candidates'] > before, 'the screened kernels did not run'
        assert np.array_equal(ss.cpu().numpy(), seq) and np.array_equal(_bits(fs), _bits(fit))
        e.set_decode_screen(False)
        e.es_set_decode('coop', 2)
        assert e.es_decode_path(B, 5) == 'coop'
        fc_, sc_ = e.es_evaluate(GEN, 0, 5, SIGMA, PARENT_OF, return_seq=True)
        assert np.array_equal(sc_.cpu().numpy(), seq) and np.array_equal(_bits(fc_), _bits(fit))
        assert e.stats()['coop_timeouts'] == 0
    finally:
        e.close()


def test_advance():
    """The survivors are the formula's offspring over the rows read back before the advance, bit for bit, with fresh
    statistics; the advance checks every parent of the generation and leaves no row valid; es_set_parent invalidates its
    slot only."""
    import nicnes
    dims, parents, table = E._world()
    e = _loaded(8, max_parents=6, max_elites=2)
    try:
        e.es_sensitivity([0, 1, 2], 8, UNDERFLOW)
        s = _rows(e, (0, 1, 2))
        e.es_set_elite(0, 1)
        fit = torch.from_numpy(np.array([[9.0, 8.0], [1.0, 2.0], [7.0, 0.0], [3.0, 6.5], [np.nan, 0.5]])).to(e.device)
        order = e.es_select(fit, 4)
        assert list(order.cpu().numpy()) == [0, 1, 4, 7]
        e.es_set_parent(1, parents[1])                    # slot 1's row is no longer valid: pair 3 names it
        with pytest.raises(nicnes.NicnesError, match='no valid sensitivity'):
            e.es_advance(GEN, SIGMA, PARENT_OF, order, n_front=1)
        assert np.array_equal(e.es_row(0).cpu().numpy(), parents[0]), 'the refused advance swapped the tables'
        e.es_offspring(GEN, 0, 0, SIGMA, 0)               # ... and slots 0 and 2 stay valid
        e.es_set_sensitivity(s[1], slot=1)
        assert np.array_equal(_bits(e.es_sensitivity_row(1)), _bits(s[1]))
        e.es_advance(GEN, SIGMA, PARENT_OF, order, n_front=1)
        want = [parents[1]] + [_want(parents, s[PARENT_OF[i >> 1]], i >> 1, i & 1, PARENT_OF[i >> 1]) for i in (0, 1, 4, 7)]
        for r, th in enumerate(want):
            assert np.array_equal(_bits(e.es_row(r)), _bits(th)), r
            mean, zeros = e.es_row_stats(r)
            assert mean == R.parent_mean(th) and zeros == int((th == 0).sum()), r
        # five parents now, none with a sensitivity
        for p in range(5):
            with pytest.raises(nicnes.NicnesError, match='invalid'):
                e.es_sensitivity_row(p)
        sentinel = torch.full((1, 2), -7.0, dtype=torch.float64, device=e.device)
        with pytest.raises(nicnes.NicnesError, match='invalid argument.*no valid sensitivity'):
            e.es_evaluate(GEN + 1, 0, 1, SIGMA, [0], fitness_out=sentinel)
        e.es_sensitivity([0, 4], 8, UNDERFLOW)
        f = e.es_evaluate(GEN + 1, 0, 2, SIGMA, [0, 4]).cpu().numpy()
        assert np.isfinite(f).all() and (sentinel.cpu().numpy() == -7.0).all()
        s4 = e.es_sensitivity_row(4).cpu().numpy()
        got = e.es_offspring(GEN + 1, 1, 1, SIGMA, 4)
        assert np.array_equal(_bits(got), _bits(_want(want, s4, 1, 1, 4, gen=GEN + 1)))
        with pytest.raises(nicnes.NicnesError, match='no valid sensitivity'):
            e.es_evaluate(GEN + 1, 0, 2, SIGMA, [0, 1])
        e.es_set_parent(4, parents[0])
        with pytest.raises(nicnes.NicnesError, match='no valid sensitivity'):
            e.es_offspring(GEN + 1, 0, 0, SIGMA, 4)
        e.es_offspring(GEN + 1, 0, 0, SIGMA, 0)
    finally:
        e.close()


ES_EXP = {
    'algorithm': 'nic_es', 'dataset': 'mscoco', 'nb_offspring': 10, 'population_size': 3, 'num_elites': 1,
    'num_elite_cands': 0, 'selection': 'uniform',
    'config': {'noise_stdev': 0.01, 'batch_size': 16, 'patience': 100, 'stdev_divisor': 2.0, 'bs_multiplier': 1.0,
               'snapshot_freq': 0},
    'policy_options': {'net': 'fc_caption', 'fitness': 'greedy', 'model_options': {}},
}


def _spec(mutation, **model_options):
    import copy
    from nicnes.es import ESExperimentSpec
    exp = copy.deepcopy(ES_EXP)
    exp['policy_options']['model_options'] = dict(model_options, safe_mutations=mutation)
    return ESExperimentSpec(exp)


def _master_engine(spec, B):
    import nicnes
    fc, gts, df, n = E._workload(B)
    e = nicnes.Engine(**spec.engine_kwargs(noise_len=NOISE_LEN, noise_seed=SEED, max_batch=B))
    e.set_noise_table(E._world()[2])
    keys, vals = nicnes.df_table_arrays(df)
    e.set_df_table(keys, vals, np.log(float(n)))
    return e, (fc, gts)


def _parents_now(e, n):
    return np.stack([e.es_row(i).cpu().numpy() for i in range(n)])


def test_master_sum_equals_the_calls_by_hand():
    """EngineESMaster with SM-G-SUM, two generations: the parents after each equal those of the same calls made by hand
    (sensitivity of the distinct parents on min(B, batch_size) rows, evaluate, select, advance), and a second run's."""
    from nicnes.es import EngineESMaster, draw_parents
    spec = _spec('SM-G-SUM', safe_mutation_underflow=UNDERFLOW)
    B = 24
    start = list(E._world()[1])
    e, batch = _master_engine(spec, B)
    try:
        runs = []
        for _ in range(2):
            m = EngineESMaster(spec, e, seed=3, thetas=start)
            after = []
            for g in (1, 2):
                m.step(batch)
                assert m.n_parents == 2 and m.last['sigma'] == 0.01
                after.append(_parents_now(e, m.n_parents))
            runs.append(after)
            e.es_free()
        for g in range(2):
            assert np.array_equal(_bits(runs[0][g]), _bits(runs[1][g])), g
        assert not np.array_equal(runs[0][0], runs[0][1])
        e.es_create(3, 1)
        e.es_set_mutation_divide()
        e.es_set_parents(start)
        n_parents = 3
        for g in (1, 2):
            e.set_batch(*batch)
            po = draw_parents(3, g, spec.n_pairs, n_parents)
            e.es_sensitivity(sorted(set(int(p) for p in po)), min(B, spec.batch_size), UNDERFLOW)
            fit = e.es_evaluate(g, 0, spec.n_pairs, 0.01, po)
            order = e.es_select(fit, 2)
            e.es_advance(g, 0.01, po, order, 0)
            n_parents = 2
            assert np.array_equal(_bits(_parents_now(e, 2)), _bits(runs[0][g - 1])), g
    finally:
        e.close()


def test_master_vector(tmp_path):
    """EngineESMaster with SM-VECTOR and a .npy file: the shared vector is the file's, clamped as Sensitivity.
    set_sensitivity does, it survives the advances, and the survivors are the formula's offspring over it."""
    from nicnes.es import EngineESMaster
    from nicnes.mutations import clamp_file
    dims, parents, table = E._world()
    raw = np.random.Generator(np.random.PCG64(5)).uniform(0.0, 40.0, dims.D).astype(np.float32)
    path = str(tmp_path / 'sens.npy')
    np.save(path, raw)
    spec = _spec('SM-VECTOR', safe_mutation_vector=path, safe_mutation_underflow=0.5)
    vec = clamp_file(torch.from_numpy(raw), 0.5).numpy()
    e, batch = _master_engine(spec, 24)
    try:
        m = EngineESMaster(spec, e, seed=3, thetas=list(parents))
        old = [p.copy() for p in parents]
        for g in (1, 2):
            m.step(batch)
            po, order = m.last['parent_of'], m.last['order']
            want = [_want(old, vec, int(i) >> 1, int(i) & 1, int(po[int(i) >> 1]), gen=g) for i in order]
            got = _parents_now(e, m.n_parents)
            assert np.array_equal(_bits(got), _bits(np.stack(want))), g
            assert np.array_equal(_bits(e.es_sensitivity_row(0)), _bits(vec))
            old = [r.copy() for r in got]
    finally:
        e.close()


@pytest.mark.parametrize('mutation,mode', [('', 'plain'), ('SM-PROPORTIONAL', 'scale')])
def test_master_other_mutations_keep_their_bits(mutation, mode):
    """The plain and SM-PROPORTIONAL masters against tests/es_ref.Replay, as before the divide mode existed."""
    from nicnes.es import EngineESMaster
    dims, parents, table = E._world()
    spec = _spec(mutation)
    e, batch = _master_engine(spec, 24)
    try:
        m = EngineESMaster(spec, e, seed=3, thetas=list(parents))
        rep = R.Replay(spec, list(parents), table, SEED, dims, seed=3, mode=mode)
        for g in (1, 2):
            m.step(batch)
            parent_of, _, sigma = rep.generation(m.last['fitness'], [])
            assert np.array_equal(m.last['parent_of'], parent_of) and sigma == m.last['sigma']
            assert m.n_parents == len(rep.parents)
            assert np.array_equal(_bits(_parents_now(e, m.n_parents)), _bits(np.stack(rep.parents))), g
    finally:
        e.close()


def test_refusals():
    import nicnes
    dims, parents, table = E._world()
    B = 8
    fc, gts, df, n = E._workload(B)
    e = E._engine(B)
    try:
        e.es_set_parents(parents)
        e.es_set_mutation_divide()
        with pytest.raises(nicnes.NicnesError, match='invalid'):          # no batch held
            e.es_sensitivity([0], 1, UNDERFLOW)
        keys, vals = nicnes.df_table_arrays(df)
        e.set_df_table(keys, vals, np.log(float(n)))
        e.set_batch(fc, gts)
        for slots, rows, uf in (([0], 0, UNDERFLOW), ([0], B + 1, UNDERFLOW), ([0], B, 0.0), ([0], B, -1.0), ([3], B, UNDERFLOW),
                                ([0, -1], B, UNDERFLOW)):
            with pytest.raises(nicnes.NicnesError, match='invalid'):
                e.es_sensitivity(slots, rows, uf)
        # divide without any sensitivity: refused before anything is enqueued
        sentinel = torch.full((2, 2), -7.0, dtype=torch.float64, device=e.device)
        with pytest.raises(nicnes.NicnesError, match='no valid sensitivity'):
            e.es_evaluate(GEN, 0, 2, SIGMA, [0, 2], fitness_out=sentinel)
        with pytest.raises(nicnes.NicnesError, match='no valid sensitivity'):
            e.es_offspring(GEN, 0, 0, SIGMA, 0)
        order = torch.zeros(1, dtype=torch.int32, device=e.device)
        with pytest.raises(nicnes.NicnesError, match='no valid sensitivity'):
            e.es_advance(GEN, SIGMA, [0], order, 0)
        torch.cuda.synchronize()
        assert (sentinel.cpu().numpy() == -7.0).all()
        assert np.array_equal(e.es_row(0).cpu().numpy(), parents[0])
        with pytest.raises(nicnes.NicnesError, match='not supported'):
            e.es_set_mutation(3)
        e.es_sensitivity([0], B, UNDERFLOW)
        e.es_evaluate(GEN, 0, 1, SIGMA, [0], fitness_out=sentinel[:1])
        # a new ES state: no table, the plain mode
        e.es_free()
        e.es_create(6, 2)
        e.es_set_parents(parents)
        with pytest.raises(nicnes.NicnesError, match='invalid'):
            e.es_sensitivity_row(0)
        got = e.es_offspring(GEN, 0, 0, SIGMA, 2)
        assert np.array_equal(_bits(got), _bits(R.offspring(parents[2], table, E._idx(0), SIGMA, 0, 'plain')))
    finally:
        e.close()
