"""GPU: EngineMaster with a Validator on the HIP engine, end to end: every iteration's stats row carries the
validation CIDEr of the theta that iteration evaluated (the pre-update theta, scored by Split.evaluate on a resident
split), the best theta is written on improvement, and the run's numbers are those of the same run without a validator
(validation reads theta and touches nothing the evaluates use)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from oracle import oracle as O          # noqa: E402

NOISE_LEN = 1 << 23


class _Labels:
    def __init__(self, gts):
        self.labels = np.concatenate(gts, 0)
        n = np.array([g.shape[0] for g in gts])
        self.label_start_ix = np.cumsum(np.concatenate([[0], n[:-1]])) + 1      # 1-based, inclusive
        self.label_end_ix = self.label_start_ix + n - 1


class _Loader:
    """the surface of nicnes.data.CocoFcDataLoader a Validator and the master read, over arrays in memory"""

    def __init__(self, fc, gts, n_val):
        self.fc, self.gts, self.pos, self.seq_length = fc, gts, 0, 16
        self.labels = _Labels(gts)
        n = len(gts)
        self.info = {'images': [{'id': 1000 + i} for i in range(n)]}
        self.ix_to_word = {str(i): 'w%d' % i for i in range(1, 9488)}
        self.split_ix = {'val': list(range(n - n_val, n)), 'train': list(range(n - n_val))}

    def fc_feature(self, ix):
        return self.fc[ix]

    def get_batch(self, split, batch_size=None):
        tr = self.split_ix['train']
        ix = [tr[(self.pos + k) % len(tr)] for k in range(batch_size)]
        self.pos += batch_size
        return {'fc_feats': np.repeat(self.fc[ix], 5, axis=0), 'gts': [self.gts[i] for i in ix]}


def _spec(P):
    from nicnes import config as C
    exp = {'algorithm': 'nic_nes', 'nb_offspring': P,
           'config': {'noise_stdev': 0.01, 'batch_size': 8, 'l2coeff': 1e-3, 'snapshot_freq': 0, 'single_batch': True,
                      'patience': 5, 'num_val_items': 9},
           'policy_options': {'net': 'fc_caption', 'fitness': 'greedy', 'model_options': {}},
           'optimizer_options': {'type': 'adam', 'args': {'stepsize': 1e-2}}}
    return C.ExperimentSpec(exp)


def test_master_records_the_validation_score_of_the_evaluated_theta(tmp_path):
    import nicnes
    import nicnes.synthetic as S
    from nicnes import master as M
    from nicnes.validation import Validator
    dims = O.Dims()
    theta = O.make_theta(dims, 0, 4.0, 0.1)
    fc = np.random.Generator(np.random.PCG64(1234)).standard_normal((27, dims.F)).astype(np.float32)
    base, _, _ = O.decode(dims, theta, fc)
    gts, df, n = S.build_references(base, dims.vocab_size, seed=9, n_refs=5, df_sets=128)
    table = O.noise_table(NOISE_LEN, 123)
    P = 4
    runs = {}
    for name in ('plain', 'validated'):
        e = nicnes.Engine(max_batch=8, max_members=P, noise_len=NOISE_LEN, noise_seed=0)
        try:
            e.set_noise_table(table)
            keys, vals = nicnes.df_table_arrays(df)
            e.set_df_table(keys, vals, np.log(float(n)))
            loader = _Loader(fc, gts, n_val=11)
            spec = _spec(P)
            v = Validator(e, loader, 'val', spec.config.num_val_items) if name == 'validated' else None
            m = M.EngineMaster(spec, e, log_dir=str(tmp_path / name), theta=theta, validator=v)
            thetas, scores = [], []
            for k in range(1, 4):                                   # the theta each iteration evaluates, and its score
                thetas.append(e.theta()[0].clone())
                if v is not None:
                    scores.append(v.split.evaluate()['CIDEr'])
                m.run(loader, max_iterations=k)
            runs[name] = m.stats, e.theta()[0].cpu().numpy()
            if v is not None:
                assert v.image_ids == [1000 + i for i in range(16, 25)]         # the first 9 of the 11 val images
                assert [r['val_score'] for r in m.stats] == scores
                assert all(np.isfinite(scores)) and scores[0] > 0         # the references derive from theta's captions
                best = max(scores)
                assert [r['best_val_score'] for r in m.stats] == [max(scores[:k + 1]) for k in range(3)]
                path = os.path.join(str(tmp_path / name), 'models', 'best', 'best_elite', '0_0_elite.pth')
                assert m.best_elites == [(path, best)]
                from nicnes.nes import vector_from_state_dict, param_shapes
                saved = vector_from_state_dict(torch.load(path, weights_only=True), param_shapes(e))
                want = thetas[scores.index(best)].cpu()
                assert torch.equal(saved.double(), want if scores.index(best) else want.float().double())
                stats, preds = v.eval_split(incl_gts=True)
                assert len(preds) == 9 and all(len(p['gts']) == 5 for p in preds)
                assert stats['CIDEr'] == v.split.evaluate()['CIDEr']
        finally:
            e.close()
    for a, b in zip(*[r[0] for r in runs.values()]):
        assert all(a[k] == b[k] for k in a if k != 'step_time'), (a, b)
    assert np.array_equal(runs['plain'][1], runs['validated'][1])
