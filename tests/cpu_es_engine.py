"""Test helper: the es_* surface of nicnes.Engine that nicnes.es.EngineESMaster calls, in numpy, from tests/es_ref.py (the
host restatement of an offspring, the selection) and the oracle's decode and scorer on tests/cpu_engine.py's tiny workload,
so the rank logic of EngineESMaster runs over gloo without a GPU."""
import numpy as np
import torch

from oracle import cider_ref as CR
from oracle import oracle as O
from tests import es_ref as R
from tests.cpu_engine import _Cfg


class OracleESEngine:
    """nan_at = (generation, pair): that pair's fitness comes back NaN from whichever rank's shard holds it (a decode
    fault's NaN fitness)."""

    def __init__(self, dims, fc, gts, df, ref_len_raw, table, max_members, noise_seed=0, nan_at=None):
        self.device = torch.device('cpu')
        self.dims, self.D = dims, dims.D
        self.cfg = _Cfg(dims)
        self.cfg.max_members = int(max_members)
        self.fc, self.gts, self.table, self.seed = fc, gts, table, noise_seed
        self.scorer = CR.CiderDOracle(df, ref_len_raw)
        self.nan_at = nan_at
        self.mode = 'plain'
        self.parents, self.elites = [], {}
        self.theta32 = None
        self.decode = ('fused', 0)
        self.evaluated = []                                # (generation, pair_begin, count) of every es_evaluate

    # ---- the calls of EngineESMaster.__init__
    def es_create(self, max_parents, max_elites=1):
        self.max_parents, self.max_elites = int(max_parents), int(max_elites)

    def es_set_mutation(self, mode='plain'):
        self.mode = mode

    def es_set_decode(self, mode='fused', S=0):
        self.decode = (mode, int(S))

    def set_fitness_mode(self, fitness):
        assert fitness == 'greedy'

    def es_set_parents(self, thetas):
        self.parents = [np.asarray(t, np.float32).copy() for t in thetas]

    # ---- a generation
    def set_batch(self, fc, gts):
        self.fc, self.gts = np.asarray(fc, np.float32), gts

    def _idx(self, generation, pair):
        return O.noise_index(self.seed, generation, pair, self.table.size, self.D)

    def _child(self, generation, pair, sign, sigma, parent):
        return R.offspring(self.parents[parent], self.table, self._idx(generation, pair), np.float32(sigma), sign, self.mode)

    def es_evaluate(self, generation, pair_begin, count, sigma, parent_of, fitness_out=None):
        assert len(parent_of) == count
        self.evaluated.append((int(generation), int(pair_begin), int(count)))
        out = torch.empty((count, 2), dtype=torch.float64)
        for k in range(count):
            for s in range(2):
                seq, _, _ = O.decode(self.dims, self._child(generation, pair_begin + k, s, sigma, int(parent_of[k])), self.fc)
                out[k, s] = CR.rollout_fitness(self.scorer, seq, self.gts)[0]
            if self.nan_at == (generation, pair_begin + k):
                out[k, 1] = float('nan')
        return out

    def es_select(self, fitness, n_keep):
        return torch.from_numpy(R.select(fitness.numpy(), n_keep))

    def es_load_theta(self, slot, table='parents'):
        self.theta32 = (self.parents[slot] if table == 'parents' else self.elites[slot]).copy()

    def es_set_elite(self, elite_slot, slot, table='parents'):
        self.elites[elite_slot] = (self.parents[slot] if table == 'parents' else self.elites[slot]).copy()

    def es_advance(self, generation, sigma, parent_of, order, n_front=0):
        new = [self.elites[i].copy() for i in range(n_front)]
        for i in order.numpy():
            new.append(self._child(generation, int(i) >> 1, int(i) & 1, sigma, int(parent_of[int(i) >> 1])))
        self.parents = new

    def es_row(self, slot, table='parents'):
        return torch.from_numpy((self.parents[slot] if table == 'parents' else self.elites[slot]).copy())


class ScriptedValidator:
    """accuracy() of whatever theta the engine holds: a fixed function of its first weights, and a count of the calls."""

    def __init__(self, engine):
        self.engine, self.calls = engine, 0

    def accuracy(self):
        self.calls += 1
        return float(np.abs(self.engine.theta32[:64].astype(np.float64)).sum())
