"""Test helper: tests/cpu_es_engine.OracleESEngine with the divide mutation of SM-G-SUM / SM-VECTOR (the es_sensitivity /
es_set_sensitivity surface nicnes.es.EngineESMaster calls), in numpy from tests/es_safe_ref.py, and a record of every es_*
call in the order it was made. The sensitivity is oracle/sensitivity_ref.py's, with calc_sensitivity's clamp."""
import numpy as np

from tests import es_safe_ref as SRF
from tests.cpu_es_engine import OracleESEngine


class SafeOracleESEngine(OracleESEngine):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.calls = []                    # (name, args) of the es_* calls a generation makes, in order
        self.sens = {}                     # parent slot -> its sensitivity; valid while the slot's row stands
        self.shared = None

    @property
    def B(self):
        return int(np.asarray(self.fc).shape[0])

    def es_set_mutation(self, mode='plain'):
        assert mode in ('plain', 'scale')
        self.calls.append(('es_set_mutation', mode))
        super().es_set_mutation(mode)

    def es_set_mutation_divide(self):
        self.calls.append(('es_set_mutation_divide', None))
        self.mode = 'divide'

    def es_set_parents(self, thetas):
        super().es_set_parents(thetas)
        self.sens = {}

    def es_sensitivity(self, slots, rows, underflow):
        slots = [int(s) for s in slots]
        self.calls.append(('es_sensitivity', (tuple(slots), int(rows), float(underflow))))
        assert 1 <= rows <= self.B and underflow > 0 and all(0 <= s < len(self.parents) for s in slots)
        self.shared = None
        for s in slots:
            self.sens[s] = SRF.oracle_sensitivity(self.dims, self.parents[s], np.asarray(self.fc, np.float32)[:rows],
                                                  underflow)

    def es_set_sensitivity(self, vec, slot=None):
        v = np.asarray(vec.numpy() if hasattr(vec, 'numpy') else vec, np.float32).copy()
        self.calls.append(('es_set_sensitivity', slot))
        if slot is None:
            self.shared = v
        else:
            self.shared = None
            self.sens[int(slot)] = v

    def es_sensitivity_row(self, slot):
        import torch
        return torch.from_numpy((self.shared if self.shared is not None else self.sens[int(slot)]).copy())

    def _child(self, generation, pair, sign, sigma, parent):
        if self.mode != 'divide':
            return super()._child(generation, pair, sign, sigma, parent)
        s = self.shared if self.shared is not None else self.sens[parent]     # KeyError: no valid sensitivity
        return SRF.offspring(self.parents[parent], self.table, self._idx(generation, pair), np.float32(sigma), sign,
                             'divide', s)

    def es_evaluate(self, generation, pair_begin, count, sigma, parent_of, fitness_out=None):
        self.calls.append(('es_evaluate', (int(generation), int(pair_begin), int(count))))
        return super().es_evaluate(generation, pair_begin, count, sigma, parent_of, fitness_out)

    def es_advance(self, generation, sigma, parent_of, order, n_front=0):
        self.calls.append(('es_advance', int(generation)))
        super().es_advance(generation, sigma, parent_of, order, n_front)
        self.sens = {}                     # the rows were the old table's; a shared vector stays
