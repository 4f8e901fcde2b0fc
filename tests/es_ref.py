"""Host restatement of the engine's nic_es generation step (tests/test_gpu_es.py), from oracle pieces and nicnes.es.Podium.

An offspring is (parent, noise index, sign): theta_p + delta' or theta_p - delta' in fp32, delta' = fp32(sigma z) (plain)
or fp32(fp32(sigma z) * a_p) with a_p = |theta_p|, mean|theta_p| at exact zeros (SM-PROPORTIONAL, nets.py:107-111)."""
import types

import numpy as np

from oracle import oracle as O


def parent_mean(theta):
    """The engine's mean|theta_p|: an fp64 sum, one rounding to fp32."""
    return np.float32(np.abs(theta.astype(np.float64)).mean())


def mean_off_boundary(theta, rel=1e-10):
    """True when the fp64 mean is further than rel (relative) from the midpoint between two fp32 values: another fp64
    summation order (error far below rel at these sizes) then rounds to the same fp32."""
    m = float(np.abs(theta.astype(np.float64)).mean())
    f = np.float32(m)
    lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
    mids = (0.5 * (float(lo) + float(f)), 0.5 * (float(f) + float(hi)))
    return min(abs(m - mids[0]), abs(m - mids[1])) > rel * m


def delta(theta_p, table, idx, sigma, mode):
    d = np.float32(sigma) * table[idx: idx + theta_p.size]
    if mode == 'scale':
        a = np.where(theta_p == 0, parent_mean(theta_p), np.abs(theta_p)).astype(np.float32)
        d = d * a
    return d.astype(np.float32)


def offspring(theta_p, table, idx, sigma, sign, mode):
    """sign 0: +, 1: - (offspring id = 2 pair + sign)."""
    d = delta(theta_p, table, idx, sigma, mode)
    return (theta_p - d) if sign else (theta_p + d)


def select(fitness, n_keep):
    """Offspring ids in descending fitness, ties to the lower id, NaN last, -0 == +0."""
    f = np.asarray(fitness, np.float64).ravel()
    nan = np.isnan(f)
    key = np.where(nan, 0.0, -f) + 0.0
    return np.lexsort((np.arange(f.size), key, nan))[:n_keep].astype(np.int32)


class FakeLoader:
    """The attributes nicnes.validation.Validator reads, over given fc rows and label rows."""

    def __init__(self, fc, gts, T=16):
        n = fc.shape[0]
        self._fc = fc
        self.seq_length = T
        self.split_ix = {'val': list(range(n))}
        self.info = {'images': [{'id': 1000 + i} for i in range(n)]}
        self.ix_to_word = {}
        rows = np.concatenate(gts, 0).astype(np.int32)
        ends = np.cumsum([g.shape[0] for g in gts])
        self.labels = types.SimpleNamespace(labels=rows, label_start_ix=ends - np.array([g.shape[0] for g in gts]) + 1,
                                            label_end_ix=ends)

    def fc_feature(self, ix):
        return self._fc[ix]


class Replay:
    """EngineESMaster's generations on the host: the same draw_parents, select, Podium and Schedule, numpy parents."""

    def __init__(self, spec, parents, table, noise_seed, dims, seed=0, mode='plain'):
        from nicnes.es import Podium
        from nicnes.master import Schedule
        self.spec, self.table, self.noise_seed, self.dims, self.seed, self.mode = spec, table, noise_seed, dims, seed, mode
        self.parents = [np.asarray(p, np.float32) for p in parents]
        self.elites = []                                   # theta of the podium's places
        self.podium = Podium(spec.num_elites)
        self.sched = Schedule(spec.config, spec.nb_offspring)
        self.cands = list(range(min(spec.num_elite_cands, len(self.parents))))

    def generation(self, fitness, val_scores):
        """fitness [pairs, 2] and the candidates' validation scores as the engine gave them. Returns (parent_of, every
        offspring's theta as a function (pair, sign) -> theta, sigma)."""
        from nicnes.es import draw_parents
        spec, sc = self.spec, self.sched
        sc.incr_iteration()
        g, sigma = sc.iteration, sc.noise_stdev
        parent_of = draw_parents(self.seed, g, spec.n_pairs, len(self.parents), spec.selection, spec.tournament_size)
        old = self.parents

        def child(pair, sign):
            idx = O.noise_index(self.noise_seed, g, pair, self.table.size, self.dims.D)
            return offspring(old[parent_of[pair]], self.table, idx, sigma, sign, self.mode)
        scored = [('g%dc%d' % (g, i), val_scores[i], slot) for i, slot in enumerate(self.cands)]
        elites = list(self.elites) + [None] * (spec.num_elites - len(self.elites))
        for place, tab, src in self.podium.record_elites(scored):
            elites[place] = old[src] if tab == 'parents' else elites[src]
        self.elites = elites[:len(self.podium.best_elites())]
        sc.record_generation(self.podium.is_bad_generation())
        n_keep = spec.population_size - spec.num_elites
        order = select(fitness, n_keep)
        self.parents = list(self.elites) + [child(int(i) >> 1, int(i) & 1) for i in order]
        self.cands = [len(self.elites) + i for i in range(spec.num_elite_cands)]
        return parent_of, child, sigma
