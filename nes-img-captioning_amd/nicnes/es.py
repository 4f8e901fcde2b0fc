"""nic_es, the truncation-selection GA of the reference's src/algorithm/nic_es/, on the engine.

  ESExperimentSpec     the mscoco_es.json surface (ESExperiment, nic_es/experiment.py:13-20)
  ESTask / ESResult    nic_es_master.py:27-34, with parent slots and (pair, sign) ids where the reference has paths
  draw_parents         the parent of every offspring pair (ESWorker.fitness, nic_es_worker.py:150-162), counter-based
  Podium               tools/podium.py on scores and slots
  EngineESMaster.run   ESMaster.run_master + ESIteration.record_parents (nic_es_master.py:55-148, nic_es/iteration.py)

Where the engine departs from the reference (DESIGN.md, section "nic_es"):
* The unit is the antithetic pair: pair k of a generation gives offspring 2k = parent + delta' and 2k + 1 = parent -
  delta' (ESWorker.fitness draws one-sided offspring; delta is symmetric, so the population has the same
  distribution), and nb_offspring must be even.
* An offspring is (parent slot, noise index, sign), never a file: its theta exists in LDS during the decode, and only
  the selected offspring are written, on the device (Engine.es_advance).
* The parents of a generation are drawn by a counter-based hash, then sorted across the pair ids (pairs are
  exchangeable), so members that share a parent launch next to each other.
* From zero, population_size host-initialised parents are perturbed; the reference makes generation 1's offspring
  fresh random models (ESIteration.init_from_zero keeps the parents None).
"""
import os
import time
from collections import namedtuple

import numpy as np

from .config import (Config, PolicyOptions, ModelOptions, NotSupported, GREEDY_FITNESS, load_experiment,
                     _model_opt_fields)

result_fields = ['worker_id', 'evaluated_model_id', 'fitness', 'evaluated_model', 'eval_return', 'mem_usage',
                 'evaluated_cand', 'evaluated_cand_id', 'score']
ESResult = namedtuple('ESResult', field_names=result_fields, defaults=(None,) * len(result_fields))

es_task_fields = ['elite', 'population', 'batch_data', 'parents', 'noise_stdev', 'log_dir', 'elites', 'ref_batch']
ESTask = namedtuple('ESTask', field_names=es_task_fields, defaults=(None,) * len(es_task_fields))

MASK64 = (1 << 64) - 1
_PARENT_STREAM = 0xbb67ae8584caa73b      # keeps the parent draws apart from the noise-index and sample-draw hashes


def splitmix64(x):
    """include/nicnes_math.h nn_splitmix64."""
    z = (x + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


class ESExperimentSpec:
    """What the engine needs from an mscoco_es.json-shaped experiment. ExperimentSpec stays the nic_nes reader."""

    def __init__(self, exp, vocab_size=9487, seq_length=16):
        exp = load_experiment(exp)
        if exp.get('algorithm') != 'nic_es':
            raise NotSupported('algorithm %r: ESExperimentSpec reads nic_es experiments' % exp.get('algorithm'))
        if exp.get('dataset', 'mscoco') != 'mscoco':
            raise NotSupported('dataset %r: the engine implements the mscoco fc_caption path' % exp.get('dataset'))
        self.exp = exp
        self.config = Config(**exp['config'])
        po = dict(exp['policy_options'])
        self.policy_options = PolicyOptions(**po)
        mo = dict(po.get('model_options', {}))
        mo.setdefault('vocab_size', vocab_size)
        mo.setdefault('seq_length', seq_length)
        self.model_options = ModelOptions(**{k: v for k, v in mo.items() if k in _model_opt_fields})
        self.nb_offspring = int(exp['nb_offspring'])
        self.population_size = int(exp.get('population_size', self.nb_offspring))     # experiment.py:16
        self.num_elites = int(exp['num_elites'])
        self.num_elite_cands = int(exp['num_elite_cands'])
        self.selection = exp.get('selection', 'uniform')
        self.tournament_size = exp.get('tournament_size')
        self._validate()

    def _validate(self):
        po, mo = self.policy_options, self.model_options
        if po.net != 'fc_caption':
            raise NotSupported('net %r: the engine implements fc_caption' % po.net)
        if self.fitness not in GREEDY_FITNESS:
            raise NotSupported('fitness %r: nic_es on the engine implements %s' % (po.fitness, ', '.join(GREEDY_FITNESS)))
        if po.vbn or mo.vbn_e or mo.layer_n:
            raise NotSupported('virtual batch norm / layer norm are not implemented by the engine')
        if self.mutation not in ('', 'SM-PROPORTIONAL'):
            raise NotSupported('safe_mutations %r: nic_es on the engine implements plain and SM-PROPORTIONAL'
                               % self.mutation)
        if self.nb_offspring < 2 or self.nb_offspring % 2:
            raise NotSupported('nb_offspring %d: the engine evaluates antithetic pairs, so it must be even'
                               % self.nb_offspring)
        if self.selection not in ('uniform', 'tournament'):
            raise NotSupported("selection %r: 'uniform' or 'tournament'" % (self.selection,))
        if self.selection == 'tournament' and not (self.tournament_size and int(self.tournament_size) >= 1):
            raise NotSupported('tournament selection needs tournament_size >= 1')
        if not 0 <= self.num_elites < self.population_size:
            raise NotSupported('num_elites must be in [0, population_size)')
        if self.population_size - self.num_elites > self.nb_offspring:
            raise NotSupported('population_size - num_elites parents cannot be selected from nb_offspring offspring')
        if not 0 <= self.num_elite_cands <= self.population_size - self.num_elites:
            raise NotSupported('num_elite_cands must be in [0, population_size - num_elites]')

    @property
    def fitness(self):
        return self.policy_options.fitness or 'greedy'

    @property
    def mutation(self):
        return self.model_options.safe_mutations or ''

    @property
    def n_pairs(self):
        return self.nb_offspring // 2

    @property
    def sigma(self):
        return float(self.config.noise_stdev)

    @property
    def batch_size(self):
        return int(self.config.batch_size)

    def engine_kwargs(self, noise_len=1 << 27, noise_seed=0, max_batch=None):
        mo = self.model_options
        return dict(vocab_size=int(mo.vocab_size), input_encoding_size=int(mo.input_encoding_size or 128),
                    rnn_size=int(mo.rnn_size or 128), fc_feat_size=int(mo.fc_feat_size or 2048),
                    seq_length=int(mo.seq_length or 16), max_batch=int(max_batch or self.batch_size),
                    max_members=self.n_pairs, noise_len=int(noise_len), noise_seed=int(noise_seed))


def draw_parents(seed, generation, n_pairs, n_parents, selection='uniform', tournament_size=None, sort_parents=True):
    """The parent slot of each of a generation's n_pairs pairs: int32 [n_pairs] in [0, n_parents).

    uniform: one draw per pair (rs.randint, nic_es_worker.py:161). tournament: the lowest of k = min(tournament_size,
    n_parents) distinct draws (rs.choice(..., replace=False).min(), :150-157: the parents are ordered best first).
    Every draw is splitmix64 of (seed, generation, pair, draw number): any rank computes the same parents with no
    communication. With sort_parents the draws are then sorted ascending across the pair ids."""
    if n_parents < 1 or n_pairs < 0:
        raise ValueError('n_parents >= 1 and n_pairs >= 0 needed')
    if selection not in ('uniform', 'tournament'):
        raise ValueError('selection %r' % (selection,))
    out = np.empty(n_pairs, np.int32)
    for k in range(n_pairs):
        key = splitmix64((seed ^ _PARENT_STREAM ^ (((generation << 32) | (k & 0xffffffff)) & MASK64)) & MASK64)
        if selection == 'uniform':
            out[k] = splitmix64(key) % n_parents
        else:
            out[k] = min(tournament_draws(key, n_parents, tournament_size))
    if sort_parents:
        out.sort(kind='stable')
    return out


def tournament_draws(key, n_parents, tournament_size):
    """min(tournament_size, n_parents) distinct parent slots: a partial Fisher-Yates over range(n_parents), draw t
    from splitmix64(key ^ t)."""
    k = min(int(tournament_size), n_parents)
    moved = {}                                   # the permutation's entries that differ from the identity
    picks = []
    for t in range(k):
        r = t + splitmix64((key ^ t) & MASK64) % (n_parents - t)
        vr, vt = moved.get(r, r), moved.get(t, t)
        picks.append(vr)
        moved[r] = vt
    return picks


class Podium:
    """tools/podium.py on scores and slots: the num_elites best validated elites so far, best first, and whether a
    generation added one ('good') or not ('bad', counted against the patience).

    An elite is (key, score); key is whatever names the candidate (the engine master uses 'g<generation>c<i>'). After
    record_elites, `moves` lists how the elite table follows: (place, 'elites', old place) for an elite that moved
    down, (place, 'parents', slot) for a new one, bottom place first, so applying them in order never reads a row
    already overwritten."""

    def __init__(self, num_elites):
        self.num_elites = int(num_elites)
        self._best = []                          # [(key, score)] best first, at most num_elites
        self._bad_generation = True
        self.moves = []

    def record_elites(self, cands):
        """cands: [(key, score, parent_slot)] of this generation's validated candidates. The order is podium.py:41-43:
        the elites held, then the candidates, sorted by score with a stable sort, so a tie keeps the one held (and
        the earlier candidate)."""
        held = [(k, sc, ('elites', i)) for i, (k, sc) in enumerate(self._best)]
        new = [(k, float(sc), ('parents', int(slot))) for k, sc, slot in cands]
        ranked = sorted(held + new, key=lambda c: c[1], reverse=True)[:self.num_elites]
        self.moves = []
        for place in range(len(ranked) - 1, -1, -1):
            table, src = ranked[place][2]
            if table == 'parents':
                self._bad_generation = False      # a new elite on the podium (podium.py:53-57)
                self.moves.append((place, 'parents', src))
            elif src != place:
                self.moves.append((place, 'elites', src))
        self._best = [(k, sc) for k, sc, _ in ranked]
        return self.moves

    def is_bad_generation(self):
        status = self._bad_generation
        self._bad_generation = True
        return status

    def best_elites(self):
        return list(self._best)


class EngineESMaster:
    """ESMaster.run_master on one engine. Per generation (nic_es_master.py:68-127 and ESIteration.record_parents):
    evaluate the offspring; validate the previous generation's elite candidates; update the podium and the patience /
    schedule curriculum; select population_size - num_elites parents, the first num_elite_cands of them being the next
    candidates; the new parents are the podium's elites + the selected."""

    def __init__(self, spec, engine, validator=None, log_dir=None, seed=0, thetas=None, from_single=None,
                 sort_parents=True):
        from .master import Schedule
        self.spec, self.e, self.validator = spec, engine, validator
        self.log_dir = log_dir or spec.config.log_dir or 'logs/nices'
        self.seed = int(seed)
        self.sort_parents = bool(sort_parents)
        self.sched = Schedule(spec.config, spec.nb_offspring)
        self.podium = Podium(spec.num_elites)
        self.stats = []
        if spec.n_pairs > engine.cfg.max_members:
            raise ValueError('the engine needs max_members >= nb_offspring / 2 = %d' % spec.n_pairs)
        engine.es_create(max(spec.population_size, 1), max(spec.num_elites, 1))
        engine.es_set_mutation('scale' if spec.mutation == 'SM-PROPORTIONAL' else 'plain')
        engine.set_fitness_mode(spec.fitness)
        parents = self._initial_parents(thetas, from_single)
        engine.es_set_parents(parents)
        self.n_parents = len(parents)
        # the first candidates (init_from_singles: the given models; init_from_zero: fresh ones, here the first parents)
        self.cands = list(range(min(spec.num_elite_cands, self.n_parents)))

    def _initial_parents(self, thetas, from_single):
        from .nes import param_shapes, vector_from_state_dict, _load_state
        if thetas is not None:
            return [np.asarray(t, np.float32) for t in thetas]
        if from_single:
            paths = [from_single] if isinstance(from_single, str) else list(from_single)
            shapes = param_shapes(self.e)
            return [np.asarray(vector_from_state_dict(_load_state(p), shapes), np.float32) for p in paths]
        return [self.initial_theta(self.seed, i) for i in range(self.spec.population_size)]

    def initial_theta(self, seed, i):
        """PolicyNet.initialize_params (nets.py:62-69) for parent i of a run from zero: xavier_normal_ weights, zero
        biases, from numpy PCG64 so every host draws the same parents."""
        rng = np.random.Generator(np.random.PCG64([int(seed), int(i)]))
        off, D = self.e.offsets, self.e.D
        cfg = self.e.cfg
        V1, E, R, F = cfg.vocab_size + 1, cfg.input_encoding_size, cfg.rnn_size, cfg.fc_feat_size
        theta = np.zeros(D, np.float32)
        for t, shp in ((0, (E, F)), (2, (V1, E)), (3, (V1, R)), (5, (5 * R, E)), (7, (5 * R, R))):
            std = np.sqrt(2.0 / float(shp[0] + shp[1]))
            n = shp[0] * shp[1]
            theta[off[t]: off[t] + n] = (rng.standard_normal(n) * std).astype(np.float32)
        return theta

    # -------------------------------------------------------------------------------------------------
    def parents_of(self, generation):
        return draw_parents(self.seed, generation, self.spec.n_pairs, self.n_parents, self.spec.selection,
                            self.spec.tournament_size, self.sort_parents)

    def _validate_candidates(self, generation):
        """Steps 2 and 3: the validation score of each candidate row (ESWorker.accuracy), the podium, the elite table."""
        e = self.e
        scored = []
        if self.validator is not None:
            for i, slot in enumerate(self.cands):
                e.es_load_theta(slot)
                scored.append(('g%dc%d' % (generation, i), float(self.validator.accuracy()), slot))
        for place, table, src in self.podium.record_elites(scored):
            e.es_set_elite(place, src, table)
        return scored

    def step(self, batch):
        """One generation on `batch` ((fc, gts), or the reference's batch dict). Returns its stats record."""
        import torch
        from ._lib import DecodeFault
        from .nes import engine_batch
        e, spec, sc = self.e, self.spec, self.sched
        t0 = time.time()
        sc.incr_iteration()
        g = sc.iteration
        sigma = sc.noise_stdev
        fc, gts = engine_batch(batch, e) if isinstance(batch, dict) else batch
        e.set_batch(fc, gts)
        parent_of = self.parents_of(g)
        fit = e.es_evaluate(g, 0, spec.n_pairs, sigma, parent_of)                                    # 1
        n_keep = spec.population_size - spec.num_elites
        order = e.es_select(fit, n_keep)                      # 4, enqueued behind the evaluate: no host sync between
        fit_h = fit.cpu().numpy()
        if np.isnan(fit_h).any():                             # nothing of this generation is recorded
            raise DecodeFault('generation %d: NaN fitness; the parents, podium and candidates are those before it' % g)
        scored = self._validate_candidates(g)                                                        # 2, 3
        sc.record_generation(self.podium.is_bad_generation())
        n_front = len(self.podium.best_elites())
        e.es_advance(g, sigma, parent_of, order, n_front)                                            # 5
        self.n_parents = n_front + n_keep
        self.cands = [n_front + i for i in range(spec.num_elite_cands)]
        self.last = {'generation': g, 'parent_of': parent_of, 'fitness': fit_h, 'order': order.cpu().numpy(),
                     'validated': scored, 'sigma': sigma}
        best = self.podium.best_elites()
        rec = {'iter': g, 'score_mean': float(fit_h.mean()), 'score_max': float(fit_h.max()),
               'score_min': float(fit_h.min()), 'noise_stdev': sc.noise_stdev, 'batch_size': sc.batch_size,
               'best_val_score': best[0][1] if best else None, 'step_time': time.time() - t0}
        self.stats.append(rec)
        freq = spec.config.snapshot_freq
        if freq and g % freq == 0:
            self.save_snapshot()
        if torch.cuda.is_available():
            torch.cuda.current_stream(e.device).synchronize()
        return rec

    def run(self, batches, generations=None):
        """batches: an iterable of batches (or a callable (batch_size) -> iterable, re-made when the curriculum changes
        the batch size, as ESMaster.run_master breaks out to a new trainloader)."""
        limit = generations if generations is not None else self.spec.config.max_nb_iterations
        done = 0
        while not limit or done < limit:
            stream = batches(self.sched.batch_size) if callable(batches) else batches
            progressed = False
            for batch in stream:
                self.step(batch)
                done += 1
                progressed = True
                if (limit and done >= limit) or self.sched.patience_reached or self.sched.schedule_reached:
                    break
            if not progressed or not callable(batches):
                break
        return self.stats

    # -------------------------------------------------------------------------------------------------
    def save_snapshot(self):
        """Parents, elite candidates and best elites as .pth state dicts in the reference's layout
        (models/offspring/0_i_parent_params.pth, models/elite/0_i_elite_params.pth, models/best/best_elite/0_i_elite.pth;
        ESIteration, Podium). Resuming from infos is not implemented."""
        import torch
        from .nes import param_shapes, state_dict_from_vector
        shapes = param_shapes(self.e)
        md = os.path.join(self.log_dir, 'models')
        out = {'parents': [], 'elites_to_evaluate': [], 'best_elites': []}

        def save(sub, name, row, table):
            d = os.path.join(md, sub)
            os.makedirs(d, exist_ok=True)
            path = os.path.join(d, name)
            torch.save(state_dict_from_vector(self.e.es_row(row, table), shapes), path)
            return path
        for i in range(self.n_parents):
            out['parents'].append((i, save('offspring', '0_%d_parent_params.pth' % i, i, 'parents')))
        for i, slot in enumerate(self.cands):
            out['elites_to_evaluate'].append((i, save('elite', '0_%d_elite_params.pth' % i, slot, 'parents')))
        for i, (_, score) in enumerate(self.podium.best_elites()):
            out['best_elites'].append((save(os.path.join('best', 'best_elite'), '0_%d_elite.pth' % i, i, 'elites'), score))
        return out
