"""nic_es, the truncation-selection GA of the reference's src/algorithm/nic_es/, on the engine.

  ESExperimentSpec     the mscoco_es.json surface (ESExperiment, nic_es/experiment.py:13-20)
  ESTask / ESResult    nic_es_master.py:27-34, with parent slots and (pair, sign) ids where the reference has paths
  draw_parents         the parent of every offspring pair (ESWorker.fitness, nic_es_worker.py:150-162), counter-based
  Podium               tools/podium.py on scores and slots
  EngineESMaster.run   ESMaster.run_master + ESIteration.record_parents (nic_es_master.py:55-148, nic_es/iteration.py)
  es_shard             the pairs of a generation a rank evaluates (ESMaster hands ESTasks to whichever worker is free)
  python -m nicnes.es  a run of an experiment JSON, alone or as one rank of a torchrun world (main)

Where the engine departs from the reference (DESIGN.md, section "nic_es"):
* The unit is the antithetic pair: pair k of a generation gives offspring 2k = parent + delta' and 2k + 1 = parent -
  delta' (ESWorker.fitness draws one-sided offspring; delta is symmetric, so the population has the same
  distribution), and nb_offspring must be even.
* An offspring is (parent slot, noise index, sign), never a file: its theta exists in LDS during the decode, and only
  the selected offspring are written, on the device (Engine.es_advance).
* The parents of a generation are drawn by a counter-based hash, then sorted across the pair ids (pairs are
  exchangeable), so members that share a parent launch next to each other.
* Over several ranks (EngineESMaster(rank=, world_size=)) every rank evaluates its own es_shard of the pairs, the
  fitness is gathered, and selection, podium, schedule and the advance run replicated on every rank: the parent and
  elite tables stay identical with no theta ever sent (the reference's workers write every offspring to a shared disk).
* SM-G-SUM: the sensitivity belongs to the parent, so a generation computes one vector per distinct parent drawn
  (Engine.es_sensitivity), replicated on every rank, before the evaluate; SM-VECTOR shares one vector among all parents.
* From zero, population_size host-initialised parents are perturbed; the reference makes generation 1's offspring
  fresh random models (ESIteration.init_from_zero keeps the parents None).
"""
import os
import time
from collections import namedtuple

import numpy as np

from .config import (Config, PolicyOptions, ModelOptions, NotSupported, GREEDY_FITNESS, load_experiment,
                     _model_opt_fields, is_wide)

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
        if is_wide(mo):
            raise NotSupported('nic_es is not implemented for models wider than 128 units (rnn_size %s, '
                               'input_encoding_size %s): nicnes_es_create refuses them'
                               % (mo.rnn_size, mo.input_encoding_size))
        if self.fitness not in GREEDY_FITNESS:
            raise NotSupported('fitness %r: nic_es on the engine implements %s' % (po.fitness, ', '.join(GREEDY_FITNESS)))
        if po.vbn or mo.vbn_e or mo.layer_n:
            raise NotSupported('virtual batch norm / layer norm are not implemented by the engine')
        if self.mutation == 'SM-G-ABS':
            raise NotSupported("SM-G-ABS: the reference's _calc_abs_sensitivity raises AttributeError "
                               "(self.nb_params on Sensitivity, safe_mutations.py:125)")
        if self.mutation not in ('', 'SM-PROPORTIONAL', 'SM-G-SUM', 'SM-VECTOR'):
            raise NotSupported('safe_mutations %r (Mutation, src/algorithm/nets.py:16-21)' % self.mutation)
        if self.mutation == 'SM-G-SUM' and not self.underflow > 0:
            raise NotSupported('SM-G-SUM needs safe_mutation_underflow > 0 (the reference divides by it)')
        if self.mutation == 'SM-VECTOR' and not mo.safe_mutation_vector:
            raise NotSupported('SM-VECTOR needs model_options.safe_mutation_vector')
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
    def underflow(self):
        """model_options.safe_mutation_underflow: the clamp of SM-G-SUM's sensitivity and of SM-VECTOR's file."""
        return float(self.model_options.safe_mutation_underflow or 0.0)

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


def es_shard(n_pairs, rank, world):
    """(begin, count) of the pairs rank `rank` of `world` evaluates (include/nicnes_math.h nn_es_shard): the first
    n_pairs % world ranks take n_pairs // world + 1 pairs, the rest n_pairs // world; contiguous, in rank order."""
    n_pairs, rank, world = int(n_pairs), int(rank), int(world)
    if world < 1 or not 0 <= rank < world:
        raise ValueError('rank %d of %d ranks' % (rank, world))
    if n_pairs < world:
        raise ValueError('%d pairs cannot be split over %d ranks: every rank needs a pair' % (n_pairs, world))
    q, r = divmod(n_pairs, world)
    return rank * q + min(rank, r), q + (1 if rank < r else 0)


def pad_shard(fit_local, n_pairs, world):
    """A rank's shard fitness [count, 2] padded with zeros to the largest share [ceil(n_pairs / world), 2]: what an
    all-gather of equal parts takes."""
    import torch
    pad = -(-int(n_pairs) // int(world))
    out = torch.zeros((pad, 2), dtype=fit_local.dtype, device=fit_local.device)
    out[:fit_local.shape[0]] = fit_local
    return out


def compact_shards(padded_all, n_pairs, world):
    """The gathered padded shares [world * pad, 2] -> the generation's fitness [n_pairs, 2] in pair order."""
    import torch
    pad = -(-int(n_pairs) // int(world))
    rows = padded_all.reshape(int(world), pad, 2)
    return torch.cat([rows[r, :es_shard(n_pairs, r, world)[1]] for r in range(int(world))], 0).contiguous()


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
    candidates; the new parents are the podium's elites + the selected.

    Over world_size ranks (one engine each) every rank runs the same generations: it evaluates its own es_shard of the
    pairs, the fitness is gathered (comm=None: torch.distributed on `group`, gloo or nccl; comm='engine': the engine's
    C-ABI communicator after Engine.comm_init), and everything after the gather is replicated, so every rank ends a
    generation with the same parents, elites, podium, candidates and schedule. Rank 0 holds the Validator; its scores
    reach the other ranks in one collective (they pass validator=True and never score). Snapshots are rank 0's.
    decode: Engine.es_set_decode's mode, or ('coop', S); the default is 'fused' on one rank and 'auto' over several,
    where a rank's share may no longer fill the GPU with one workgroup per pair and slab."""

    def __init__(self, spec, engine, validator=None, log_dir=None, seed=0, thetas=None, from_single=None,
                 sort_parents=True, rank=0, world_size=1, group=None, comm=None, decode=None):
        from .master import Schedule
        self.spec, self.e, self.validator = spec, engine, validator
        self.rank, self.world, self.group = int(rank), int(world_size), group
        if comm not in (None, 'engine'):
            raise ValueError("comm: None (torch.distributed) or 'engine' (the engine's RCCL communicator)")
        self.comm = comm
        self.shard = es_shard(spec.n_pairs, self.rank, self.world)
        if decode is None:
            decode = 'fused' if self.world == 1 else 'auto'
        self.decode = decode
        if decode != 'fused' or self.world > 1:       # (today's single-rank callers' engines are left untouched)
            engine.es_set_decode(*((decode,) if isinstance(decode, str) else tuple(decode)))
        self.log_dir = log_dir or spec.config.log_dir or 'logs/nices'
        self.seed = int(seed)
        self.sort_parents = bool(sort_parents)
        self.sched = Schedule(spec.config, spec.nb_offspring)
        self.podium = Podium(spec.num_elites)
        self.stats = []
        if spec.n_pairs > engine.cfg.max_members:
            raise ValueError('the engine needs max_members >= nb_offspring / 2 = %d' % spec.n_pairs)
        engine.es_create(max(spec.population_size, 1), max(spec.num_elites, 1))
        if spec.mutation in ('SM-G-SUM', 'SM-VECTOR'):
            engine.es_set_mutation_divide()
        else:
            engine.es_set_mutation('scale' if spec.mutation == 'SM-PROPORTIONAL' else 'plain')
        if spec.mutation == 'SM-VECTOR':          # one file, one vector for every parent of every generation
            from .mutations import load_vector_file
            engine.es_set_sensitivity(load_vector_file(spec.model_options.safe_mutation_vector, spec.underflow))
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
            scores = []
            if self.rank == 0:
                for slot in self.cands:
                    e.es_load_theta(slot)
                    scores.append(float(self.validator.accuracy()))
            scores = self._share_scores(scores, len(self.cands))
            scored = [('g%dc%d' % (generation, i), scores[i], slot) for i, slot in enumerate(self.cands)]
        for place, table, src in self.podium.record_elites(scored):
            e.es_set_elite(place, src, table)
        return scored

    def _share_scores(self, scores, n):
        """Rank 0's validation scores on every rank, in one collective (as EngineMaster._validate shares its score)."""
        if self.world == 1 or n == 0:
            return scores
        import torch
        t = torch.zeros((n, 2), dtype=torch.float64, device=self.e.device)
        if self.rank == 0:
            t[:, 0] = torch.tensor(scores, dtype=torch.float64)
        if self.comm == 'engine':
            allv = torch.empty((self.world * n, 2), dtype=torch.float64, device=self.e.device)
            self.e.allgather_fitness(t, allv)
            t = allv[:n]
        else:
            import torch.distributed as dist
            t = self._host_if_gloo(t)
            dist.broadcast(t, src=dist.get_global_rank(self.group, 0) if self.group is not None else 0, group=self.group)
        return [float(v) for v in t[:, 0].cpu().numpy()]

    def _host_if_gloo(self, t):
        """gloo moves host memory: a device tensor goes through the host (the rehearsal of several ranks on one GPU)."""
        import torch.distributed as dist
        return t.cpu() if dist.get_backend(self.group) == 'gloo' else t

    def _gather_fitness(self, fit_local):
        """The generation's fitness [n_pairs, 2] in pair order on every rank, from the ranks' shards (unequal by at most
        one pair): padded to the largest share, gathered, compacted."""
        n = self.spec.n_pairs
        if self.comm == 'engine':          # (also at one rank: the communicator's identity exchange)
            return self.e.es_allgather_fitness(fit_local, n)
        if self.world == 1:
            return fit_local
        import torch
        import torch.distributed as dist
        mine = self._host_if_gloo(pad_shard(fit_local, n, self.world))
        allp = torch.empty((self.world * mine.shape[0], 2), dtype=mine.dtype, device=mine.device)
        dist.all_gather_into_tensor(allp, mine, group=self.group)
        return compact_shards(allp, n, self.world).to(self.e.device)

    def step(self, batch):
        """One generation on `batch` ((fc, gts), or the reference's batch dict), on every rank. Returns its stats
        record."""
        import torch
        from ._lib import DecodeFault
        from .nes import engine_batch, is_drawn, draw_engine_batches
        e, spec, sc = self.e, self.spec, self.sched
        t0 = time.time()
        before = dict(sc.__dict__)
        sc.incr_iteration()
        g = sc.iteration
        sigma = sc.noise_stdev
        if is_drawn(batch):                # a batch of a resident training set: drawn on the device
            draw_engine_batches(batch, e)
        else:
            fc, gts = engine_batch(batch, e) if isinstance(batch, dict) else batch
            e.set_batch(fc, gts)
        parent_of = self.parents_of(g)
        begin, count = self.shard
        if spec.mutation == 'SM-G-SUM':
            # One sensitivity per distinct parent of the WHOLE generation, on every rank (the reference caches it per
            # (task_id, parent_id), safe_mutations.py:34-52): the advance re-forms survivors of pairs other ranks
            # decoded. Rows: the batch's unique images, the first orig_batch_size of them (Mutator.prepare's rule).
            rows = int(e.B)
            if rows > spec.batch_size > 0:
                rows = spec.batch_size
            e.es_sensitivity(sorted(set(int(p) for p in parent_of)), rows, spec.underflow)
        fit = self._gather_fitness(e.es_evaluate(g, begin, count, sigma, parent_of[begin:begin + count]))   # 1
        n_keep = spec.population_size - spec.num_elites
        order = e.es_select(fit, n_keep)                      # 4, enqueued behind the evaluate: no host sync between
        fit_h = fit.cpu().numpy()
        if np.isnan(fit_h).any():                             # nothing of this generation is recorded, on any rank
            sc.__dict__.update(before)
            raise DecodeFault('generation %d: NaN fitness; the parents, podium, candidates and schedule are those before it'
                              % g)
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
        if self.rank == 0 and freq and g % freq == 0:
            self.save_snapshot()
        if torch.cuda.is_available() and torch.device(e.device).type == 'cuda':
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


# ---- python -m nicnes.es: a run of an experiment, alone or as one rank of a torchrun world -----------------------------
class _RowsLoader:
    """What nicnes.validation.Validator reads, over given fc rows and their label rows (a synthetic 'val' split)."""

    def __init__(self, fc, gts, T):
        import types
        n = fc.shape[0]
        self._fc, self.seq_length, self.ix_to_word = fc, T, {}
        self.split_ix = {'val': list(range(n))}
        self.info = {'images': [{'id': i} for i in range(n)]}
        counts = np.array([g.shape[0] for g in gts])
        ends = np.cumsum(counts)
        self.labels = types.SimpleNamespace(labels=np.concatenate(gts, 0).astype(np.int32),
                                            label_start_ix=ends - counts + 1, label_end_ix=ends)

    def fc_feature(self, ix):
        return self._fc[ix]


def _synthetic_rows(engine, theta, n, fc_seed, ref_seed, df_sets=0):
    """n seeded images with references derived from the greedy captions of `theta` (nicnes.synthetic): (fc, gts, df,
    ref_len_raw). The handle's theta is set to `theta`: a validation may have left another row there, on rank 0 only."""
    from . import synthetic as S
    engine.set_theta(theta)
    fc = S.fc_feats(n, engine.cfg.fc_feat_size, fc_seed)
    sp = engine.make_split(fc)
    base = sp.decode().cpu().numpy()
    sp.close()
    gts, df, ref_len_raw = S.build_references(base, engine.cfg.vocab_size, ref_seed, 5, max(df_sets, n),
                                              engine.cfg.seq_length)
    return fc, gts, df, ref_len_raw


def parse_args(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m nicnes.es', description='nic_es generations of an mscoco_es.json-shaped '
                                 'experiment on the engine; under torchrun (RANK / LOCAL_RANK / WORLD_SIZE) one rank of a '
                                 'world that shards every generation over its GPUs')
    ap.add_argument('experiment', help='experiment JSON (algorithm nic_es)')
    ap.add_argument('--generations', type=int, default=None, help='default: config.max_nb_iterations')
    ap.add_argument('--seed', type=int, default=0, help='parent draws, initial parents, noise indices')
    ap.add_argument('--comm', choices=['torch', 'engine'], default='torch',
                    help="the fitness exchange: torch.distributed, or the engine's own RCCL communicator")
    ap.add_argument('--backend', choices=['gloo', 'nccl'], default='nccl', help='torch.distributed backend')
    ap.add_argument('--share-gpu', action='store_true',
                    help='every rank on device 0 with the coop decode off (a rehearsal of the ranks on one GPU)')
    ap.add_argument('--synthetic', action='store_true', help='batches and a validation split from nicnes.synthetic')
    ap.add_argument('--dump', default=None, metavar='DIR',
                    help='every rank writes its final parent and elite rows (rank<r>.npz) and podium, schedule and '
                         'per-generation fitness (rank<r>.json) there')
    ap.add_argument('--log_dir', default=None)
    ap.add_argument('--data_root', default='.', help="directory the caption_options paths are relative to")
    ap.add_argument('--df_path', default=None, help='document-frequency table of the training split (data.load_df_table)')
    ap.add_argument('--resident-train', action='store_true',
                    help='hold the training split on the GPU and draw every batch there (data.ResidentTrainLoader)')
    ap.add_argument('--fc-cache', default=None, metavar='PATH',
                    help='with --resident-train: one packed [N, F] .npy of the split, written once, memory-mapped after')
    ap.add_argument('--noise_len', type=int, default=1 << 27)
    ap.add_argument('--decode', default=None, help="fused | auto | coop2 | coop4 (default: fused alone, auto over ranks)")
    return ap.parse_args(argv)


def main(argv=None):
    import json
    args = parse_args(argv)
    rank, world = int(os.environ.get('RANK', '0')), int(os.environ.get('WORLD_SIZE', '1'))
    local_rank = int(os.environ.get('LOCAL_RANK', str(rank)))
    import torch
    import nicnes
    from . import synthetic as S
    from .validation import Validator
    dev = 0 if args.share_gpu else local_rank
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist
        # (--comm engine: torch.distributed only carries the communicator id, over gloo)
        if args.comm == 'engine' or args.backend == 'gloo':
            dist.init_process_group('gloo', rank=rank, world_size=world)
        else:
            dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda', dev))
    exp = load_experiment(args.experiment)
    loader = None
    if args.synthetic:
        spec = ESExperimentSpec(exp)
    else:
        from . import data
        loader = data.loader_from_caption_options(exp, int(exp['config'].get('batch_size') or 1), seed=args.seed,
                                                  root=args.data_root)
        spec = ESExperimentSpec(exp, vocab_size=loader.vocab_size, seq_length=loader.seq_length)
    eng = nicnes.Engine(device=dev, **spec.engine_kwargs(noise_len=args.noise_len, noise_seed=args.seed))
    comm = None
    if args.share_gpu and world > 1:
        eng.set_decode_coop(0)          # ranks time-sharing one GPU: the coop decode assumes the whole device
    if world > 1 and args.comm == 'engine':
        uid = [nicnes.Engine.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(uid, src=0)
        eng.comm_init(world, rank, uid[0])
        comm = 'engine'
    eng.set_noise_table(S.noise_table(args.noise_len))
    num_val = spec.config.num_val_items
    validator = None
    if args.synthetic:
        dims = S.Dims(eng.cfg.vocab_size, eng.cfg.input_encoding_size, eng.cfg.rnn_size, eng.cfg.fc_feat_size,
                      eng.cfg.seq_length)
        theta0 = S.init_theta(dims, args.seed)                 # the captions the synthetic references derive from
        made = {}

        def batches(bs):
            if bs not in made:
                made[bs] = _synthetic_rows(eng, theta0, bs, 1234, 4321, df_sets=256)
            fc, gts, df, n = made[bs]
            keys, vals = nicnes.df_table_arrays(df)
            eng.set_df_table(keys, vals, np.log(float(n)))
            while True:
                yield fc, gts
        if num_val:
            vfc, vgts, _, _ = _synthetic_rows(eng, theta0, int(num_val), 1236, 4322)
            validator = Validator(eng, _RowsLoader(vfc, vgts, eng.cfg.seq_length), 'val', int(num_val)) if rank == 0 \
                else True
    else:
        from . import data
        if args.df_path:
            df, n = data.load_df_table(args.df_path)
        else:
            df, n = {}, 1.0
        keys, vals = nicnes.df_table_arrays(df)
        eng.set_df_table(keys, vals, np.log(float(n)))

        train = data.ResidentTrainLoader(loader, eng, fc_cache=args.fc_cache) if args.resident_train else loader

        def batches(bs):
            while True:
                yield train.get_batch('train', batch_size=bs)
        if num_val is None or num_val:
            validator = Validator(eng, loader, 'val', 5000 if num_val is None else int(num_val)) if rank == 0 else True
    decode = {None: None, 'fused': 'fused', 'auto': 'auto', 'coop2': ('coop', 2), 'coop4': ('coop', 4)}[args.decode]
    m = EngineESMaster(spec, eng, validator=validator, log_dir=args.log_dir, seed=args.seed, rank=rank, world_size=world,
                       comm=comm, decode=decode)
    fitness = []
    limit = args.generations if args.generations is not None else spec.config.max_nb_iterations
    done = 0
    while not limit or done < limit:       # EngineESMaster.run, keeping every generation's fitness for --dump
        for batch in batches(m.sched.batch_size):
            m.step(batch)
            fitness.append(m.last['fitness'].tolist())
            done += 1
            if (limit and done >= limit) or m.sched.patience_reached or m.sched.schedule_reached:
                break
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
        n_el = len(m.podium.best_elites())
        np.savez(os.path.join(args.dump, 'rank%d.npz' % rank),
                 parents=np.stack([eng.es_row(i).cpu().numpy() for i in range(m.n_parents)]),
                 elites=np.stack([eng.es_row(i, 'elites').cpu().numpy() for i in range(n_el)]) if n_el
                 else np.zeros((0, eng.D), np.float32))
        with open(os.path.join(args.dump, 'rank%d.json' % rank), 'w') as f:
            json.dump({'rank': rank, 'world': world, 'shard': list(m.shard), 'decode_path': eng.es_decode_path(
                           m.sched.batch_size, m.shard[1]) if hasattr(eng, 'es_decode_path') else None,
                       'podium': m.podium.best_elites(), 'cands': m.cands, 'schedule': m.sched.to_dict(),
                       'fitness': fitness, 'stats': [{k: v for k, v in r.items() if k != 'step_time'} for r in m.stats]},
                      f)
    if rank == 0:
        print(json.dumps({'generations': done, 'world': world, 'best_val_score': m.stats[-1]['best_val_score'],
                          'score_mean': m.stats[-1]['score_mean'],
                          'step_time_s': [round(r['step_time'], 4) for r in m.stats]}), flush=True)
    if validator not in (None, True):
        validator.close()
    if comm == 'engine':
        eng.comm_destroy()
    eng.close()
    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == '__main__':
    import sys
    sys.exit(main())
