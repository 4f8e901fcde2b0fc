"""The worlds of the sampled-pick tests (tests/test_sample_planted.py on the CPU, tests/test_gpu_sample_pick.py on the
GPU): small models (F = 128) whose sampled decode is aimed, draw by draw, at chosen ids with the oracle's planted draws
(oracle.decode_sample_planted). Everything here is made from numpy PCG64 seeds and the oracle, once per process.

A world is theta (flat xavier logits, or the gain-4 'well-conditioned' one), edits of logit.bias, and a shape. The
edits of the 'stairs' worlds: a step of +0.75 nat on every id from 64 s on (1.08 bits, so the lane's integer reference
r = ceil(m log2e) rises exactly once at stage s: in mid-block, at a block start, at the last stage) and spikes of +2.0
on single ids, each in one lane half, so the two lanes of a row carry different r.

Candidates: every id of the stages either side of the block boundaries (8 stages), of the level-1 round boundary (20
blocks, reached with V1 > 10240) and of the tail, plus the ids either side of each step and each spike +- 1. Targets
are dealt round-robin over the (member, sign, row, step) positions, which outnumber the candidates in every world."""
import numpy as np

from oracle import oracle as O

NOISE_LEN = 1 << 23
NOISE_SEED = 7
TABLE_SEED = 123
IT = 3
SIGMA = 0.01
F = 128
MIN_HALF_WIDTH = 1e-5              # ten times tests/test_oracle_golden.U_MARGIN

STEP, SPIKE = 0.75, 2.0
WORLDS = {
    'flat': dict(vocab=9487, T=16, B=130, members=2, theta=(1.0, 0.0)),
    'wc': dict(vocab=9487, T=16, B=130, members=2, theta=(4.0, 0.1)),
    'stairs': dict(vocab=9487, T=16, B=130, members=2, theta=(1.0, 0.0), steps=(3, 77, 148),
                   spikes=(5, 2596, 6463, 9484)),
    'v16384': dict(vocab=16383, T=3, B=40, members=6, theta=(1.0, 0.0)),
    'stairs1000': dict(vocab=999, T=16, B=40, members=1, theta=(1.0, 0.0), steps=(3, 8, 13, 15),
                       spikes=(5, 612, 831, 996)),
    'v68': dict(vocab=67, T=16, B=40, members=1, theta=(1.0, 0.0)),
    'v60': dict(vocab=59, T=7, B=40, members=1, theta=(1.0, 0.0)),
    'v8': dict(vocab=7, T=16, B=40, members=1, theta=(1.0, 0.0)),
    'v255': dict(vocab=255, T=16, B=40, members=1, theta=(1.0, 0.0)),      # a full 64-column last stage
}
PLANTED_WORLDS = ['flat', 'wc', 'stairs', 'v16384', 'stairs1000', 'v68', 'v60', 'v8']
CANDIDATE_STAGES = (0, 1, 7, 8, 9, 15, 16, 63, 64, 151, 152, 159, 160, 161, 167, 168)

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def dims(world):
    w = WORLDS[world]
    return O.Dims(w['vocab'], 128, 128, F, w['T'])


def table():
    return _once('table', lambda: O.noise_table(NOISE_LEN, TABLE_SEED))


def theta(world):
    def make():
        w, d = WORLDS[world], dims(world)
        th = O.make_theta(d, 0, *w['theta'])
        o = d.offsets()['logit.bias'][0]
        for s in w.get('steps', ()):
            th[o + 64 * s: o + d.V1] += np.float32(STEP)
        for v in w.get('spikes', ()):
            th[o + v] += np.float32(SPIKE)
        return th
    return _once(('theta', world), make)


def fc(world):
    B = WORLDS[world]['B']
    return _once(('fc', B), lambda: np.random.Generator(np.random.PCG64(100 + B)).standard_normal((B, F))
                 .astype(np.float32))


def member_thetas(world):
    """theta +- sigma z of each member: [(theta+, theta-), ...], with the members' noise indices."""
    def make():
        d = dims(world)
        idx = [O.noise_index(NOISE_SEED, IT, k, NOISE_LEN, d.D) for k in range(WORLDS[world]['members'])]
        return idx, [tuple(O.perturb(theta(world), table(), i, SIGMA, sign) for sign in (+1, -1)) for i in idx]
    return _once(('members', world), make)


def candidates(world):
    w, V1 = WORLDS[world], WORLDS[world]['vocab'] + 1
    nst = (V1 + 63) // 64
    stages = set(CANDIDATE_STAGES) | {nst - 9, nst - 8, nst - 2, nst - 1}
    ids = {64 * s + j for s in stages if 0 <= s < nst for j in range(64)}
    for s in w.get('steps', ()):
        ids |= {64 * s - 1, 64 * s}
    for v in w.get('spikes', ()):
        ids |= {v - 1, v, v + 1}
    return np.asarray(sorted(v for v in ids if 0 < v < V1), np.int32)


def targets(world):
    """[members, 2, B, T]: the candidates dealt round-robin over the positions."""
    w = WORLDS[world]
    c = candidates(world)
    n = w['members'] * 2 * w['B'] * w['T']
    assert n >= len(c)
    return c[np.arange(n) % len(c)].reshape(w['members'], 2, w['B'], w['T'])


def plant(world, tg):
    """The oracle's planted draws for targets tg [members, 2, B, T]: (u, half_width, seq, lp), each [members, 2, B, T]."""
    d = dims(world)
    _, ths = member_thetas(world)
    out = [[O.decode_sample_planted(d, ths[k][s], fc(world), tg[k, s]) for s in range(2)] for k in range(len(ths))]
    return tuple(np.stack([np.stack([out[k][s][i] for s in range(2)]) for k in range(len(ths))]) for i in range(4))


def planted(world):
    return _once(('planted', world), lambda: plant(world, targets(world)))


def decode_with(world, u):
    """oracle.decode_sample of every member and sign with the draws u [members, 2, B, T]: (seq, lp, fragile)."""
    d = dims(world)
    _, ths = member_thetas(world)
    out = [[O.decode_sample(d, ths[k][s], fc(world), u[k, s]) for s in range(2)] for k in range(len(ths))]
    return tuple(np.stack([np.stack([out[k][s][i] for s in range(2)]) for k in range(len(ths))]) for i in range(3))
