"""The worlds of tests/test_gpu_xent_shapes.py (GPU) and tests/test_xent_worlds_host.py (their guards on the CPU): for
every path of the teacher-forced forward (csrc/xent_kernels.hip) that tests/test_gpu_xent.py's
F = 128, <= 130-row, contiguous-word cases leave out, a shape that reaches it and tests/xent_ref.py's values there.
Theta is make_theta(dims, 0, 4.0, 0.1) throughout; every generator is a PCG64. Not a test module.

Member worlds (fitness mode 'xent', sigma 0.01, iteration 3, members 0..3):
  M1  V1 68  F 256   T 16  one batch, 300 rows, images of 1..7 rows: nK = 2; three slabs with a 44-row tail; the reduce
                           kernel's second pass on 44 threads
  M2  V1 68  F 2048  T 3   one batch, 129 rows: the workload's F (nK = 16); a 1-row tail slab
  M3  V1 8   F 128   T 3   two batches of 100 images with 513 and 257 rows: stride 513, five slabs, the smaller batch
                           skips two whole slabs, three reduce passes
  M4  V1 68  F 384   T 16  one batch, 40 rows: nK = 3; label rows with zeros inside (M4_KINDS)
Flat worlds (theta itself):
  S1  V1 8   F 256   T 3   one split: 130 one-row images, one image of 300 rows, 200 images of 1..3 rows, 400 one-row
                           images (1,229 rows); the ranges S1_RANGES
  S2  V1 68  F 2048  T 1   257 one-row images: a row's image at up to 255 * 2048 floats, and a one-row second
                           pseudo-member
  H1  V1 8   F 128   T 3   the handle's own flat path: three batches of 64 images with 200, 300 and 513 rows
  D   V1 68  F 256   T 16  a resident training set of 40 images of 1..7 rows and the draws DRAWS from it
  G   V1 8   F 128   T 3   one-batch worlds of 130, 513 and 5 rows for one handle that grows and shrinks

Label rows extend test_gpu_xent._labels: lengths cycle through 0, 1, 5 and T (cut to T), every third word a planted id
walking through 3, 4, 31, 32, 63, 64 (those within the vocabulary) and V; id 0 is the end target of every row."""
import numpy as np

from oracle import oracle as O
from tests import xent_ref as X

NOISE_LEN = 1 << 23
SEED = 7
SIGMA = 0.01
IT = 3
P = 4
LP_BAR = 1e-5
PLANT = (3, 4, 31, 32, 63, 64)

_cache = {}


def table():
    if 'table' not in _cache:
        _cache['table'] = O.noise_table(NOISE_LEN, 123)
    return _cache['table']


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _freeze(x):
    """every array reachable through dicts, lists and tuples: read-only"""
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _freeze(v)
    return x


def words(V, n, r, rng):
    """n words of row r: random ids in 1..V, every third one a planted id"""
    plant = [v for v in PLANT if v <= V] + [V]
    w = rng.integers(1, V + 1, n)
    for j in range(n):
        if (r + j) % 3 == 0:
            w[j] = plant[(r + j) // 3 % len(plant)]
    return w


def labels(V, T, n_rows, rng):
    """label rows [n_rows, T]: row r has min((0, 1, 5, T)[r % 4], T) words, then padding"""
    lab = np.zeros((n_rows, T), np.int32)
    for r in range(n_rows):
        n = min((0, 1, 5, T)[r % 4], T)
        lab[r, :n] = words(V, n, r, rng)
    return lab


def cyclic_counts(total, period):
    """rows per image 1, 2, .., period, 1, .. until `total` rows are used (the last image takes what is left)"""
    out, k = [], 0
    while sum(out) < total:
        out.append(min(1 + k % period, total - sum(out)))
        k += 1
    return out


def spread_counts(n_img, total, rng):
    """n_img images, every one with a row, `total` rows in all: the spare rows thrown at random"""
    c = np.ones(n_img, np.int64)
    for i in rng.integers(0, n_img, total - n_img):
        c[i] += 1
    return [int(v) for v in c]


def batch_of(lab, counts, F, rng):
    """(fc [images, F], gts): the rows of `lab` cut into images of `counts` rows"""
    assert sum(counts) == lab.shape[0]
    at = np.concatenate([[0], np.cumsum(counts)])
    gts = [lab[at[i]:at[i + 1]] for i in range(len(counts))]
    return rng.standard_normal((len(counts), F)).astype(np.float32), gts


# ---- the reduce order of nicnes_xent_reduce_kernel --------------------------------------------------------------------
def reduce_order(lp_sum, n_tok):
    """(sum lp_sum, sum n_tok) as the device adds them: thread i of 256 sums rows i, i + 256, .. in order in fp64, then
    for w in 128, 64, .., 1: part[:w] += part[w:2w]. fitness = the quotient, loss = its negative."""
    lp = np.asarray(lp_sum, np.float64)
    nt = np.asarray(n_tok, np.int64)
    part = np.zeros(256, np.float64)
    cnt = np.zeros(256, np.int64)
    for i in range(256):
        for r in range(i, lp.shape[0], 256):
            part[i] = part[i] + lp[r]
            cnt[i] += nt[r]
    w = 128
    while w > 0:
        part[:w] = part[:w] + part[w:2 * w]
        cnt[:w] = cnt[:w] + cnt[w:2 * w]
        w >>= 1
    return float(part[0]), int(cnt[0])


def reduce_fitness(lp_sum, n_tok):
    a, n = reduce_order(lp_sum, n_tok)
    return a / float(n)


# ---- member worlds ----------------------------------------------------------------------------------------------------
MEMBER_WORLDS = {
    'M1': dict(vocab=67, F=256, T=16, rows=(300,)),
    'M2': dict(vocab=67, F=2048, T=3, rows=(129,)),
    'M3': dict(vocab=7, F=128, T=3, rows=(513, 257), images=100),
    'M4': dict(vocab=67, F=384, T=16, rows=(40,)),
}
# M4: the row kinds and where they stand. Rows 1..6 have (row & 31) < 16, rows 17..22 have it >= 16 (the two 16-row
# halves of a 32-row group; both lane halves of a wave hold all 32 rows, so either half of the lanes sees every kind),
# rows 33..38 lie in the second 32-row group (another wave); every other row is an ordinary one.
M4_KINDS = ('alt', 'lead0', 'full', 'tail', 'zero', 'plain')
M4_AT = {base + i: kind for base in (1, 17, 33) for i, kind in enumerate(M4_KINDS)}


def m4_counted(kind, T):
    """the steps that count in a row of this kind (None: an ordinary row, whatever its length)"""
    return {'alt': [0] + list(range(1, T + 1, 2)),           # [w, 0, w, 0, ..]: behind every word, words at 0, 2, ..
            'lead0': [0, 2, 3],                               # [0, w, w, 0, ..]
            'full': list(range(T + 1)),                       # [w] * T: all T + 1 steps
            'tail': [0, T - 1, T],                            # words at T - 2 and T - 1 only
            'zero': [0]}.get(kind)


def _m4_labels(V, T, rng):
    lab = labels(V, T, 40, rng)
    for r, kind in M4_AT.items():
        w = words(V, T, r, rng)
        row = np.zeros(T, np.int32)
        if kind == 'alt':
            row[0::2] = w[0::2]
        elif kind == 'lead0':
            row[1:3] = w[1:3]
        elif kind == 'full':
            row[:] = w
        elif kind == 'tail':
            row[T - 2:] = w[T - 2:]
        elif kind == 'plain':
            row[:5] = w[:5]
        lab[r] = row
    return lab


def member_inputs(name):
    """dims, theta, batches [(fc, gts)], member_batch (None with one batch): no restatement run"""
    key = ('in', name)
    if key not in _cache:
        c = MEMBER_WORLDS[name]
        dims = O.Dims(vocab_size=c['vocab'], F=c['F'], T=c['T'])
        batches = []
        for i, rows in enumerate(c['rows']):
            rng = _rng(700 + 10 * i + sum(map(ord, name)))
            lab = _m4_labels(c['vocab'], c['T'], rng) if name == 'M4' else labels(c['vocab'], c['T'], rows, rng)
            counts = spread_counts(c['images'], rows, rng) if 'images' in c else cyclic_counts(rows, 7)
            batches.append(batch_of(lab, counts, c['F'], rng))
        mb = [k % len(batches) for k in range(P)] if len(batches) > 1 else None
        _cache[key] = _freeze(dict(dims=dims, theta=O.make_theta(dims, 0, 4.0, 0.1), batches=batches, mb=mb))
    return _cache[key]


def candidate_ref(dims, theta, batch, member, sign, sigma=SIGMA, it=IT):
    """the restatement of member `member`, sign +1 / -1, on one batch"""
    idx = O.noise_index(SEED, it, member, NOISE_LEN, dims.D)
    fr, lab, _ = X.rows_of(*batch)
    lp, lp_sum, n_tok = X.forced(dims, O.perturb(theta, table(), idx, sigma, sign), fr, lab)
    return dict(lp=lp, lp_sum=lp_sum, n_tok=n_tok, fit=-X.loss_of(lp_sum, n_tok), mask=X.counted(lab))


def theta_ref(dims, theta, batch):
    fr, lab, _ = X.rows_of(*batch)
    lp, lp_sum, n_tok = X.forced(dims, theta, fr, lab)
    return dict(lp=lp, lp_sum=lp_sum, n_tok=n_tok, fit=-X.loss_of(lp_sum, n_tok), mask=X.counted(lab))


def member_world(name):
    """member_inputs plus ref[k, s] for members 0..3 and both signs, each on the member's batch"""
    key = ('world', name)
    if key not in _cache:
        w = dict(member_inputs(name))
        w['ref'] = {(k, s): candidate_ref(w['dims'], w['theta'], w['batches'][w['mb'][k] if w['mb'] else 0], k, sign)
                    for k in range(P) for s, sign in enumerate((+1, -1))}
        _cache[key] = _freeze(w)
    return _cache[key]


def m4_theta_ref():
    """theta itself on M4's rows (the host guards compare the three places a row's steps are counted on it)"""
    if 'M4theta' not in _cache:
        w = member_inputs('M4')
        _cache['M4theta'] = _freeze(theta_ref(w['dims'], w['theta'], w['batches'][0]))
    return _cache['M4theta']


# ---- flat worlds ------------------------------------------------------------------------------------------------------
S1_ONES, S1_BIG, S1_MIXED, S1_TAIL = 130, 300, 200, 400
# name: (label rows, row0 % 128, pseudo-members, the first image is searched from this one on); 'whole' is the split
S1_RANGES = {
    'r255': (255, 64, 1, 140),       # inside the 1..3-row images
    'r256': (256, 66, 1, None),      # from the 6th image of the last run on: 256 rows of 256 different images
    'r257': (257, 83, 2, 148),       # a one-row second pseudo-member
    'r384': (384, 100, 2, 100),      # the 300-row image at rows 30..329 of the range: over its row 256
    'r385': (385, 99, 2, 99),        # .. at rows 31..330; sign - of the second pseudo-member has one row
    'r513': (513, 1, 3, 1),          # .. at rows 129..428; a one-row third pseudo-member
    'whole': (None, 0, 5, 0),
}


def s1_counts():
    return [1] * S1_ONES + [S1_BIG] + [1 + k % 3 for k in range(S1_MIXED)] + [1] * S1_TAIL


def s1_ranges(starts):
    """name -> (first, count) in images, found from the row starts: the first image at or behind the range's hint whose
    row start + the wanted rows is a row start too"""
    starts = np.asarray(starts)
    at = {int(v): i for i, v in enumerate(starts)}
    tail0 = S1_ONES + 1 + S1_MIXED                               # the first image of the last run
    out = {}
    for name, (rows, _, _, hint) in S1_RANGES.items():
        if rows is None:
            out[name] = (0, len(starts) - 1)
            continue
        f = tail0 + 5 if hint is None else hint
        while int(starts[f]) + rows not in at:
            f += 1
        out[name] = (f, at[int(starts[f]) + rows] - f)
    return out


def flat_world(name):
    """S1 / S2: dims, theta, fc, gts, starts [images + 1], ranges {name: (first, count)} and the restatement of theta on
    every row (lp, lp_sum, n_tok, mask)"""
    key = ('flat', name)
    if key not in _cache:
        w = dict(flat_inputs(name))
        w['ref'] = theta_ref(w['dims'], w['theta'], (w['fc'], w['gts']))
        _cache[key] = _freeze(w)
    return _cache[key]


def flat_inputs(name):
    key = ('flatin', name)
    if key not in _cache:
        vocab, F, T, counts = {'S1': (7, 256, 3, s1_counts()), 'S2': (67, 2048, 1, [1] * 257)}[name]
        dims = O.Dims(vocab_size=vocab, F=F, T=T)
        rng = _rng(900 + ord(name[1]))
        fc, gts = batch_of(labels(vocab, T, sum(counts), rng), counts, F, rng)
        starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        ranges = s1_ranges(starts) if name == 'S1' else {'whole': (0, len(counts))}
        _cache[key] = _freeze(dict(dims=dims, theta=O.make_theta(dims, 0, 4.0, 0.1), fc=fc, gts=gts, starts=starts,
                                   ranges=ranges))
    return _cache[key]


H1 = dict(vocab=7, F=128, T=3, rows=(200, 300, 513), images=64)


def h1_inputs():
    if 'H1in' not in _cache:
        dims = O.Dims(vocab_size=H1['vocab'], F=H1['F'], T=H1['T'])
        batches = []
        for i, rows in enumerate(H1['rows']):
            rng = _rng(1100 + i)
            batches.append(batch_of(labels(H1['vocab'], H1['T'], rows, rng), spread_counts(H1['images'], rows, rng),
                                    H1['F'], rng))
        _cache['H1in'] = _freeze(dict(dims=dims, theta=O.make_theta(dims, 0, 4.0, 0.1), batches=batches))
    return _cache['H1in']


def h1_world():
    """h1_inputs plus ref[k]: theta on batch k"""
    if 'H1' not in _cache:
        w = dict(h1_inputs())
        w['ref'] = [theta_ref(w['dims'], w['theta'], b) for b in w['batches']]
        _cache['H1'] = _freeze(w)
    return _cache['H1']


# ---- drawn batches ----------------------------------------------------------------------------------------------------
D = dict(vocab=67, F=256, T=16, images=40, members=2)
# [2, B] image indices: an image twice inside a batch and in both batches
DRAWS = {
    'first': [[5, 9, 5, 0, 39, 17, 9, 23, 6, 30, 2, 11], [9, 5, 13, 13, 38, 1, 0, 27, 6, 35, 4, 20]],
    'large': [[(7 * i + 3) % 40 for i in range(28)] + [3, 17],
              [(11 * i + 1) % 40 for i in range(25)] + [3, 3, 10, 10, 39]],
}


def drawn_inputs():
    """dims, theta, the set (fc [40, F], gts) and per draw the host-gathered batches"""
    if 'Din' not in _cache:
        dims = O.Dims(vocab_size=D['vocab'], F=D['F'], T=D['T'])
        rng = _rng(1300)
        counts = [1 + k % 7 for k in range(D['images'])]
        fc, gts = batch_of(labels(D['vocab'], D['T'], sum(counts), rng), counts, D['F'], rng)
        host = {name: [(fc[np.array(ix)], [gts[i] for i in ix]) for ix in draw] for name, draw in DRAWS.items()}
        _cache['Din'] = _freeze(dict(dims=dims, theta=O.make_theta(dims, 0, 4.0, 0.1), fc=fc, gts=gts, host=host))
    return _cache['Din']


def draw_rows(name):
    """label rows of each of the draw's batches"""
    w = drawn_inputs()
    return [sum(g.shape[0] for g in gts) for _, gts in w['host'][name]]


def drawn_world():
    """drawn_inputs plus ref[draw][k, s]: member k (on batch k) of D['members'], both signs"""
    if 'D' not in _cache:
        w = dict(drawn_inputs())
        w['ref'] = {name: {(k, s): candidate_ref(w['dims'], w['theta'], w['host'][name][k], k, sign)
                           for k in range(D['members']) for s, sign in enumerate((+1, -1))} for name in DRAWS}
        _cache['D'] = _freeze(w)
    return _cache['D']


# ---- one handle, growing and shrinking --------------------------------------------------------------------------------
G_ROWS = (130, 513, 5)


def grow_inputs():
    """dims, theta and one batch per entry of G_ROWS (V1 8, F 128, T 3; images of 1..7 rows)"""
    if 'G' not in _cache:
        dims = O.Dims(vocab_size=7, F=128, T=3)
        batches = []
        for i, rows in enumerate(G_ROWS):
            rng = _rng(1500 + i)
            batches.append(batch_of(labels(7, 3, rows, rng), cyclic_counts(rows, 7), 128, rng))
        _cache['G'] = _freeze(dict(dims=dims, theta=O.make_theta(dims, 0, 4.0, 0.1), batches=batches))
    return _cache['G']
