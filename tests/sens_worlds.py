"""The worlds of tests/test_gpu_sens_paths.py (GPU) and tests/test_sens_paths_host.py (their guards on the CPU): for
every path nicnes_sens_run's dispatcher can take, a vocabulary, a theta and a row count that
send a run down it, and the restatement oracle's vector there. All at F = 128 (short oracle and GPU runs); fc rows
from PCG64(78); 'wc' = make_theta(dims, 3, 4.0, 0.1), 'xavier' = make_theta(dims, 0, 1.0, 0.0). Not a test module."""
import numpy as np
import torch

from oracle import oracle as O
from oracle import sensitivity_ref as SR

F = 128
L = 5                     # forward_for_sensitivity's length
SPLIT = 100
EMB_CH = 16               # pairs per chunk of the two-pass embedding sums (sensitivity.hip)
EMB_MAXP = 4096           # pairs at most: rows <= 819
MAX_ROWS = EMB_MAXP // L
SEGMENTS = ('img_embed.weight', 'img_embed.bias', 'embed.weight', 'logit.weight', 'logit.bias', 'core.i2h.weight',
            'core.i2h.bias', 'core.h2h.weight', 'core.h2h.bias')
ALL_FAST = dict(logit_fast=True, bwd_fused=True, gates_bsq=True, emb_two_pass=True)
SWITCHES = {'logit': 'NICNES_SENS_TILE_LOGIT', 'bwd': 'NICNES_SENS_TILE_BWD', 'gates': 'NICNES_SENS_TILE_GATES',
            'emb': 'NICNES_SENS_EMB_KC', 'scalar': 'NICNES_SENS_TILE_SCALAR'}
SWITCH_BIT = {'logit': 'logit_fast', 'bwd': 'bwd_fused', 'gates': 'gates_bsq', 'emb': 'emb_two_pass', 'scalar': None}


def paths(**cleared):
    """the four bits, all fast but the ones named False"""
    return dict(ALL_FAST, **cleared)


# id: (vocab, theta kind, rows, the bits sens_paths() must report with no switch set)
_AS_129 = paths(logit_fast=False)
SHAPE_CASES = {
    'base': (999, 'wc', 12, ALL_FAST),
    'rows_1': (999, 'wc', 1, ALL_FAST), 'rows_32': (999, 'wc', 32, ALL_FAST), 'rows_33': (999, 'wc', 33, ALL_FAST),
    'rows_64': (999, 'wc', 64, ALL_FAST), 'rows_65': (999, 'wc', 65, ALL_FAST), 'rows_128': (999, 'wc', 128, ALL_FAST),
    'rows_129': (999, 'wc', 129, _AS_129),
    'rows_max': (999, 'wc', MAX_ROWS, _AS_129),
    'odd_cl': (1027, 'wc', 65, ALL_FAST),
    'K97': (9603, 'wc', 8, paths(gates_bsq=False, emb_two_pass=False)),
    'K98': (9699, 'xavier', 8, paths(gates_bsq=False, emb_two_pass=False)),
}
# vocab: (V1 % 4, K, nsp, cl = V1 / nsp, the % 4 of the i2h.weight and h2h.weight offsets); nsp: the parts p Wl is split in
# over the vocabulary (the largest divisor d <= 32 of V1 with V1 / d >= 32, else 1), cl the reduction length of each
VOCAB_FACTS = {
    999: (0, 11, 25, 40, 0, 0),          # 1000 = 2^3 5^3
    1027: (0, 11, 4, 257, 0, 0),         # 1028 = 4 257: an odd, prime reduction length (4 chunks of 64 and 1 value)
    9603: (0, 97, 28, 343, 0, 0),        # 9604 = 4 7^4: the first K past the fast kernels' 96
    9699: (0, 98, 25, 388, 0, 0),        # 9700 = 2^2 5^2 97
    127: (0, 2, 4, 32, 0, 0),
}
# Vocabularies whose V1 is no multiple of 4 would misalign core.i2h.weight and everything after it (the facts as above)
# and so clear the backward bit and drop every V-strided product to scalar loads by shape alone; nicnes_create refuses
# them (V1 % 4 != 0: the decode kernels' 16-byte rows), so no handle reaches nicnes_sens_run that way.
REFUSED_VOCABS = {
    1000: (1, 11, 13, 77, 1, 1),         # 1001 = 7 11 13
    1002: (3, 11, 17, 59, 3, 3),         # 1003 = 17 59
    1008: (1, 11, 1, 1009, 1, 1),        # 1009 prime
    9601: (2, 97, 2, 4801, 2, 2),        # 9602 = 2 4801
}
# What such a shape would run, forced by the two switches that stand for it (the tile kernel's gemms for dX / dH, scalar
# loads in every product), at one block of rows, a full logit slab and the first row count past it, both thetas:
# id: (vocab, kind, rows, switches, bits)
FORCED_CASES = {
    'unaligned_like_%s_%d' % (kind, rows): (999, kind, rows, ('bwd', 'scalar'),
                                            paths(bwd_fused=False, logit_fast=rows <= 128))
    for kind in ('wc', 'xavier') for rows in (12, 128, 129)}
# every other (vocab, kind, rows) the GPU module runs: the all-switches case, the buffer-reuse sequence, the forced
# embedding ranges at a small K, the limit's handle
EXTRA_WORLDS = [(999, 'wc', 41), (999, 'wc', 8), (127, 'xavier', 12), (127, 'xavier', MAX_ROWS)]
REUSE_ROWS = (12, 129, 8, 128, 12)
ES_VOCAB, ES_SEEDS, ES_ROWS = 999, (3, 11, 23), 129

_cache = {}


def dims_of(vocab):
    return O.Dims(vocab_size=vocab, F=F)


def theta_of(vocab, kind):
    key = ('theta', vocab, kind)
    if key not in _cache:
        d = dims_of(vocab)
        if isinstance(kind, int):                               # a nic_es parent: 'wc' from that seed
            _cache[key] = O.make_theta(d, kind, 4.0, 0.1)
        else:
            _cache[key] = O.make_theta(d, 3, 4.0, 0.1) if kind == 'wc' else O.make_theta(d, 0, 1.0, 0.0)
    return _cache[key]


def fc_rows(n):
    """the first n of MAX_ROWS + 1 rows drawn once (so the rows of a smaller batch are the first rows of a larger)"""
    if 'fc' not in _cache:
        _cache['fc'] = np.random.Generator(np.random.PCG64(78)).standard_normal((MAX_ROWS + 1, F)).astype(np.float32)
    return _cache['fc'][:n]


def reference(vocab, kind, rows, perm=None):
    """oracle/sensitivity_ref.py's raw vector on the first `rows` fc rows (in the order perm, if given), computed once"""
    key = ('ref', vocab, kind, rows, None if perm is None else tuple(perm))
    if key not in _cache:
        d = dims_of(vocab)
        fc = fc_rows(rows) if perm is None else fc_rows(rows)[np.asarray(perm)]
        _cache[key] = SR.sum_sensitivity((d.V1, d.E, d.R, F), theta_of(vocab, kind), fc, rows).numpy()
        _cache[key].setflags(write=False)
    return _cache[key]


def oracle_tokens(vocab, kind, rows):
    """[rows, L] the token fed to cells 1..L by the oracle's forward (column 0: BOS; then its greedy tokens of steps
    1..L-1, torch.max over the log-probs as forward_for_sensitivity takes them)"""
    d = dims_of(vocab)
    net = SR.SensitivityNet(d.V1, d.E, d.R, F)
    net.load_vector(theta_of(vocab, kind))
    with torch.no_grad():
        fc = torch.as_tensor(fc_rows(rows))
        h = c = fc.new_zeros(rows, d.R)
        h, c = net.core(net.img_embed(fc), h, c)
        it = torch.zeros(rows, dtype=torch.long)
        fed = []
        for _ in range(L):
            fed.append(it.numpy().copy())
            h, c = net.core(net.embed(it), h, c)
            it = torch.max(torch.log_softmax(net.logit(h), dim=1), 1)[1].view(-1).long()
    return np.stack(fed, axis=1)


def segments(vocab):
    """[(name, offset, size)] of dims.offsets(), in theta order"""
    offs = dims_of(vocab).offsets()
    return [(name, offs[name][0], int(np.prod(offs[name][1]))) for name in SEGMENTS]


def segment_ratios(got, ref, vocab):
    """{segment: the worst |got - ref| / bound over it}, the bound being tests/test_gpu_mutations.py's bar on the whole
    vector (SENS_RTOL |ref| + 1e-6 max |ref|, elementwise): all <= 1 exactly when _sens_close holds"""
    from tests.test_gpu_mutations import SENS_RTOL
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    bound = SENS_RTOL * np.abs(ref) + 1e-6 * np.abs(ref).max()
    return {name: float((err[o:o + n] / bound[o:o + n]).max()) for name, o, n in segments(vocab)}


def all_worlds():
    """every distinct (vocab, kind, rows) the GPU module compares with the oracle"""
    w = [(v, k, r) for v, k, r, _ in SHAPE_CASES.values()] + EXTRA_WORLDS
    w += [(v, k, r) for v, k, r, _, _ in FORCED_CASES.values()]
    w += [(999, 'wc', r) for r in REUSE_ROWS] + [(ES_VOCAB, s, ES_ROWS) for s in ES_SEEDS[::2]]
    return sorted(set(w), key=str)
