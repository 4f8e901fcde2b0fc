"""CPU: the preconditions of tests/test_gpu_xent_shapes.py's worlds (tests/xent_worlds.py), so that a later change of a
seed or a count cannot empty a case: exact row counts, the offsets and pseudo-members of every flat range, non-empty
slabs and halves, the lane halves, tiles and stages the targets reach, the three places a row's counted steps are
derived in on rows with zeros inside, and the host emulation of the device's reduce order."""
import math

import numpy as np
import pytest

from tests import xent_ref as X
from tests import xent_worlds as W


def _rows(batch):
    return sum(g.shape[0] for g in batch[1])


def _all_label_sets():
    out = {}
    for name in W.MEMBER_WORLDS:
        w = W.member_inputs(name)
        out[name] = (w['dims'], [X.rows_of(*b)[1] for b in w['batches']])
    for name in ('S1', 'S2'):
        w = W.flat_inputs(name)
        out[name] = (w['dims'], [X.rows_of(w['fc'], w['gts'])[1]])
    w = W.h1_inputs()
    out['H1'] = (w['dims'], [X.rows_of(*b)[1] for b in w['batches']])
    w = W.drawn_inputs()
    out['D'] = (w['dims'], [X.rows_of(w['fc'], w['gts'])[1]] + [X.rows_of(*b)[1] for d in w['host'].values() for b in d])
    w = W.grow_inputs()
    out['G'] = (w['dims'], [X.rows_of(*b)[1] for b in w['batches']])
    return out


# ---- row counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(W.MEMBER_WORLDS))
def test_member_world_row_counts_are_exact(name):
    w, c = W.member_inputs(name), W.MEMBER_WORLDS[name]
    assert tuple(_rows(b) for b in w['batches']) == c['rows']
    assert len({b[0].shape[0] for b in w['batches']}) == 1, 'batches of one handle have the same image count'
    assert all(b[0].shape == (len(b[1]), c['F']) for b in w['batches'])
    assert all(g.shape[0] >= 1 and g.shape[1] == c['T'] for b in w['batches'] for g in b[1])
    assert (w['mb'] is None) == (len(c['rows']) == 1)
    assert (w['dims'].V1, w['dims'].F, w['dims'].T) == (c['vocab'] + 1, c['F'], c['T'])
    assert w['dims'].F >> 7 == {'M1': 2, 'M2': 16, 'M3': 1, 'M4': 3}[name], 'nK'


def test_m1_images_have_one_to_seven_rows():
    n = [g.shape[0] for g in W.member_inputs('M1')['batches'][0][1]]
    assert set(n[:-1]) == set(range(1, 8)) and 1 <= n[-1] <= 7


def test_m3_batches_differ_by_two_whole_slabs():
    w = W.member_inputs('M3')
    a, b = (_rows(x) for x in w['batches'])
    assert ((a + 127) // 128, (b + 127) // 128) == (5, 3) and (a % 128, b % 128) == (1, 1)
    assert w['mb'] == [0, 1, 0, 1]
    assert (a + 255) // 256 == 3, 'three passes of the reduce loop'
    for batch in w['batches']:
        assert len({g.shape[0] for g in batch[1]}) > 2, 'the rows per image vary'


def test_h1_and_grow_row_counts():
    w = W.h1_inputs()
    assert tuple(_rows(b) for b in w['batches']) == (200, 300, 513)
    assert {b[0].shape[0] for b in w['batches']} == {64}
    at = np.concatenate([[0], np.cumsum([_rows(b) for b in w['batches']])])
    assert at[1] % 128 != 0 and at[2] % 128 != 0, 'row0 of batches 1 and 2 inside a slab'
    assert tuple(_rows(b) for b in W.grow_inputs()['batches']) == W.G_ROWS == (130, 513, 5)


def test_s2_is_257_images_of_one_row():
    w = W.flat_inputs('S2')
    assert np.array_equal(w['starts'], np.arange(258)) and w['fc'].shape == (257, 2048) and w['dims'].T == 1
    assert w['ranges'] == {'whole': (0, 257)}


# ---- S1 -----------------------------------------------------------------------------------------------------------------
def _s1():
    w = W.flat_inputs('S1')
    _, _, row_img = X.rows_of(w['fc'], w['gts'])
    return w, w['starts'], row_img


def test_s1_is_built_as_stated():
    w, st, _ = _s1()
    n = np.diff(st)
    assert (n[:130] == 1).all() and n[130] == 300 and set(n[131:331]) == {1, 2, 3} and (n[331:] == 1).all()
    assert len(n) == 130 + 1 + 200 + W.S1_TAIL and st[-1] >= 900
    assert set(w['ranges']) == set(W.S1_RANGES)


@pytest.mark.parametrize('name', sorted(W.S1_RANGES))
def test_s1_range_has_its_rows_offset_and_pseudo_members(name):
    w, st, _ = _s1()
    rows, mod, n_pm, _ = W.S1_RANGES[name]
    first, count = w['ranges'][name]
    r0, r1 = int(st[first]), int(st[first + count])
    assert r1 - r0 == (rows if rows is not None else int(st[-1]))
    assert r0 % 128 == mod and (r1 - r0 + 255) // 256 == n_pm


def test_s1_ranges_cover_the_row_counts_and_offsets():
    w, st, _ = _s1()
    got = sorted(int(st[f + c] - st[f]) for f, c in w['ranges'].values())
    assert got == [255, 256, 257, 384, 385, 513, int(st[-1])]
    off = [int(st[f]) for f, c in w['ranges'].values()]
    assert sum(1 for r0 in off if r0 > 0 and r0 % 128 != 0) >= 2


# (rows of sign +, rows of sign -) of every pseudo-member
S1_HALVES = {
    'r255': [(128, 127)], 'r256': [(128, 128)], 'r257': [(128, 128), (1, 0)], 'r384': [(128, 128), (128, 0)],
    'r385': [(128, 128), (128, 1)], 'r513': [(128, 128), (128, 128), (1, 0)],
    'whole': [(128, 128)] * 4 + [(128, 77)],
}


@pytest.mark.parametrize('name', sorted(W.S1_RANGES))
def test_s1_pseudo_member_halves(name):
    w, st, _ = _s1()
    first, count = w['ranges'][name]
    rows = int(st[first + count] - st[first])
    halves = []
    for k in range((rows + 255) // 256):
        left = rows - 256 * k
        halves.append((min(128, left), min(128, max(left - 128, 0))))
    assert halves == S1_HALVES[name]
    assert all(a > 0 for a, _ in halves)


def test_s1_a_pseudo_member_of_256_different_images():
    w, st, row_img = _s1()
    first, count = w['ranges']['r256']
    r0 = int(st[first])
    assert first >= 331, 'inside the last run of one-row images'
    win = row_img[r0:r0 + 256]
    assert len(set(win.tolist())) == 256 and win[-1] - win[0] == 255, 'img_n = 256 is needed, and is enough'
    # the whole split's last full pseudo-member (rows 768..1023) too holds more than 128 images
    assert len(set(row_img[768:1024].tolist())) > 128


def test_s1_the_300_row_image_straddles_a_pseudo_member_boundary():
    w, st, _ = _s1()
    a, b = int(st[130]), int(st[131])
    assert b - a == 300
    crossing = []
    for name, (first, count) in w['ranges'].items():
        r0, r1 = int(st[first]), int(st[first + count])
        if r0 <= a and b <= r1 and any(a - r0 < m < b - r0 for m in range(256, r1 - r0, 256)):
            crossing.append(name)
    assert {'r384', 'r385', 'r513', 'whole'} <= set(crossing)
    # and in one of them a sign half changes inside it as well
    first, _ = w['ranges']['r513']
    assert a - int(st[first]) < 256 < 384 < b - int(st[first])


# ---- slabs ----------------------------------------------------------------------------------------------------------------
def test_m1_every_slab_has_rows_of_length_0_and_T():
    w = W.member_inputs('M1')
    _, lab, _ = X.rows_of(*w['batches'][0])
    T = w['dims'].T
    n_words = (lab > 0).sum(1)
    assert lab.shape[0] == 300
    for slab in range(3):
        n = n_words[128 * slab:128 * (slab + 1)]
        assert n.shape[0] == (128, 128, 44)[slab]
        assert (n == 0).any() and (n == T).any() and (n == 1).any() and (n == 5).any()
    # the reduce loop's second pass: threads 0..43 take a second row
    assert 300 - 256 == 44


@pytest.mark.parametrize('name', ['M1', 'M2', 'M4', 'S2', 'D'])
def test_targets_reach_both_lane_halves_both_tiles_and_the_partial_stage(name):
    dims, sets = _all_label_sets()[name]
    assert dims.V1 == 68
    for lab in sets[:1] if name != 'D' else sets[1:]:
        mask = X.counted(lab)
        tgt = np.concatenate([lab, np.zeros((lab.shape[0], 1), lab.dtype)], 1)[mask]
        assert {int(t >> 2) & 1 for t in tgt} == {0, 1}, 'lane halves'
        first_stage = tgt[tgt < 64]
        assert {int(t >> 5) for t in first_stage} == {0, 1}, 'both 32-id tiles of a stage'
        assert (tgt >= 64).any() and (tgt == dims.V1 - 1).any(), 'the partial last stage and its last id'
        if name != 'D' or lab.shape[0] > 60:
            assert {3, 4, 31, 32, 63, 64, 67, 0} <= set(tgt.tolist())


def test_no_label_outside_the_vocabulary():
    for name, (dims, sets) in _all_label_sets().items():
        for lab in sets:
            assert lab.dtype == np.int32 and lab.min() >= 0 and lab.max() <= dims.V1 - 1, name
            assert lab.shape[1] == dims.T


# ---- M4: zeros inside label rows ------------------------------------------------------------------------------------------
def test_m4_kinds_stand_in_both_16_row_halves_of_a_group_and_in_two_groups():
    for kind in W.M4_KINDS:
        at = [r for r, k in W.M4_AT.items() if k == kind]
        assert {(r & 31) < 16 for r in at if r < 32} == {True, False}
        assert {r >> 5 for r in at} == {0, 1}


def test_m4_rows_are_of_their_kinds():
    w = W.member_inputs('M4')
    _, lab, _ = X.rows_of(*w['batches'][0])
    T = w['dims'].T
    for r, kind in W.M4_AT.items():
        row = lab[r]
        if kind == 'alt':
            assert (row[0::2] > 0).all() and (row[1::2] == 0).all()
        elif kind == 'lead0':
            assert row[0] == 0 and (row[1:3] > 0).all() and (row[3:] == 0).all()
        elif kind == 'full':
            assert (row > 0).all()
        elif kind == 'tail':
            assert (row[:T - 2] == 0).all() and (row[T - 2:] > 0).all()
        elif kind == 'zero':
            assert (row == 0).all()
        else:
            assert (row[:5] > 0).all() and (row[5:] == 0).all()
        want = W.m4_counted(kind, T)
        if want is not None:
            assert np.flatnonzero(X.counted(row[None])[0]).tolist() == want, kind


def test_m4_the_three_counts_agree_row_by_row():
    """counted(), n_tok and the non-zero steps of the restatement's lp; `last` = the last word's position + 1"""
    w = W.member_inputs('M4')
    _, lab, _ = X.rows_of(*w['batches'][0])
    r = W.m4_theta_ref()
    mask = X.counted(lab)
    assert np.array_equal(mask, r['mask'])
    assert np.array_equal(mask.sum(1), r['n_tok'])
    assert np.array_equal((r['lp'] != 0).sum(1), r['n_tok'])
    assert np.array_equal(r['lp'] != 0, mask)
    for i in range(lab.shape[0]):
        last = int(np.flatnonzero(mask[i]).max())
        nz = np.flatnonzero(lab[i] > 0)
        assert last == (int(nz.max()) + 1 if nz.size else 0)
        assert r['n_tok'][i] == 1 + nz.size
    assert np.isfinite(r['lp_sum']).all() and (r['lp_sum'] < 0).all()


# ---- the reduce order -----------------------------------------------------------------------------------------------------
def _tree(x):
    """a plain pairwise tree: element i meets element i + n / 2"""
    if len(x) == 1:
        return x[0]
    h = len(x) // 2
    return _tree([x[i] + x[i + h] for i in range(h)])


@pytest.mark.parametrize('n', [1, 5, 44, 128, 130, 255, 256, 257, 300, 513, 1229])
def test_reduce_order_against_fsum_and_the_plain_tree(n):
    rng = np.random.Generator(np.random.PCG64(40 + n))
    lp = -rng.random(n) * 60.0
    nt = rng.integers(1, 18, n).astype(np.int32)
    a, c = W.reduce_order(lp, nt)
    assert c == int(nt.sum())
    exact = math.fsum(lp.tolist())
    assert abs(a - exact) <= 1e-12 * abs(exact)
    assert W.reduce_fitness(lp, nt) == a / float(c)
    if n <= 256:
        padded = lp.tolist() + [0.0] * (256 - n)
        assert a == _tree(padded)
    else:
        # not a plain sum in row order in general: the order is part of the contract
        part = [0.0] * 256
        for i, v in enumerate(lp.tolist()):
            part[i % 256] += v
        assert a == _tree(part)


def test_reduce_order_on_the_worlds_rows_is_within_an_ulp_of_row_order():
    """lp_sum is a sum of fp32 values, so at these row counts every fp64 partial sum is exact and the device's order and
    xent_ref.loss_of's row order meet in the same bits; the random fp64 rows above are where the order shows"""
    for r in (W.m4_theta_ref(), W.flat_world('S1')['ref']):
        a, n = W.reduce_order(r['lp_sum'], r['n_tok'])
        assert n == int(r['n_tok'].sum())
        assert abs(-a / n - X.loss_of(r['lp_sum'], r['n_tok'])) <= 1e-12


# ---- drawn batches ----------------------------------------------------------------------------------------------------------
def test_draws_repeat_images_and_the_large_one_outgrows_the_first():
    w = W.drawn_inputs()
    assert len(w['gts']) == 40 and {g.shape[0] for g in w['gts']} == set(range(1, 8))
    for name, draw in W.DRAWS.items():
        a, b = draw
        assert len(a) == len(b) == {'first': 12, 'large': 30}[name]
        assert len(set(a)) < len(a) and len(set(b)) < len(b), 'an image twice inside a batch'
        assert set(a) & set(b), 'an image in both batches'
        assert min(a + b) >= 0 and max(a + b) < 40
    first, large = sum(W.draw_rows('first')), sum(W.draw_rows('large'))
    assert large > first + 8, 'the second draw outgrows a max_refs just above the first'
    assert W.draw_rows('first')[0] != W.draw_rows('first')[1]
