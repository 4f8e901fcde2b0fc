"""CPU: the host restatement of the beam-search decode (tests/beam_ref.py) and the inputs of the GPU tests.

With K = 1 the restatement is the oracle's greedy decode (tokens on every row the oracle does not mark fragile,
log-probs within the project's 1e-5 bar). The definition's edge rules are checked on hand-made log-prob tables. Every
workload tests/test_gpu_beam.py decodes is checked here, under the restatement alone, to be worth decoding: in every
case (the images decoded at one width) at most FRAGILE_CAP are fragile (a condition: change the seed or theta's gain
and biases, never the cap), and the workload holds an image whose K = 3 caption differs from the greedy one, one whose
winner finished after another hypothesis had finished, and one that reaches step T. The workload of seq_length 1 has a
single step: its best word is the greedy one and nothing can finish earlier, so it can only hold the last. The C ABI,
the built library and the ctypes table all name the new entries."""
import os
import re

import numpy as np
import pytest

from oracle import oracle as O
from tests import beam_ref as BR
from tests.beam_ref import FRAGILE_CAP

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_STEP = ('v128_t1',)       # seq_length 1
NEW_ENTRIES = ('nicnes_split_decode_beam', 'nicnes_split_evaluate_beam', 'nicnes_test_beam_select',
               'nicnes_set_beam_waves')


def test_fragile_gap_is_the_derived_one():
    src = open(os.path.join(REPO, 'tests', 'test_gpu_es.py')).read()
    assert re.search(r'^FRAGILE_CAP = 0\.10\b', src, re.M) and FRAGILE_CAP == 0.10      # the project's cap, not ours
    assert BR.FRAGILE_GAP == pytest.approx(2 * 16 * 1e-5) and BR.SCORE_TOL == pytest.approx(16 * 1e-5)


# ------------------------------------------------------------------ K = 1 is the oracle's greedy decode -------------
@pytest.mark.parametrize('name', ['v8', 'v68_t3', 'v128'])
def test_beam_1_restates_the_oracle(name):
    dims, theta, fc, _ = BR.workload_inputs(name)
    fc = fc[:24]
    oseq, olp, fragile = O.decode(dims, theta, fc)
    model = BR.Model(dims, theta)
    kept = 0
    for i in range(fc.shape[0]):
        if fragile[i].any():
            continue
        kept += 1
        r = BR.beam_search(model, fc[i], 1)
        assert np.array_equal(r['tokens'], oseq[i]), (name, i)
        n = int(np.argmax(oseq[i] == 0)) + 1 if (oseq[i] == 0).any() else dims.T    # steps up to the end token
        assert abs(r['score'] - float(olp[i, :n].astype(np.float64).sum())) <= n * 1e-5, (name, i)
    assert kept >= 0.9 * fc.shape[0]


def test_restatement_log_probs_are_the_oracles():
    """one step, every id: the root's log-prob row against the oracle's lp of the greedy token"""
    dims, theta, fc, _ = BR.workload_inputs('v128')
    model = BR.Model(dims, theta)
    oseq, olp, _ = O.decode(dims, theta, fc[:8])
    for i in range(8):
        lp = model.logprobs(model.start(fc[i])[0])
        assert lp.dtype == np.float32 and int(np.argmax(lp)) == oseq[i, 0]
        assert abs(float(lp.max()) - float(olp[i, 0])) <= 1e-5


# ------------------------------------------------------------------ the edge rules on hand-made tables -------------
def _row(V1, **kw):
    """a log-prob row: -20 everywhere but the given ids (v3=-0.5 -> id 3)"""
    r = np.full(V1, -20.0, np.float32)
    for k, v in kw.items():
        r[int(k[1:])] = v
    return r


def test_vocabulary_smaller_than_the_beam():
    """V1 = 3 < K = 5: step 1 has 3 candidates, the live set holds 2 (id 0 finishes), step 2 has 6"""
    rows = {(): [-1.0, -0.5, -2.0], (1,): [-0.1, -3.0, -4.0], (2,): [-5.0, -0.2, -0.3]}
    r = BR.table_search(lambda p: rows.get(p, [-1.0, -1.0, -1.0]), 5, 2)
    assert sorted(f[1] for f in r['finished']) == [1, 2, 2, 2, 2, 2]
    assert r['tokens'].tolist() == [1, 0] and r['score'] == pytest.approx(-0.6)


def test_a_finisher_is_overtaken_later():
    """the end token is taken at step 1 with -1.2; the hypothesis that went on finishes at step 3 with -0.9"""
    def tab(p):
        if p == ():
            return _row(6, v0=-1.2, v2=-0.4, v3=-3.0)
        if p == (2,):
            return _row(6, v4=-0.3, v0=-2.5)
        if p == (2, 4):
            return _row(6, v0=-0.2, v1=-2.0)
        return _row(6, v0=-9.0)
    r = BR.table_search(tab, 2, 4)
    assert r['tokens'].tolist() == [2, 4, 0, 0] and r['score'] == pytest.approx(-0.9) and r['late_winner']
    g = BR.table_search(tab, 1, 4)
    assert g['tokens'].tolist() == [2, 4, 0, 0]


def test_equal_scores_across_beams_take_the_lower_beam_then_the_lower_id():
    lp = np.full((3, 8), -5.0, np.float32)
    lp[0, 6] = lp[1, 2] = lp[2, 1] = -1.0          # the same candidate score from three beams
    lp[1, 5] = -1.0                                # and twice in beam 1
    cand = BR.select(lp, np.zeros(3), [True, True, True], 3)
    assert [(b, v) for _, b, v in cand[:3]] == [(0, 6), (1, 2), (1, 5)]
    cand = BR.select(lp, np.zeros(3), [True, False, True], 3)      # a dead row gives no candidate
    assert [(b, v) for _, b, v in cand[:3]] == [(0, 6), (2, 1), (0, 0)]


def test_a_tie_between_finished_hypotheses_goes_to_the_earlier_one():
    """-1 at step 1 and -0.5 - 0.5 at step 2 (exact in fp64): the step-1 finisher wins; two ties of one step go by
    selection order"""
    def tab(p):
        if p == ():
            return _row(6, v0=-1.0, v3=-0.5)
        if p == (3,):
            return _row(6, v0=-0.5, v1=-4.0)
        return _row(6, v0=-9.0)
    r = BR.table_search(tab, 2, 3)
    assert r['tokens'].tolist() == [0, 0, 0] and r['score'] == -1.0 and r['fragile']

    def tab2(p):
        if p == ():
            return _row(6, v2=-0.5, v4=-0.5)
        return _row(6, v0=-0.25, v1=-7.0)
    r = BR.table_search(tab2, 2, 3)
    assert r['tokens'].tolist() == [2, 0, 0] and r['score'] == -0.75


def test_reaching_T_without_an_end_token():
    r = BR.table_search(lambda p: _row(6, v5=-0.1, v4=-0.7, v0=-30.0), 3, 4)
    assert r['tokens'].tolist() == [5, 5, 5, 5] and r['reached_T'] and r['score'] == pytest.approx(-0.4)
    assert not r['late_winner']


# ------------------------------------------------------------------ the GPU tests' inputs ---------------------------
@pytest.mark.parametrize('name', list(BR.WORKLOADS))
def test_gpu_workload_is_not_vacuous_and_mostly_checkable(name):
    dims, theta, fc, cases, ref = BR.workload(name)
    model = BR.Model(dims, theta)
    for K, first, count in cases:
        n = sum(ref[(K, i)]['fragile'] for i in range(first, first + count))
        print('%s K = %d, %d images from %d: %d fragile' % (name, K, count, first, n))
        assert n <= FRAGILE_CAP * count, \
            '%s K = %d: %d of %d images fragile: change the seed or theta, not the cap' % (name, K, n, count)
    sound = [(K, i, r) for (K, i), r in ref.items() if not r['fragile']]
    assert any(r['reached_T'] for _, _, r in sound)
    if name in ONE_STEP:
        return
    assert any(r['late_winner'] for _, _, r in sound)
    k3 = [(i, r) for K, i, r in sound if K == 3]
    assert any(not np.array_equal(r['tokens'], BR.beam_search(model, fc[i], 1)['tokens']) for i, r in k3[:40])


def test_the_restatement_stops_where_the_definition_allows():
    """-0.5 finished at step 1, the live hypothesis at -1.0 cannot catch up: no later step is asked for"""
    asked = []

    def tab(p):
        asked.append(p)
        return _row(6, v0=-0.5, v2=-1.0)
    r = BR.table_search(tab, 2, 5)
    assert asked == [()] and r['tokens'].tolist() == [0] * 5 and r['score'] == -0.5 and not r['fragile']
    r = BR.table_search(lambda p: _row(6, v0=-0.5, v2=-0.5001) if p == () else _row(6, v0=-3.0), 2, 5)
    assert r['fragile']                          # within the gap, another implementation may go on a step


# ------------------------------------------------------------------ the ABI names the new entries -------------------
def test_header_library_and_ctypes_table_name_the_beam_entries():
    from nicnes import _lib
    header = open(os.path.join(REPO, 'include', 'nicnes.h')).read()
    L = _lib.lib()
    for name in NEW_ENTRIES:
        assert re.search(r'\bint %s\(' % name, header), name
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
