"""CPU: the host side of the beam-search evaluation. Validator(beam_size=K) passes K to the split's evaluate and
Validator() passes no beam keyword at all (so the greedy path, and any engine without a beam decode, is called as
before); python -m nicnes.evaluate takes --beam_size 1..8; Split's argument check refuses a width outside 1..8 before
anything reaches the engine."""
import numpy as np
import pytest

from nicnes import evaluate as EV
from nicnes import validation as V


class _Split:
    def __init__(self):
        self.calls = []

    def evaluate(self, return_seq=False, **kw):
        self.calls.append(dict(kw, return_seq=return_seq))
        stats = {k: 0.5 for k in V.METRIC_KEYS}
        return (stats, np.asarray([[3, 1, 0, 0], [2, 0, 0, 0]], np.int32)) if return_seq else stats

    def close(self):
        pass


class _Engine:
    def make_split(self, fc, gts=None, df=None, ref_len_raw=None):
        self.split = _Split()
        return self.split


class _Labels:
    labels = np.asarray([[3, 1, 0, 0], [2, 2, 0, 0], [1, 0, 0, 0]], np.int32)
    label_start_ix = np.asarray([1, 3])
    label_end_ix = np.asarray([2, 3])


class _Loader:
    split_ix = {'val': [0, 1]}
    info = {'images': [{'id': 11}, {'id': 12}]}
    ix_to_word = {'1': 'a', '2': 'b', '3': 'c'}
    seq_length = 4
    labels = _Labels()

    def fc_feature(self, ix):
        return np.zeros(8, np.float32)


def test_validator_passes_the_beam_only_when_one_is_given():
    e = _Engine()
    v = V.Validator(e, _Loader(), 'val', 2)
    stats, preds = v.eval_split()
    v.accuracy()
    assert e.split.calls == [{'return_seq': True}, {'return_seq': False}]
    assert [p['caption'] for p in preds] == ['c a', 'b']
    v = V.Validator(e, _Loader(), 'val', 2, beam_size=3)
    v.eval_split()
    assert v.accuracy() == 0.5
    assert e.split.calls == [{'return_seq': True, 'beam_size': 3}, {'return_seq': False, 'beam_size': 3}]
    for bad in (0, 9):
        with pytest.raises(ValueError):
            V.Validator(e, _Loader(), 'val', 2, beam_size=bad)


def test_cli_takes_a_beam_size():
    base = ['--exp', 'x.json', '--model', 'm.pth', '--out', 'o.json']
    assert EV.parse_args(base).beam_size is None
    assert EV.parse_args(base + ['--beam_size', '5']).beam_size == 5
    for bad in ('0', '9'):
        with pytest.raises(SystemExit):
            EV.parse_args(base + ['--beam_size', bad])


def test_split_refuses_a_width_outside_1_to_8():
    from nicnes.engine import Split
    assert [Split._beam(k) for k in (1, 8)] == [1, 8]
    for bad in (0, 9, -3):
        with pytest.raises(ValueError):
            Split._beam(bad)
