"""CPU: the step queue's host rules through nicnes_decode_queue_plan (which kernel a screened fused decode runs for which
members, slabs, workers and mode, the environment variables included; the ring size), and the new entries' place in the
header and the binding."""
import os
import re

import pytest

from nicnes import _lib
from nicnes.engine import decode_queue_plan

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'nicnes.h')


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    monkeypatch.delenv('NICNES_DECODE_QUEUE', raising=False)
    monkeypatch.delenv('NICNES_DECODE_QUEUE_WORKERS', raising=False)


@pytest.mark.parametrize('members,slabs,n_cu,mode,workers,want', [
    (512, 1, 256, 'auto', 0, (True, 256)),      # the flagship line: two member slabs per CU
    (257, 1, 256, 'auto', 0, (True, 256)),
    (256, 1, 256, 'auto', 0, (False, 256)),     # at the worker count: every member slab resident, the one-launch kernel
    (64, 1, 256, 'auto', 0, (False, 64)),
    (200, 2, 256, 'auto', 0, (True, 256)),      # member slabs, not members, are the tasks
    (128, 2, 256, 'auto', 0, (False, 256)),
    (512, 1, 256, 0, 0, (False, 256)),          # off
    (3, 1, 256, 1, 0, (True, 3)),               # forced on below the worker count: one worker per member slab
    (13, 1, 256, 1, 5, (True, 5)),              # a forced worker count
    (5, 1, 256, 'auto', 4, (True, 4)),
    (4, 1, 256, 'auto', 4, (False, 4)),
    (512, 1, 304, 'auto', 0, (True, 304)),      # another CU count
])
def test_path_rule(members, slabs, n_cu, mode, workers, want):
    use, grid, _ = decode_queue_plan(members, slabs, n_cu, mode, workers)
    assert (use, grid) == want


@pytest.mark.parametrize('env,want', [
    ({}, (True, 256)),                                                          # default: auto, one worker per CU
    ({'NICNES_DECODE_QUEUE': '0'}, (False, 256)),
    ({'NICNES_DECODE_QUEUE': '2'}, (True, 256)),
    ({'NICNES_DECODE_QUEUE': '1', 'NICNES_DECODE_QUEUE_WORKERS': '7'}, (True, 7)),
    ({'NICNES_DECODE_QUEUE': '2', 'NICNES_DECODE_QUEUE_WORKERS': '600'}, (False, 512)),   # auto: not above the worker count
    ({'NICNES_DECODE_QUEUE': '3'}, (True, 256)),                                # not a mode: the default stays
    ({'NICNES_DECODE_QUEUE': 'on', 'NICNES_DECODE_QUEUE_WORKERS': '0'}, (True, 256)),
    ({'NICNES_DECODE_QUEUE': '2', 'NICNES_DECODE_QUEUE_WORKERS': '0'}, (True, 256)),   # no worker count: one per CU
])
def test_path_rule_from_the_environment(monkeypatch, env, want):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    use, grid, _ = decode_queue_plan(512, 1, 256)
    assert (use, grid) == want


@pytest.mark.parametrize('items,slots', [(1, 1), (2, 2), (3, 4), (13, 16), (256, 256), (257, 512), (512, 512), (513, 1024)])
def test_ring_size_is_the_power_of_two_at_or_above_the_member_slabs(items, slots):
    assert decode_queue_plan(items, 1, 256, 1, 0)[2] == slots
    assert slots >= items and slots & (slots - 1) == 0 and (slots == 1 or slots // 2 < items)


def test_plan_rejects_bad_arguments():
    for args in ((0, 1, 256, 1, 0), (4, 0, 256, 1, 0), (4, 1, 0, 1, 0), (4, 1, 256, 3, 0), (4, 1, 256, 1, -1)):
        with pytest.raises(_lib.NicnesError):
            decode_queue_plan(*args)


def test_new_entries_are_declared_and_bound():
    text = open(HEADER).read()
    for name in ('nicnes_set_decode_queue', 'nicnes_decode_queue_plan'):
        assert re.search(r'\bint %s\(' % name, text), name
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().nicnes_set_decode_queue(None, 1, 0) == _lib.ERR_INVALID      # a null handle fails cleanly
