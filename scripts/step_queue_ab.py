#!/usr/bin/env python3
"""A/B of the screened decode's step queue on the bench workload: the parent commit's tree against this tree (the queue
wherever the decode has more member slabs than CUs) and this tree with NICNES_DECODE_QUEUE=0 (the parent's kernel),
interleaved on one GPU in one session, each run a fresh process.

    git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/nes-img-captioning_amd     (any checkout of the parent, built)
    python scripts/step_queue_ab.py --parent /tmp/parent --rounds 5 --out profiles/step_queue_bench_ab.json
    python scripts/step_queue_ab.py --parent /tmp/parent --shapes --out profiles/step_queue_bench_other_shapes.json

Every run is `bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR` (+ a shape's arguments) of its tree, started
through this file's --child mode, which only adds one thing to the bench process: the engine's stats() are written to
a file when the bench closes its engine (bench.py prints tie_fallbacks alone). The arrays of --dump-outputs (fitness,
noise_sum, theta, update_ratio) are compared bit for bit across the arms of a round and then deleted.

The bar (the rule the decode changes before this one were held to): every run of this tree above every run of the
parent, and median ratio >= 1 + 5 x (the two arms' relative spreads, (max - min) / median, added). This tree with the
queue off must equal the parent within the two arms' spreads."""
import argparse
import json
import os
import runpy
import shutil
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = ['--gpus', '1', '--steps', '20', '--warmup', '5']
SHAPES = {'--population 256': ['--population', '256'], '--population 64': ['--population', '64'],
          '--theta-gain 4 --bias-std 0.1': ['--theta-gain', '4', '--bias-std', '0.1'],
          '--preset configs3': ['--preset', 'configs3']}
ARRAYS = ('fitness', 'noise_sum', 'theta', 'update_ratio')
COUNTERS = ('tie_fallbacks', 'screen_candidates', 'screen_fallback_rows', 'screen_rows_over_cap', 'screen_rows_undecided',
            'screen_rows_evicted', 'screen_rows_nonfinite', 'screen_rows_settled_later', 'screen_resweep_rows',
            'screen_resweep_steps', 'screen_resweep_waves')


def child(tree, stats_path, bench_args):
    """bench.py of `tree` in this process, with the engine's stats() saved at close."""
    sys.path[:0] = [tree, os.path.join(tree, 'nes-img-captioning_amd')]
    import nicnes
    close = nicnes.Engine.close

    def close_and_tell(self):
        if not os.path.exists(stats_path):          # (close runs again when the object is collected)
            st = {k: int(v) for k, v in self.stats().items()}
            with open(stats_path, 'w') as f:
                json.dump(st, f)
        close(self)
    nicnes.Engine.close = close_and_tell
    sys.argv = [os.path.join(tree, 'bench.py')] + bench_args
    runpy.run_path(sys.argv[0], run_name='__main__')


def run(tree, extra, env_add, tmp, tag):
    dump, stats_path = os.path.join(tmp, tag), os.path.join(tmp, tag + '.json')
    env = dict(os.environ, **env_add)
    cmd = ([sys.executable, os.path.abspath(__file__), '--child', tree, stats_path, '--'] + BENCH + extra +
           ['--dump-outputs', dump])
    r = subprocess.run(cmd, cwd=tree, env=env, capture_output=True, text=True, timeout=400)
    if r.returncode != 0:
        sys.exit('%s failed (%d):\n%s' % (tag, r.returncode, r.stderr[-3000:]))
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    with open(stats_path) as f:
        st = json.load(f)
    os.remove(stats_path)
    arrays = {a: np.load(os.path.join(dump, a + '.npy')) for a in ARRAYS}
    shutil.rmtree(dump)
    return rec, st, arrays


def same_bits(a, b):
    return all(a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in ARRAYS)


def spread(v):
    return (max(v) - min(v)) / float(np.median(v))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--child':
        return child(sys.argv[2], sys.argv[3], sys.argv[5:])
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', required=True, help='a built checkout of the parent commit')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--shapes', action='store_true', help='one interleaved pair of each other shape instead')
    ap.add_argument('--out', required=True)
    a = ap.parse_args()
    parent = os.path.abspath(a.parent)
    tmp = tempfile.mkdtemp(prefix='step_queue_ab_')
    try:
        if a.shapes:
            out = {'command': 'one interleaved pair each, parent then this tree: bench.py %s + the arguments named; '
                              'counters from eng.stats() at the end of each run' % ' '.join(BENCH), 'pairs': {}}
            for name, extra in SHAPES.items():
                rp, sp, ap_ = run(parent, extra, {}, tmp, 'parent')
                rq, sq, aq = run(REPO, extra, {}, tmp, 'pr')
                out['pairs'][name] = {
                    'parent': rp['value'], 'pr': rq['value'], 'ratio': rq['value'] / rp['value'],
                    'decode_path': rq['roofline']['decode']['path'], 'queue_steps': sq.get('queue_steps', 0),
                    'takes_the_step_queue': sq.get('queue_steps', 0) > 0,
                    'outputs_bit_identical': same_bits(ap_, aq),
                    'counters_equal': all(sp[k] == sq[k] for k in COUNTERS),
                    'counters': {k: [sp[k], sq[k]] for k in COUNTERS}}
                print(name, json.dumps({k: v for k, v in out['pairs'][name].items() if k != 'counters'}), flush=True)
        else:
            arms = {'parent': (parent, {}), 'pr': (REPO, {}), 'pr_queue_off': (REPO, {'NICNES_DECODE_QUEUE': '0'})}
            res = {k: {'members_per_s': [], 'ms_per_step': [], 'kernel_ms_per_launch': [], 'queue_steps_per_run': [],
                       'queue_timeouts_per_run': [], 'counters_per_run': []} for k in arms}
            bits, counters = [], []
            for r in range(a.rounds):
                got = {}
                for k, (tree, env) in arms.items():
                    rec, st, arrays = run(tree, [], env, tmp, k)
                    got[k] = (st, arrays)
                    res[k]['members_per_s'].append(rec['value'])
                    res[k]['ms_per_step'].append(rec['ms_per_step'])
                    res[k]['kernel_ms_per_launch'].append(rec['roofline']['kernel_ms_per_launch'])
                    res[k]['queue_steps_per_run'].append(st.get('queue_steps', 0))
                    res[k]['queue_timeouts_per_run'].append(st.get('queue_timeouts', 0))
                    res[k]['counters_per_run'].append({c: st[c] for c in COUNTERS})
                    print(r, k, rec['value'], rec['ms_per_step'], flush=True)
                bits.append(all(same_bits(got['parent'][1], got[k][1]) for k in ('pr', 'pr_queue_off')))
                counters.append(all(got['parent'][0][c] == got[k][0][c] for k in ('pr', 'pr_queue_off') for c in COUNTERS))
            for k in arms:
                v = res[k]['members_per_s']
                res[k]['median'] = float(np.median(v))
                res[k]['spread'] = spread(v)
            bar = 1.0 + 5.0 * (res['parent']['spread'] + res['pr']['spread'])
            ratio = res['pr']['median'] / res['parent']['median']
            out = dict(res)
            out.update({
                'ratio_of_medians': ratio, 'acceptance_bar': bar, 'meets_bar': bool(ratio >= bar),
                'every_pr_run_beats_every_parent_run': bool(min(res['pr']['members_per_s']) >
                                                            max(res['parent']['members_per_s'])),
                'ratio_of_medians_queue_off': res['pr_queue_off']['median'] / res['parent']['median'],
                'queue_off_within_spread_of_parent': bool(
                    abs(res['pr_queue_off']['median'] / res['parent']['median'] - 1.0) <=
                    res['parent']['spread'] + res['pr_queue_off']['spread']),
                'last_step_outputs_bit_identical_per_round': bits, 'counters_equal_per_round': counters,
                'command': 'bench.py %s --dump-outputs DIR; parent, this tree and this tree with NICNES_DECODE_QUEUE=0 '
                           'interleaved on one GPU in one session, %d rounds, a fresh process per run' %
                           (' '.join(BENCH), a.rounds)})
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
        print(json.dumps({k: v for k, v in out.items() if k not in ('parent', 'pr', 'pr_queue_off', 'pairs')}, indent=1))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
