#!/usr/bin/env python3
"""What it costs to get an iteration's batches to the GPU: the host loader (CocoFcDataLoader.get_batch -> unique_batch
-> Engine.set_batches) against the resident training set (ResidentTrainLoader -> Engine.draw_batches), on one GPU at
the default dims, pop = 512, B = 128, screened default.

It writes a synthetic data set to a temporary directory first (--images per-image fc .npy files of N(0,1) rows, 5
random references each, the info json and the label store): the files CocoFcDataLoader reads. Nothing else is read.

  (a) wall time per EngineMaster.run iteration (perf_counter around a run that ends in a device synchronise), from the
      host loader, from the resident loader and from a FIXED batch (the GPU-only iteration: nothing is loaded), with
      single_batch true and with per-member batches at batches_per_iteration 8, 64 and 512. After a warm-up of every
      shape, --rounds interleaved rounds; medians with min-max. The headline is how far each loader sits above the
      GPU-only time.
      The resident loader's host side is also timed alone (get_batch for one iteration's batches, and the stack of
      their indices), so that what it adds to an iteration is measured and not inferred.
  (b) one draw against Engine.set_batches on the same images (1, 64 and 512 batches), from a set of --set-images random
      rows made in memory (the real split's 113,287: a 928 MB set is read from HBM, where (a)'s small split would sit in
      the Infinity Cache): device time (events around the call) and host time of the call (perf_counter, no
      synchronise inside the window). With --kernels (the
      scripts/trace_summary.py JSON of a `--draw-only` run under rocprofv3 --kernel-trace) the draw at 512 batches is
      split into fc gather, reference gather, cook and image tables, and the fc gather is put against the float4-copy
      ceiling (6.29 TB/s) as bytes moved (read + written) over kernel time.

  python scripts/trainset_ab.py --out profiles/trainset_ab.json [--kernels trace_summary.json]
  rocprofv3 --kernel-trace ... -- python scripts/trainset_ab.py --draw-only 512
"""
import argparse
import itertools
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'nes-img-captioning_amd'))

P, B = 512, 128
COPY_CEILING_TBS = 6.29          # measured float4 copy, the yardstick DESIGN.md 13 uses for nicnes_es_advance


def write_dataset(root, n_images, F, T, vocab, seed=0):
    from nicnes import data as Dt
    rng = np.random.Generator(np.random.PCG64(seed))
    images = [{'id': 1000 + i, 'split': 'train', 'file_path': '%d.jpg' % i} for i in range(n_images)]
    with open(os.path.join(root, 'cocotalk.json'), 'w') as f:
        json.dump({'ix_to_word': {str(i): 'w%d' % i for i in range(1, vocab + 1)}, 'images': images}, f)
    os.makedirs(os.path.join(root, 'fc'))
    for im in images:
        np.save(os.path.join(root, 'fc', '%d.npy' % im['id']), rng.standard_normal(F, dtype=np.float32))
    labels = random_labels(rng, n_images, T, vocab)
    start = 5 * np.arange(n_images) + 1
    Dt.LabelStore(labels, start, start + 4).save_npz(os.path.join(root, 'labels.npz'))
    return labels


def random_labels(rng, n_images, T, vocab):
    """5 zero-padded label rows of 8 .. T - 1 random words per image: [5 * n_images, T]."""
    labels = rng.integers(1, vocab + 1, (5 * n_images, T))
    lengths = rng.integers(8, T, (5 * n_images, 1))
    labels[np.arange(T)[None, :] >= lengths] = 0
    return labels


def big_set(e, n_images, dims):
    """A training set of n_images random rows made in memory (no files): (TrainSet, fc [n, F], labels [5 n, T])."""
    rng = np.random.Generator(np.random.PCG64(11))
    fc = rng.standard_normal((n_images, dims.F), dtype=np.float32)
    labels = random_labels(rng, n_images, dims.T, dims.vocab_size).astype(np.int32)
    return e.make_trainset(fc, labels.reshape(n_images, 5, dims.T)), fc, labels


def spec_for(G):
    from nicnes import config as C
    exp = {'algorithm': 'nic_nes', 'dataset': 'mscoco', 'nb_offspring': P,
           'config': {'noise_stdev': 0.01, 'batch_size': B, 'l2coeff': 1e-3, 'snapshot_freq': 0,
                      'single_batch': G == 1},
           'policy_options': {'net': 'fc_caption', 'fitness': 'greedy'},
           'optimizer_options': {'type': 'adam', 'args': {'stepsize': 1e-3}}}
    if G > 1:
        exp['batches_per_iteration'] = G
    return C.ExperimentSpec(exp)


def stats(v):
    return {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v)), 'all': [float(x) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=4096)
    ap.add_argument('--set-images', type=int, default=113287, help='rows of the in-memory set of (b): the COCO train split')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batches', default='1,8,64,512')
    ap.add_argument('--draw-only', type=int, default=0, metavar='G',
                    help='only 10 draws of G batches (the run to put under rocprofv3 --kernel-trace)')
    ap.add_argument('--kernels', default=None, help='trace_summary.py JSON of a --draw-only 512 run')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'trainset_ab.json'))
    a = ap.parse_args()
    import torch
    import nicnes
    import nicnes.synthetic as S
    from nicnes import data as Dt
    from nicnes import master as M
    from nicnes.validation import corpus_df
    if not torch.cuda.is_available():
        sys.exit('trainset_ab: needs a GPU (a timing on anything else says nothing)')
    dims = S.Dims()
    noise_len = 1 << 27
    e = nicnes.Engine(max_batch=B, max_members=P, noise_len=noise_len)
    e.set_noise_table(S.noise_table(noise_len))
    theta = S.init_theta(dims, 0, 4.0, 0.1)
    e.set_theta(theta)

    def set_df(labels, n):                  # the df table of the first n images' references
        keys, vals = corpus_df([labels[5 * i: 5 * i + 5].astype(np.int32) for i in range(n)])
        e.set_df_table(keys, vals, np.log(float(n)))

    if a.draw_only:
        ts, _, set_labels = big_set(e, a.set_images, dims)
        set_df(set_labels, 4096)
        ix = np.random.default_rng(1).integers(0, a.set_images, (a.draw_only, B)).astype(np.int32)
        for _ in range(10):
            e.draw_batches(ts, ix)
        torch.cuda.synchronize()
        ts.close()
        e.close()
        return

    root = tempfile.mkdtemp(prefix='trainset_ab_')
    try:
        t0 = time.perf_counter()
        labels = write_dataset(root, a.images, dims.F, dims.T, dims.vocab_size)
        t_write = time.perf_counter() - t0

        def loader(seed=0):
            return Dt.CocoFcDataLoader(os.path.join(root, 'cocotalk.json'), os.path.join(root, 'fc'),
                                       os.path.join(root, 'labels.npz'), batch_size=B, seed=seed)
        set_df(labels, a.images)
        t0 = time.perf_counter()
        res_loader = Dt.ResidentTrainLoader(loader(), e)
        torch.cuda.synchronize()
        t_resident = time.perf_counter() - t0

        out = {'device': torch.cuda.get_device_name(0), 'pop': P, 'B': B, 'images': a.images, 'rounds': a.rounds,
               'dataset_write_s': t_write, 'resident_set_build_s': t_resident,
               'note': 'the synthetic split is %d images (%.0f MB of fc files, all in the page cache after the first '
                       'pass): a real 113,287-image split reads colder files, so the host side here is a lower bound'
                       % (a.images, a.images * dims.F * 4 / 1e6)}

        # ---- (a) wall time per iteration -------------------------------------------------------------------
        def timed_run(m, batches, k, fixed=None):
            if fixed is not None:           # the GPU-only side: its batch is put on the device before the window
                m._batch_key = None
                m._set_batch(fixed)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.run(batches, max_iterations=m.sched.iteration + k)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / k * 1e3

        out['iteration_ms'] = {}
        for G in [int(g) for g in a.batches.split(',')]:
            spec = spec_for(G)
            k_fast, k_host = (4, 4) if G <= 8 else ((3, 2) if G <= 64 else (2, 1))
            sides = {}
            for name in ('gpu_only', 'resident', 'host'):
                e.set_adam_state(np.zeros(e.D), np.zeros(e.D), 0)
                sides[name] = M.EngineMaster(spec, e, theta=theta)
            host_l = loader(1)
            got = [host_l.get_batch('train', batch_size=B) for _ in range(G)]
            fixed = got[0] if G == 1 else got
            feeds = {'gpu_only': lambda k: itertools.repeat(fixed, k), 'resident': lambda k: res_loader,
                     'host': lambda k: host_l}
            ks = {'gpu_only': k_fast, 'resident': k_fast, 'host': k_host}
            for name in ('gpu_only', 'resident', 'host'):                       # warm-up of every shape
                timed_run(sides[name], feeds[name](1), 1, fixed if name == 'gpu_only' else None)
            ms = {name: [] for name in sides}
            for _ in range(a.rounds):
                for name in ('gpu_only', 'resident', 'host'):
                    ms[name].append(timed_run(sides[name], feeds[name](ks[name]), ks[name],
                                              fixed if name == 'gpu_only' else None))
            r = {name: stats(v) for name, v in ms.items()}
            # the resident loader's host side alone: get_batch (the walk of the wrapped loader's iterator, the infos and
            # the DrawnBatch objects) for one iteration's batches, and the stack of their indices
            walk = []
            for _ in range(a.rounds):
                t0 = time.perf_counter()
                drawn = [res_loader.get_batch('train', batch_size=B) for _ in range(G)]
                t1 = time.perf_counter()
                np.stack([d['image_ix'] for d in drawn])
                walk.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
            r['resident_get_batch_ms'] = stats([w[0] for w in walk])
            r['resident_index_stack_ms'] = stats([w[1] for w in walk])
            r['iterations_per_window'] = ks
            for name in ('resident', 'host'):
                r[name + '_over_gpu_only_ms'] = r[name]['median'] - r['gpu_only']['median']
                r[name + '_over_gpu_only_ratio'] = r[name]['median'] / r['gpu_only']['median']
            out['iteration_ms']['batches_%d' % G] = r
            print('(a) G=%d' % G, json.dumps({k: (v['median'] if isinstance(v, dict) and 'median' in v else v)
                                             for k, v in r.items()}), flush=True)
            del got, fixed

        # ---- (b) one draw against set_batches --------------------------------------------------------------
        # on a set of the real split's size (--set-images rows in memory, no files): the gather then reads HBM, where
        # the small on-disk split of (a) would sit in the Infinity Cache
        res_loader.close()
        out['one_call'] = {'set_images': a.set_images}
        ts, set_fc, set_labels = big_set(e, a.set_images, dims)
        for G in (1, 64, 512):
            ix = np.random.default_rng(G).integers(0, a.set_images, (G, B)).astype(np.int32)
            host_batches = [(set_fc[row], [set_labels[5 * i: 5 * i + 5] for i in row]) for row in ix]

            def call(fn):
                torch.cuda.synchronize()
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                t0 = time.perf_counter()
                fn()
                host_ms = (time.perf_counter() - t0) * 1e3
                ev1.record()
                ev1.synchronize()
                return host_ms, ev0.elapsed_time(ev1)
            fns = {'draw': lambda: e.draw_batches(ts, ix), 'set_batches': lambda: e.set_batches(host_batches)}
            for fn in fns.values():
                for _ in range(2):
                    fn()
            ms = {k: ([], []) for k in fns}
            for _ in range(a.rounds):
                for k, fn in fns.items():
                    h, d = call(fn)
                    ms[k][0].append(h)
                    ms[k][1].append(d)
            # the same state: compare the bytes
            e.set_batches(host_batches)
            want = [t.clone() for t in e.test_batch_state(5 * G * B)]
            e.draw_batches(ts, ix)
            same = all(torch.equal(x, y) for x, y in zip(e.test_batch_state(5 * G * B), want))
            out['one_call']['batches_%d' % G] = {
                'same_batch_state': bool(same),
                'draw_host_ms': stats(ms['draw'][0]), 'draw_device_ms': stats(ms['draw'][1]),
                'set_batches_host_ms': stats(ms['set_batches'][0]), 'set_batches_device_ms': stats(ms['set_batches'][1]),
                'fc_bytes_moved': 2 * G * B * dims.F * 4}
            print('(b) G=%d' % G, json.dumps({k: (v['median'] if isinstance(v, dict) else v)
                                             for k, v in out['one_call']['batches_%d' % G].items()}), flush=True)
            del host_batches

        if a.kernels:
            with open(a.kernels) as f:
                kern = json.load(f)['kernels']
            split = {}
            for name, d in kern.items():
                part = ('fc_gather' if 'gather_fc' in name else 'ref_gather' if 'gather_refs' in name else
                        'image_tables' if ('img_ngram' in name or 'fill' in name.lower()) else
                        'cook' if 'cook' in name else None)
                if part and d['launches_full_grid'] >= 5:
                    split.setdefault(part, {'ms': 0.0, 'kernels': {}})
                    split[part]['ms'] += d['mean_ms_full_grid']
                    split[part]['kernels'][name] = d['mean_ms_full_grid']
            moved = 2 * 512 * B * dims.F * 4
            if 'fc_gather' in split:
                tbs = moved / (split['fc_gather']['ms'] * 1e-3) / 1e12
                split['fc_gather'].update({'bytes_moved': moved, 'TB_per_s': tbs, 'ceiling_TB_per_s': COPY_CEILING_TBS,
                                           'share_of_float4_copy_ceiling': tbs / COPY_CEILING_TBS})
            out['draw_512_kernels'] = {'source': 'rocprofv3 --kernel-trace of 10 draws of 512 batches, a run of its own; '
                                                 'mean kernel time of the full-grid launches', 'parts': split}
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out))
        ts.close()
        e.close()
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == '__main__':
    main()
