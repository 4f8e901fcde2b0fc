#!/usr/bin/env python3
"""The teacher-forced forward (csrc/xent_kernels.hip) timed on one GPU beside the decodes of the same row count, in one
process, at V1 = 9488, F = 2048, E = R = 128, T = 16:

  split     Split.xent over 5,120 images x 5 label rows      | Split.decode of 25,600 images (25,600 rows each side)
  evaluate  one 'xent' evaluate at P = 512, B = 128 x 5 rows | the 'sample' mode's evaluate of the same 640 rows
                                                               (rows_per_image = 5; decode + CIDEr-D)

HIP events on the stream, a warm-up of every side, `--runs` interleaved rounds of `--reps` passes; medians with min - max.
The label rows are synthetic references of the model's own greedy captions (nicnes.synthetic.build_references), so the
two sides of a pair run captions of like length; every side's step counts are recorded. FLOPs of the xent sides are
counted from the rows' targets: per row the image projection 2 F E and one cell, per target one cell 2 (5 R E + 5 R R)
and one logit product 2 V1 R (a greedy decode's count plus the one logit product a full-length row's end target adds),
twice for an evaluate's two signs; the fraction is that count over the 157.3 TFLOP/s fp32 MFMA peak, a whole-call
figure. There is no threshold: the numbers are only recorded.

  python scripts/xent_ab.py --out profiles/xent_ab.json"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'nes-img-captioning_amd'))
PEAK = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=512)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--images', type=int, default=5120)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--noise_len', type=int, default=1 << 25)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'xent_ab.json'))
    a = ap.parse_args()
    import torch
    import nicnes
    import nicnes.synthetic as S
    if not torch.cuda.is_available():
        sys.exit('xent_ab: needs a GPU (a timing on anything else says nothing)')
    P, B, N, SIGMA, RPI = a.members, a.batch, a.images, 0.01, 5
    e = nicnes.Engine(max_batch=B * RPI, max_members=P, noise_len=a.noise_len)
    w = S.setup_engine_workload(e, B=B, noise=S.noise_table(a.noise_len))
    cfg = e.cfg
    V1, F, E, R, T = cfg.vocab_size + 1, cfg.fc_feat_size, cfg.input_encoding_size, cfg.rnn_size, cfg.seq_length
    cell, logit, img = 2 * (5 * R * E + 5 * R * R), 2 * V1 * R, 2 * F * E

    def flops(n_rows, n_targets, signs=1):
        return signs * (n_rows * (img + cell) + n_targets * (cell + logit))

    # the split sides: 25,600 images to decode; the first N of them with 5 references each for the loss
    fc = S.fc_feats(N * RPI, F, 4321, False)
    sp_d = e.make_split(fc)
    base = sp_d.decode(0, N).cpu().numpy()
    gts, _, _ = S.build_references(base, cfg.vocab_size, 99, RPI, N, T)
    sp_x = e.make_split(fc[:N], gts)
    x = sp_x.xent()
    seq = sp_d.decode().cpu().numpy()
    dec_steps = np.minimum((seq > 0).sum(1) + 1, T)
    batch_targets = int(sum((np.asarray(g) > 0).sum() + len(g) for g in w['gts']))
    info = {
        'split_xent': {'rows': int(x['n_tok'].numel()), 'targets': x['tokens'], 'loss': x['loss'],
                       'flops': flops(int(x['n_tok'].numel()), x['tokens'])},
        'split_decode': {'rows': int(seq.shape[0]), 'logit_steps': int(dec_steps.sum()),
                         'flops': flops(int(seq.shape[0]), int(dec_steps.sum()))},
        'evaluate_xent': {'rows': B * RPI, 'targets_per_candidate': batch_targets,
                          'flops': flops(B * RPI, batch_targets, 2 * P)},
        'evaluate_sample': {'rows': B * RPI},
    }

    def mode(name):
        e.set_fitness_mode(name)
        e.set_rows_per_image(RPI if name == 'sample' else 1)

    sides = {
        'split_xent': lambda it: sp_x.xent(),
        'split_decode': lambda it: sp_d.decode(),
        'evaluate_xent': lambda it: (mode('xent'), e.evaluate(it, 0, P, SIGMA)),
        'evaluate_sample': lambda it: (mode('sample'), e.evaluate(it, 0, P, SIGMA)),
    }

    def timed(fn, it):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for r in range(a.reps):
            fn(it + r)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / a.reps

    for fn in sides.values():                       # warm-up of every side (buffers grow here)
        fn(1)
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for run in range(a.runs):                       # interleaved rounds
        for name, fn in sides.items():
            ms[name].append(timed(fn, 10 + 10 * run))
    res = {'members': P, 'batch_images': B, 'rows_per_image': RPI, 'split_images': N, 'runs': a.runs,
           'reps_per_run': a.reps, 'device': torch.cuda.get_device_name(0), 'fp32_mfma_peak_flops': PEAK, 'sides': {}}
    for name in sides:
        med = float(np.median(ms[name]))
        d = dict(info[name], ms=ms[name], median_ms=med, min_ms=float(min(ms[name])), max_ms=float(max(ms[name])))
        if 'flops' in d:
            d['fraction_of_fp32_mfma_peak'] = d['flops'] / (med * 1e-3) / PEAK
        res['sides'][name] = d
    s = res['sides']
    res['split_xent_over_split_decode'] = s['split_xent']['median_ms'] / s['split_decode']['median_ms']
    res['evaluate_xent_over_evaluate_sample'] = s['evaluate_xent']['median_ms'] / s['evaluate_sample']['median_ms']
    res['not_measured'] = ['other batch sizes, populations and vocabularies', 'several GPUs', 'per-kernel counters '
                           '(rocprofv3) of the xent kernel', 'the xent kernel with h and c held in registers instead of '
                           'the wide frame\'s lane scratch', 'label rows of a trained model\'s data (lengths differ)']
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    e.close()


if __name__ == '__main__':
    main()
