#!/usr/bin/env python3
"""A/B of one validation pass over N = 5120 images (40 x 128) at the default dims, on one GPU:

  split   Split.evaluate(): every slab of the split decoded in one enqueue + the metrics kernels
  loop    the same images as 40 batches held by set_batches, one evaluate_theta call each (decode + CIDEr-D
          fitness of a batch): only calls the engine had before resident splits existed

Both are timed with HIP events on the stream after a warm-up of every shape, interleaved, `--runs` times each; a run
repeats its side `--reps` times so the timed window is not a few milliseconds. The tokens of the two sides are compared
first. Writes both medians, the loop's run-to-run spread and the ratio as JSON (--out).

  python scripts/val_split_ab.py --out profiles/val_split_ab.json
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'nes-img-captioning_amd'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5120)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'val_split_ab.json'))
    a = ap.parse_args()
    import torch
    import nicnes
    import nicnes.synthetic as S
    from nicnes.validation import corpus_df
    if not torch.cuda.is_available():
        sys.exit('val_split_ab: needs a GPU (a timing on anything else says nothing)')
    B = 128
    if a.images % B:
        sys.exit('--images must be a multiple of 128 (the loop side decodes whole batches)')
    nb = a.images // B
    noise_len = 1 << 23
    e = nicnes.Engine(max_batch=B, max_refs=5 * a.images, max_members=4, noise_len=noise_len)
    dims = S.Dims()
    e.set_noise_table(S.noise_table(noise_len))
    e.set_theta(S.init_theta(dims, 0, 4.0, 0.1))
    fc = S.fc_feats(a.images, dims.F)
    rng = np.random.Generator(np.random.PCG64(7))
    gts = []
    for _ in range(a.images):                       # 5 references of 8..15 words per image
        g = np.zeros((5, 16), np.int32)
        for j in range(5):
            L = int(rng.integers(8, 16))
            g[j, :L] = rng.integers(1, dims.vocab_size + 1, L)
        gts.append(g)
    keys, vals = corpus_df(gts)
    e.set_df_table(keys, vals, np.log(float(a.images)))
    e.set_batches([(fc[b * B:(b + 1) * B], gts[b * B:(b + 1) * B]) for b in range(nb)])
    split = e.make_split(fc, gts, df=(keys, vals), ref_len_raw=a.images)

    def run_split():
        return split.evaluate()

    def run_loop():
        return [e.evaluate_theta(b) for b in range(nb)]

    # same results first: the tokens of both sides
    loop_seq = torch.cat([e.evaluate_theta(b, return_seq=True)[1] for b in range(nb)])
    same = bool(torch.equal(loop_seq, split.decode()))

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.reps):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / a.reps

    for _ in range(2):                              # warm-up of every shape the timed windows use
        run_split()
        run_loop()
    torch.cuda.synchronize()
    ms = {'split': [], 'loop': []}
    for _ in range(a.runs):
        ms['loop'].append(timed(run_loop))
        ms['split'].append(timed(run_split))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = float(max(ms['loop']) - min(ms['loop']))
    res = {'images': a.images, 'runs': a.runs, 'reps_per_run': a.reps, 'device': torch.cuda.get_device_name(0),
           'tokens_equal': same, 'split_ms': ms['split'], 'loop_ms': ms['loop'], 'split_median_ms': med['split'],
           'loop_median_ms': med['loop'], 'loop_spread_ms': spread,
           'split_spread_ms': float(max(ms['split']) - min(ms['split'])),
           'ratio_loop_over_split': med['loop'] / med['split'],
           'faster_by_more_than_the_loop_spread': bool(med['loop'] - med['split'] > spread),
           'metrics': run_split(), 'decode_path_split': e.decode_path(128, (a.images + 255) // 256),
           'decode_path_loop': e.decode_path(64, 1)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    split.close()
    e.close()


if __name__ == '__main__':
    main()
