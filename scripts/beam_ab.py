#!/usr/bin/env python3
"""Beam-search decode against the greedy decode of a resident split, N = 5120 images at the default dims, on one GPU:

  beam K    Split.decode_beam(0, N, K) for K = 1, 3, 5: N x K hypothesis rows
  greedy    Split.decode of the same N images, and of K x N images (the same row count as beam K)

Every side is timed with HIP events on the stream after a warm-up of every shape, interleaved, `--runs` rounds of
`--reps` passes each; medians and the round-to-round spread are written as JSON (--out), with rows/s and the
algorithmic FLOP rate over the 157.3 TFLOP/s fp32 MFMA peak. The FLOP count is the full-length one (every row runs the
image step, the BOS step and seq_length steps of cell + logits; 2 FLOP per multiply-add): rows that stop early do less,
so the rate is an upper bound of the work rate. There is no threshold: the numbers are only recorded. The beam decode
is also timed in both of its workgroup shapes (4 and 8 waves) at N and 4 N images.

  python scripts/beam_ab.py --out profiles/beam_ab.json
  rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python3 scripts/beam_ab.py --runs 1 --reps 3 \
      --out DIR/ab.json          # the kernel statistics of profiles/beam_kernel_stats.csv, a run of its own
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'nes-img-captioning_amd'))
PEAK_FP32_MFMA = 157.3e12
BEAMS = (1, 3, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5120)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'beam_ab.json'))
    a = ap.parse_args()
    import torch
    import nicnes
    import nicnes.synthetic as S
    if not torch.cuda.is_available():
        sys.exit('beam_ab: needs a GPU (a timing on anything else says nothing)')
    N = a.images
    e = nicnes.Engine(max_batch=128, max_members=4, noise_len=1 << 23)
    dims = S.Dims()
    e.set_theta(S.init_theta(dims, 0, 4.0, 0.1))
    split = e.make_split(S.fc_feats(N * max(BEAMS), dims.F))      # decode-only: the beam rows' count of images
    T, V1, R, E, F = e.cfg.seq_length, e.cfg.vocab_size + 1, 128, 128, dims.F
    flop_row = 2.0 * (E * F + (T + 1) * (5 * R * (E + R)) + T * V1 * R)

    sides = {}
    for K in BEAMS:
        sides['beam_%d' % K] = (lambda K=K: split.decode_beam(0, N, K), N * K)
        sides['greedy_%dx' % K] = (lambda K=K: split.decode(0, N * K), N * K)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.reps):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / a.reps

    greedy = split.decode(0, N)
    beam1 = split.decode_beam(0, N, 1)
    same = float((greedy == beam1).all(1).float().mean())
    lengths = {k: float(((fn() != 0).sum(1).float().mean())) for k, (fn, _) in sides.items()}
    for _ in range(2):                              # warm-up of every shape the timed windows use
        for fn, _ in sides.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(a.runs):                         # interleaved rounds
        for k, (fn, _) in sides.items():
            ms[k].append(timed(fn))
    res = {'images': N, 'runs': a.runs, 'reps_per_run': a.reps, 'device': torch.cuda.get_device_name(0),
           'flop_per_row_full_length': flop_row, 'peak_fp32_mfma_flops': PEAK_FP32_MFMA,
           'beam_1_rows_equal_to_greedy': same, 'mean_caption_words': lengths, 'sides': {}}
    for k, (_, rows) in sides.items():
        med = float(np.median(ms[k]))
        res['sides'][k] = {'rows': rows, 'ms': ms[k], 'median_ms': med, 'spread_ms': float(max(ms[k]) - min(ms[k])),
                           'rows_per_s': rows / (med * 1e-3),
                           'flop_rate_over_peak': rows * flop_row / (med * 1e-3) / PEAK_FP32_MFMA}
    # the two workgroup shapes the launch chooses between (Engine.set_beam_waves), at N and 4 N images: what the rule
    # of nicnes_beam_waves_per_wg rests on. Medians of `runs` windows of 2 passes.
    res['shapes_ms'] = {}
    for n_img in (N, 4 * N):
        for K in BEAMS:
            for nw in (4, 8):
                e.set_beam_waves(nw)
                fn = lambda: split.decode_beam(0, n_img, K)      # noqa: E731
                fn()
                torch.cuda.synchronize()
                ts = []
                for _ in range(a.runs):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    fn()
                    fn()
                    t1.record()
                    t1.synchronize()
                    ts.append(t0.elapsed_time(t1) / 2)
                res['shapes_ms']['images_%d_K%d_waves_%d' % (n_img, K, nw)] = float(np.median(ts))
    e.set_beam_waves(0)
    for K in BEAMS:
        res['beam_%d_over_greedy_same_rows' % K] = (res['sides']['beam_%d' % K]['median_ms'] /
                                                    res['sides']['greedy_%dx' % K]['median_ms'])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    split.close()
    e.close()


if __name__ == '__main__':
    main()
