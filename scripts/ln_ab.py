#!/usr/bin/env python3
"""The layer-norm greedy decode (csrc/decode_ln_kernels.hip) timed on one GPU at P = 512, B = 128, V1 = 9488, F = 2048,
beside the wide path (csrc/decode_wide_kernels.hip) at the same widths in the same process:

  (E, R) = (128, 128)   wide (test hook NICNES_DECODE_WIDE=1) | layer_n | layer_n + affine
  (E, R) = (256, 256)   wide                                  | layer_n | layer_n + affine

The baseline of every ratio is the wide path, the structure the LN kernel is built on: the same grid, wave roles, tile
staging, logit phase and token rule, without a normalisation. What the LN side adds per cell: the 10 R / 128
pre-activation windows written and read back twice (the centred second pass, the fold), the c' and sigmoid(o) windows of
phase (d), and the elementwise passes themselves (two IEEE divisions per gate pre-activation, one per unit of c'; with
affine eight more 16-byte loads per 16 values). The run does not separate the scratch traffic from the elementwise
work. The models differ (a layer_n model is not the wide model with something switched on), so captions and their
lengths differ between the sides; steps_run records how many decode steps each side's longest caption took.

One Engine.evaluate of the 512 members per pass (decode + CIDEr-D), timed with HIP events on the stream after a warm-up
of every side, interleaved, `--runs` rounds of `--reps` passes; medians with min - max. Scratch bytes per launch are
computed from the kernels' window maps: a wave holds (3 R + E) / 128 windows (wide) or (14 R + E) / 128 (LN) of 16 KiB
plus 256 bytes, eight waves per workgroup, one workgroup per member and 128-row slab. There is no threshold: the numbers
are only recorded.

  python scripts/ln_ab.py --out profiles/ln_ab.json"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'nes-img-captioning_amd'))
SIDES = (
    # name, E, R, layer_n, affine, environment read at create
    ('wide_128', 128, 128, False, False, {'NICNES_DECODE_WIDE': '1'}),
    ('ln_128', 128, 128, True, False, {}),
    ('ln_128_affine', 128, 128, True, True, {}),
    ('wide_256', 256, 256, False, False, {}),
    ('ln_256', 256, 256, True, False, {}),
    ('ln_256_affine', 256, 256, True, True, {}),
)


def scratch_bytes(E, R, ln, workgroups):
    windows = (14 if ln else 3) * (R // 128) + E // 128
    return workgroups * 8 * (windows * 16384 + 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=512)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--noise_len', type=int, default=1 << 25)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'ln_ab.json'))
    a = ap.parse_args()
    import torch
    import nicnes
    import nicnes.synthetic as S
    if not torch.cuda.is_available():
        sys.exit('ln_ab: needs a GPU (a timing on anything else says nothing)')
    P, B, SIGMA = a.members, a.batch, 0.01
    noise = S.noise_table(a.noise_len)
    engines, info = {}, {}
    for name, E, R, ln, aff, env in SIDES:
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            e = nicnes.Engine(input_encoding_size=E, rnn_size=R, max_batch=B, max_members=P, noise_len=a.noise_len,
                              layer_n=ln, layer_n_affine=aff)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        S.setup_engine_workload(e, B=B, noise=noise)
        engines[name] = e
        path = e.decode_path(B, P)
        assert path == ('ln' if ln else 'wide'), (name, path)
        info[name] = {'E': E, 'R': R, 'layer_n': ln, 'layer_n_affine': aff, 'D': e.D, 'decode_path': path, 'env': env,
                      'scratch_bytes_per_launch': scratch_bytes(E, R, ln, P * ((B + 127) // 128))}

    def timed(e, it):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for r in range(a.reps):
            e.evaluate(it + r, 0, P, SIGMA)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / a.reps

    for name, e in engines.items():                 # warm-up of every side; the length of its longest caption
        e.evaluate(1, 0, P, SIGMA)
        _, seq = e.evaluate(2, 0, 8, SIGMA, return_seq=True)
        seq = seq.cpu().numpy()
        T = seq.shape[-1]
        ends = np.where((seq == 0).any(-1), (seq == 0).argmax(-1) + 1, T)
        info[name]['steps_run_first_8_members'] = [int(x) for x in ends.reshape(8, -1).max(1)]
    torch.cuda.synchronize()
    ms = {k: [] for k in engines}
    for run in range(a.runs):                       # interleaved rounds
        for name, e in engines.items():
            ms[name].append(timed(e, 10 + 10 * run))
    res = {'members': P, 'batch': B, 'runs': a.runs, 'reps_per_run': a.reps, 'device': torch.cuda.get_device_name(0),
           'sides': {}}
    for name in engines:
        med = float(np.median(ms[name]))
        st = engines[name].stats()
        res['sides'][name] = dict(info[name], ms=ms[name], median_ms=med, min_ms=float(min(ms[name])),
                                  max_ms=float(max(ms[name])), members_per_s=P / (med * 1e-3),
                                  tie_fallbacks=int(st['tie_fallbacks']))
    s = res['sides']
    for w in ('128', '256'):
        base = s['wide_' + w]['median_ms']
        res['ln_%s_over_wide' % w] = s['ln_' + w]['median_ms'] / base
        res['ln_%s_affine_over_wide' % w] = s['ln_%s_affine' % w]['median_ms'] / base
        res['ln_%s_affine_over_ln' % w] = s['ln_%s_affine' % w]['median_ms'] / s['ln_' + w]['median_ms']
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    for e in engines.values():
        e.close()


if __name__ == '__main__':
    main()
