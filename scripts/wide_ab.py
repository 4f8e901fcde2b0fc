#!/usr/bin/env python3
"""The wide greedy decode (csrc/decode_wide_kernels.hip) timed on one GPU at P = 512, B = 128, V1 = 9488, F = 2048:

  (a) E = R = 128   the wide path (test hook NICNES_DECODE_WIDE=1) beside the fused fp32 kernel in the same process:
                    fused with the exact exp-sum (NICNES_BOUNDED_LSE=0: the wide path's own lse rule) and fused as the
                    greedy-only product runs it unscreened (the pair-bounded lse); NICNES_SCREEN=0 for all three.
                    The difference is the price of the wide path's first structure as a whole: the B operand
                    streamed from lane scratch, 32-row tiles with a barrier per 64 MFMAs, no mid-tile store and no
                    prefetch across phases. The run does not separate these parts, so the ratio is not the cost of
                    streaming the B operand alone
  (b) (E, R) = (256, 256) and (512, 512): ms per evaluate, members/s and the algorithmic FLOP rate over the
                    157.3 TFLOP/s fp32 MFMA peak

One Engine.evaluate of the 512 members per pass (decode + CIDEr-D), timed with HIP events on the stream after a warm-up
of every side, interleaved, `--runs` rounds of `--reps` passes; medians with min - max. The FLOP count is SURVEY.md
8(d)'s, re-derived for the widths: per unique row and decode 2 [F E + (T + 1) 5 R (E + R) + T R V1] (the image
projection, T + 1 cells, T logit products; rows that end early do less, so the rate is an upper bound of the work
rate), times 2 signs x B rows per member. There is no threshold: the numbers are only recorded.

  python scripts/wide_ab.py --out profiles/wide_ab.json"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'nes-img-captioning_amd'))
PEAK_FP32_MFMA = 157.3e12
SIDES = (
    # name, E, R, environment read at create
    ('wide_128', 128, 128, {'NICNES_DECODE_WIDE': '1', 'NICNES_SCREEN': '0'}),
    ('fused_128_exact_lse', 128, 128, {'NICNES_SCREEN': '0', 'NICNES_BOUNDED_LSE': '0'}),
    ('fused_128_bounded_lse', 128, 128, {'NICNES_SCREEN': '0'}),
    ('wide_256', 256, 256, {}),
    ('wide_512', 512, 512, {}),
)


def flop_per_member(E, R, F, V1, T, B):
    return 2.0 * B * 2.0 * (F * E + (T + 1) * 5 * R * (E + R) + T * R * V1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--members', type=int, default=512)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--noise_len', type=int, default=1 << 25)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'wide_ab.json'))
    a = ap.parse_args()
    import torch
    import nicnes
    import nicnes.synthetic as S
    if not torch.cuda.is_available():
        sys.exit('wide_ab: needs a GPU (a timing on anything else says nothing)')
    P, B, SIGMA = a.members, a.batch, 0.01
    noise = S.noise_table(a.noise_len)
    engines, info = {}, {}
    for name, E, R, env in SIDES:
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            e = nicnes.Engine(input_encoding_size=E, rnn_size=R, max_batch=B, max_members=P, noise_len=a.noise_len)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        S.setup_engine_workload(e, B=B, noise=noise)
        engines[name] = e
        c = e.cfg
        info[name] = {'E': E, 'R': R, 'D': e.D, 'decode_path': e.decode_path(B, P), 'env': env,
                      'flop_per_member': flop_per_member(E, R, c.fc_feat_size, c.vocab_size + 1, c.seq_length, B)}

    def timed(e, it):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for r in range(a.reps):
            e.evaluate(it + r, 0, P, SIGMA)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / a.reps

    # the wide path at the default widths decodes the fused kernel's tokens (the bits, with the exact lse)
    _, s_w = engines['wide_128'].evaluate(1, 0, 8, SIGMA, return_seq=True)
    _, s_f = engines['fused_128_exact_lse'].evaluate(1, 0, 8, SIGMA, return_seq=True)
    same = bool(torch.equal(s_w, s_f))
    for name, e in engines.items():                 # warm-up of every side
        e.evaluate(1, 0, P, SIGMA)
        e.evaluate(2, 0, P, SIGMA)
        info[name]['bounded_lse'] = e.last_decode_bounded()
    torch.cuda.synchronize()
    ms = {k: [] for k in engines}
    for run in range(a.runs):                       # interleaved rounds
        for name, e in engines.items():
            ms[name].append(timed(e, 10 + 10 * run))
    res = {'members': P, 'batch': B, 'runs': a.runs, 'reps_per_run': a.reps, 'device': torch.cuda.get_device_name(0),
           'peak_fp32_mfma_flops': PEAK_FP32_MFMA, 'wide_128_tokens_equal_fused': same,
           'flop_formula': '2 signs x B x 2 [F E + (T + 1) 5 R (E + R) + T R V1] per member', 'sides': {}}
    for name in engines:
        med = float(np.median(ms[name]))
        st = engines[name].stats()
        res['sides'][name] = dict(info[name], ms=ms[name], median_ms=med, min_ms=float(min(ms[name])),
                                  max_ms=float(max(ms[name])), members_per_s=P / (med * 1e-3),
                                  flop_rate_over_peak=P * info[name]['flop_per_member'] / (med * 1e-3) / PEAK_FP32_MFMA,
                                  tie_fallbacks=int(st['tie_fallbacks']))
    s = res['sides']
    res['wide_128_over_fused_exact_lse'] = s['wide_128']['median_ms'] / s['fused_128_exact_lse']['median_ms']
    res['wide_128_over_fused_bounded_lse'] = s['wide_128']['median_ms'] / s['fused_128_bounded_lse']['median_ms']
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    for e in engines.values():
        e.close()


if __name__ == '__main__':
    main()
