#!/usr/bin/env python3
"""What a nic_es generation costs on one MI355X next to a nic_nes evaluate of the same size.

    python scripts/es_generation_ab.py --out profiles/es_generation_ab.json

Default dims, B = 256, 500 pairs over 50 parents (47 + 3 elites, distinct theta). Timed with device events around each
call, every variant warmed up first, then `--runs` rounds that run every variant once each, in turn (so drift and other
tenants hit them alike); the median and the spread (min, max) of each variant are reported.

  a   Engine.evaluate of 500 members on ONE shared theta (the nic_nes kernels), screened and fp32
  b   Engine.es_evaluate, parents sorted across the pair ids (draw_parents), plain / proportional x screened / fp32
  c   the same with sort_parents=False
  d   es_select + es_advance (47 survivors behind 3 elite rows), with the bytes it moves
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, 'nes-img-captioning_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HBM_COPY_CEILING = 6.29e12      # bytes/s, float4 copy on the MI355X (79 % of the 8.0 TB/s spec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'es_generation_ab.json'))
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--pairs', type=int, default=500)
    ap.add_argument('--parents', type=int, default=50)
    ap.add_argument('--elites', type=int, default=3)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--noise-len', type=int, default=1 << 27)
    ap.add_argument('--theta-gain', type=float, default=1.0,
                    help="xavier gain of the parents (1.0: the benchmark's theta; 4.0 gives peaked logits, on which the "
                         'adaptive lse policy leaves the bounded lse and with it the screened loop)')
    ap.add_argument('--lse', choices=('bounded', 'adaptive'), default='bounded',
                    help="'bounded' pins the pair-bounded lse (NICNES_BOUNDED_LSE=1) so that the screened variants screen "
                         "in every round; 'adaptive' is the engine's default policy, which sums the exp exactly for the "
                         'next 32 decodes (and so does not screen) after a bounded decode needed exact passes')
    a = ap.parse_args()
    if a.lse == 'bounded':
        os.environ['NICNES_BOUNDED_LSE'] = '1'
    import torch
    import nicnes
    import nicnes.synthetic as S
    from nicnes.es import draw_parents
    from oracle import oracle as O
    if not torch.cuda.is_available():
        sys.exit('es_generation_ab.py measures on the GPU: none found')
    P, NP, NE, B = a.pairs, a.parents, a.elites, a.batch
    SIGMA, SEED = 0.005, 1
    dims = O.Dims()
    e = nicnes.Engine(max_batch=B, max_members=P, noise_len=a.noise_len, noise_seed=SEED)
    table = torch.randn(a.noise_len, dtype=torch.float32, device=e.device, generator=torch.Generator(e.device).manual_seed(5))
    e.set_noise_table(table)
    thetas = [O.make_theta(dims, 100 + i, a.theta_gain, 0.0) for i in range(NP)]
    fc = np.random.Generator(np.random.PCG64(9)).standard_normal((B, dims.F)).astype(np.float32)
    base, _, _ = O.decode(dims, thetas[0], fc)
    gts, df, n = S.build_references(base, dims.vocab_size, seed=3, n_refs=5, df_sets=512)
    keys, vals = nicnes.df_table_arrays(df)
    e.set_df_table(keys, vals, np.log(float(n)))
    e.set_batch(fc, gts)
    e.set_theta(thetas[0])
    e.es_create(NP, NE)
    e.es_set_parents(thetas)
    for i in range(NE):
        e.es_set_elite(i, i)
    fit = torch.empty((P, 2), dtype=torch.float64, device=e.device)
    po = {True: draw_parents(SEED, 1, P, NP, sort_parents=True), False: draw_parents(SEED, 1, P, NP, sort_parents=False)}
    n_keep = NP - NE

    def nes(screen):
        def run():
            e.set_decode_screen(screen)
            e.evaluate(1, 0, P, SIGMA, fitness_out=fit)
        return run

    def es(mode, screen, sort):
        def run():
            e.es_set_mutation(mode)
            e.set_decode_screen(screen)
            e.es_evaluate(1, 0, P, SIGMA, po[sort], fitness_out=fit)
        return run

    def advance():
        e.es_set_mutation('scale')
        order = e.es_select(fit, n_keep)
        e.es_advance(1, SIGMA, po[True], order, NE)

    variants = {'a_nes_screened': nes(True), 'a_nes_fp32': nes(False)}
    for mode in ('plain', 'scale'):
        for screen in (True, False):
            for sort in (True, False):
                name = '%s_es_%s_%s' % ('b' if sort else 'c', 'proportional' if mode == 'scale' else 'plain',
                                         'screened' if screen else 'fp32')
                variants[name] = es(mode, screen, sort)
    variants['d_select_advance'] = advance             # last in a round: it replaces the parents

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    for fn in variants.values():                       # warm-up: code objects, the first-use allocations
        timed(fn)
    ms = {k: [] for k in variants}
    path = {k: [] for k in variants}
    for _ in range(a.runs):
        for k, fn in variants.items():
            before = e.stats()['screen_candidates']    # (synchronising, outside the timed window)
            ms[k].append(timed(fn))
            # which loop this decode ran: the screened one only under the bounded lse, and it leaves candidates
            path[k].append(bool(e.stats()['screen_candidates'] > before))
    assert not np.isnan(fit.cpu().numpy()).any()
    D = dims.D
    d_bytes = 4 * D * (3 * n_keep + 2 * NE + (n_keep + NE))      # survivors: theta_p + z read, row written; elites
    res = {'device': torch.cuda.get_device_name(e.device), 'pairs': P, 'offspring': 2 * P, 'parents': NP, 'elites': NE,
           'batch': B, 'sigma': SIGMA, 'runs': a.runs, 'timing': 'device events around each call, interleaved rounds',
           'theta_gain': a.theta_gain, 'parent_table_bytes': 4 * NP * ((D + 63) // 64 * 64), 'lse': a.lse, 'screened_rounds': path,
           'ms': {}}
    for k, v in ms.items():
        med = float(np.median(v))
        res['ms'][k] = {'median': med, 'min': float(min(v)), 'max': float(max(v)), 'all': [float(x) for x in v],
                        'offspring_per_s': None if k.startswith('d') else 2 * P / (med * 1e-3)}
    m = {k: res['ms'][k]['median'] for k in ms}
    res['ratios'] = {}
    for tail, nes_k in (('plain_screened', 'a_nes_screened'), ('plain_fp32', 'a_nes_fp32'),
                        ('proportional_screened', 'a_nes_screened'), ('proportional_fp32', 'a_nes_fp32')):
        res['ratios']['b_over_a_' + tail] = m['b_es_' + tail] / m[nes_k]
        res['ratios']['b_over_c_' + tail] = m['b_es_' + tail] / m['c_es_' + tail]
    res['d'] = {'bytes': d_bytes, 'effective_bytes_per_s': d_bytes / (m['d_select_advance'] * 1e-3),
                'float4_copy_ceiling_bytes_per_s': HBM_COPY_CEILING,
                'share_of_ceiling': d_bytes / (m['d_select_advance'] * 1e-3) / HBM_COPY_CEILING,
                'note': 'survivor rows read theta_p and the noise slice and write the row, elite rows are copied, then '
                        'the statistics pass reads every new row; the select kernels are included in the time'}
    e.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps({'ms_median': m, 'ratios': res['ratios'], 'd': res['d']}, indent=1))


if __name__ == '__main__':
    main()
