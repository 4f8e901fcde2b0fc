#!/usr/bin/env python3
"""What SM-G-SUM costs a nic_es generation on one MI355X, beside SM-PROPORTIONAL in the same process.

    python scripts/es_safe_ab.py --out profiles/es_safe_ab.json

scripts/es_generation_ab.py's protocol and shape (mscoco_es.json's): default dims, B = 256, 500 pairs over 50 parents (47
+ 3 elites, distinct theta), device events around each call, every variant warmed up first, then `--runs` rounds that run
every variant once each, in turn; medians with min and max. The pair-bounded lse is pinned so the screened variants screen.

  a   Engine.es_sensitivity of all 50 parents on 256 rows (one pass per parent, in a row, on one stream)
  b   the mutate launch: an evaluate's device time minus its decode and CIDEr kernels (Engine.kernel_times), which
      leaves the delta' rows' launch, the noise indices and the parent_of copy; divide and SM-PROPORTIONAL
  c   Engine.es_evaluate, divide and SM-PROPORTIONAL x screened / fp32
  d   es_select + es_advance (47 survivors behind 3 elite rows), divide and SM-PROPORTIONAL
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'es_safe_ab.json'))
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--pairs', type=int, default=500)
    ap.add_argument('--parents', type=int, default=50)
    ap.add_argument('--elites', type=int, default=3)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--rows', type=int, default=256, help='rows of the sensitivity pass (min(B, batch_size))')
    ap.add_argument('--underflow', type=float, default=1e-3)
    ap.add_argument('--noise-len', type=int, default=1 << 27)
    a = ap.parse_args()
    os.environ['NICNES_BOUNDED_LSE'] = '1'
    import torch
    import nicnes
    import nicnes.synthetic as S
    from nicnes.es import draw_parents
    from oracle import oracle as O
    if not torch.cuda.is_available():
        sys.exit('es_safe_ab.py measures on the GPU: none found')
    P, NP, NE, B = a.pairs, a.parents, a.elites, a.batch
    SIGMA, SEED = 0.005, 1
    dims = O.Dims()
    e = nicnes.Engine(max_batch=B, max_members=P, noise_len=a.noise_len, noise_seed=SEED)
    table = torch.randn(a.noise_len, dtype=torch.float32, device=e.device, generator=torch.Generator(e.device).manual_seed(5))
    e.set_noise_table(table)
    thetas = [O.make_theta(dims, 100 + i, 1.0, 0.0) for i in range(NP)]
    fc = np.random.Generator(np.random.PCG64(9)).standard_normal((B, dims.F)).astype(np.float32)
    base, _, _ = O.decode(dims, thetas[0], fc)
    gts, df, n = S.build_references(base, dims.vocab_size, seed=3, n_refs=5, df_sets=512)
    keys, vals = nicnes.df_table_arrays(df)
    e.set_df_table(keys, vals, np.log(float(n)))
    e.set_batch(fc, gts)
    e.es_create(NP, NE)
    e.es_set_parents(thetas)
    for i in range(NE):
        e.es_set_elite(i, i)
    e.set_timing(True)                                 # (three events per evaluate, in every variant alike)
    fit = torch.empty((P, 2), dtype=torch.float64, device=e.device)
    po = draw_parents(SEED, 1, P, NP, sort_parents=True)
    distinct = sorted(set(int(p) for p in po))
    n_keep = NP - NE

    def set_mode(mode):
        if mode == 'divide':
            e.es_set_mutation_divide()
        else:
            e.es_set_mutation(mode)

    def sensitivity():
        e.es_sensitivity(list(range(NP)), a.rows, a.underflow)

    def es(mode, screen):
        def run():
            set_mode(mode)
            e.set_decode_screen(screen)
            e.es_evaluate(1, 0, P, SIGMA, po, fitness_out=fit)
        return run

    def advance(mode):
        def run():
            set_mode(mode)
            order = e.es_select(fit, n_keep)
            e.es_advance(1, SIGMA, po, order, NE)
        return run

    # the order of a round: the sensitivities (valid until the first advance), the evaluates, then the two advances
    # (each replaces the parents; the divide one first, while its rows are valid)
    variants = {'a_sensitivity': sensitivity}
    for mode, name in (('divide', 'divide'), ('scale', 'proportional')):
        for screen in (True, False):
            variants['c_es_%s_%s' % (name, 'screened' if screen else 'fp32')] = es(mode, screen)
    variants['d_select_advance_divide'] = advance('divide')
    variants['d_select_advance_proportional'] = advance('scale')

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
    mutate = {'b_mutate_divide': [], 'b_mutate_proportional': []}
    screened = {k: [] for k in variants if k.startswith('c_')}
    for _ in range(a.runs):
        for k, fn in variants.items():
            before = e.stats()['screen_candidates']    # (synchronising, outside the timed window)
            ms[k].append(timed(fn))
            if k.startswith('c_'):
                screened[k].append(bool(e.stats()['screen_candidates'] > before))
                if k.endswith('fp32'):
                    mutate['b_mutate_' + k.split('_')[2]].append(ms[k][-1] - sum(e.kernel_times()))
    assert not np.isnan(fit.cpu().numpy()).any()
    s0 = None
    e.es_sensitivity([0], a.rows, a.underflow)
    s0 = e.es_sensitivity_row(0).cpu().numpy()

    def stat(v):
        return {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v)), 'all': [float(x) for x in v]}
    res = {'device': torch.cuda.get_device_name(e.device), 'pairs': P, 'offspring': 2 * P, 'parents': NP, 'elites': NE,
           'batch': B, 'sensitivity_rows': a.rows, 'underflow': a.underflow, 'distinct_parents_drawn': len(distinct),
           'sigma': SIGMA, 'runs': a.runs, 'timing': 'device events around each call, interleaved rounds', 'lse': 'bounded',
           'screened_rounds': screened, 'sensitivity_table_bytes': 4 * NP * ((dims.D + 63) // 64 * 64),
           'sensitivity_row0': {'share_above_1': float((s0 > 1).mean()), 'max': float(s0.max())},
           'ms': {k: stat(v) for k, v in list(ms.items()) + list(mutate.items())}}
    m = {k: v['median'] for k, v in res['ms'].items()}
    res['ms_per_parent_sensitivity'] = m['a_sensitivity'] / NP
    res['ratios'] = {'sensitivity_over_evaluate_screened': m['a_sensitivity'] / m['c_es_divide_screened'],
                     'sensitivity_over_evaluate_fp32': m['a_sensitivity'] / m['c_es_divide_fp32'],
                     'divide_over_proportional_screened': m['c_es_divide_screened'] / m['c_es_proportional_screened'],
                     'divide_over_proportional_fp32': m['c_es_divide_fp32'] / m['c_es_proportional_fp32'],
                     'advance_divide_over_proportional': m['d_select_advance_divide'] / m['d_select_advance_proportional']}
    e.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps({'ms_median': m, 'ms_per_parent_sensitivity': res['ms_per_parent_sensitivity'],
                      'ratios': res['ratios']}, indent=1))


if __name__ == '__main__':
    main()
