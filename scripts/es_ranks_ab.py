#!/usr/bin/env python3
"""What a rank's share of a nic_es generation costs on one MI355X, on the fused and on the coop decode path.

    python scripts/es_ranks_ab.py --out profiles/es_ranks_ab.json

Default dims, B = 256, 50 parents (distinct theta), and the 2-, 4- and 8-GPU shares of mscoco_es.json's 500 pairs: 250,
125 and 63 pairs. Timed with device events around each call, every variant warmed up first, then `--runs` rounds that run
every variant once each, in turn (so drift and other tenants hit them alike); medians with min and max.

  a   Engine.es_evaluate on the fused path (es_set_decode('fused'): the kernels every earlier build ran)
  b   Engine.es_evaluate on the coop path, ('coop', S) for S = 2 and 4 where the grid fits the GPU at once
  c   Engine.evaluate of the same count on ONE shared theta under its own shape rule (the nic_nes yardstick)

for plain and SM-PROPORTIONAL mutations (c: plain). With two or more GPUs it also records the wall time of whole
generations through `python -m nicnes.es` at W = 1, 2, 4, ... ranks over RCCL; with one it says that this is unmeasured.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, 'nes-img-captioning_amd')
for _p in (REPO, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

ES_EXP = {
    'algorithm': 'nic_es', 'dataset': 'mscoco', 'nb_offspring': 1000, 'population_size': 50, 'num_elites': 3,
    'num_elite_cands': 2, 'selection': 'uniform',
    'config': {'noise_stdev': 0.005, 'batch_size': 256, 'patience': 0, 'snapshot_freq': 0, 'num_val_items': 0},
    'policy_options': {'net': 'fc_caption', 'fitness': 'greedy', 'model_options': {'safe_mutations': 'SM-PROPORTIONAL'}},
}


def generation_wall_times(n_gpu, generations):
    """Rank 0's per-generation wall time of the CLI at W = 1, 2, 4, ... <= n_gpu ranks over RCCL (fresh processes)."""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        exp = os.path.join(d, 'es.json')
        with open(exp, 'w') as f:
            json.dump(ES_EXP, f)
        W = 1
        while W <= n_gpu:
            procs = []
            for r in range(W):
                env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(W), MASTER_ADDR='127.0.0.1',
                           MASTER_PORT='29517', PYTHONPATH=PKG + os.pathsep + os.environ.get('PYTHONPATH', ''))
                procs.append(subprocess.Popen(['timeout', '-k', '10', '600', sys.executable, '-m', 'nicnes.es', exp,
                                               '--synthetic', '--generations', str(generations), '--backend', 'nccl'],
                                              env=env, cwd=REPO, stdout=subprocess.PIPE, text=True))
            outs = [p.communicate()[0] for p in procs]
            if any(p.returncode for p in procs):
                out[str(W)] = {'error': 'exit statuses %s' % [p.returncode for p in procs]}
                break                                   # nothing further is started after a failed world
            out[str(W)] = json.loads(outs[0].strip().splitlines()[-1])
            W *= 2
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'es_ranks_ab.json'))
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--counts', type=int, nargs='+', default=[250, 125, 63])
    ap.add_argument('--parents', type=int, default=50)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--noise-len', type=int, default=1 << 27)
    ap.add_argument('--theta-gain', type=float, default=1.0)
    ap.add_argument('--lse', choices=('bounded', 'adaptive'), default='bounded',
                    help="'bounded' pins the pair-bounded lse (NICNES_BOUNDED_LSE=1), as scripts/es_generation_ab.py does")
    ap.add_argument('--generations', type=int, default=4, help='generations of the multi-GPU wall-time runs')
    a = ap.parse_args()
    if a.lse == 'bounded':
        os.environ['NICNES_BOUNDED_LSE'] = '1'
    import torch
    import nicnes
    import nicnes.synthetic as S
    from nicnes.es import draw_parents
    if not torch.cuda.is_available():
        sys.exit('es_ranks_ab.py measures on the GPU: none found')
    NP, B, PMAX = a.parents, a.batch, max(a.counts)
    SIGMA, SEED = 0.005, 1
    e = nicnes.Engine(max_batch=B, max_members=PMAX, noise_len=a.noise_len, noise_seed=SEED)
    dims = S.Dims()
    table = torch.randn(a.noise_len, dtype=torch.float32, device=e.device, generator=torch.Generator(e.device).manual_seed(5))
    e.set_noise_table(table)
    thetas = [S.init_theta(dims, 100 + i, a.theta_gain) for i in range(NP)]
    fc = S.fc_feats(B, dims.F, 9)
    e.set_theta(thetas[0])
    sp = e.make_split(fc)
    base = sp.decode().cpu().numpy()                   # the references derive from parent 0's greedy captions
    sp.close()
    gts, df, n = S.build_references(base, dims.vocab_size, seed=3, n_refs=5, df_sets=512)
    keys, vals = nicnes.df_table_arrays(df)
    e.set_df_table(keys, vals, np.log(float(n)))
    e.set_batch(fc, gts)
    e.es_create(NP, 1)
    e.es_set_parents(thetas)
    fit = torch.empty((PMAX, 2), dtype=torch.float64, device=e.device)
    occ, socc = ctypes.c_int(), ctypes.c_int()
    assert e.L.nicnes_decode_occupancy(ctypes.byref(occ), ctypes.byref(socc)) == 0
    n_cu = torch.cuda.get_device_properties(e.device).multi_processor_count
    nslabs = (B + 127) // 128

    def es(mode, count, decode):
        po = draw_parents(SEED, 1, 500, NP)[:count]       # the first shard of the generation's sorted parents

        def run():
            e.es_set_mutation(mode)
            e.es_set_decode(*decode)
            e.es_evaluate(1, 0, count, SIGMA, po, fitness_out=fit[:count])
        return run

    def nes(count):
        def run():
            e.evaluate(1, 0, count, SIGMA, fitness_out=fit[:count])
        return run

    variants, info = {}, {}
    for count in a.counts:
        e.es_set_decode('auto')
        info[str(count)] = {'nes_path': e.decode_path(B, count), 'nes_shape_G_slabs_S': e.decode_shape(B, count),
                            'es_auto_path': e.es_decode_path(B, count), 'workgroups_fused': count * nslabs}
        variants['c_nes_%d' % count] = nes(count)
        for mode, tag in (('plain', 'plain'), ('scale', 'proportional')):
            variants['a_es_fused_%s_%d' % (tag, count)] = es(mode, count, ('fused',))
            for S_ in (2, 4):
                if count * nslabs * S_ <= occ.value * n_cu:
                    variants['b_es_coop%d_%s_%d' % (S_, tag, count)] = es(mode, count, ('coop', S_))

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
    for _ in range(a.runs):
        for k, fn in variants.items():
            ms[k].append(timed(fn))
    st = e.stats()
    assert st['coop_timeouts'] == 0 and not np.isnan(fit.cpu().numpy()).any()
    res = {'device': torch.cuda.get_device_name(e.device), 'compute_units': n_cu, 'coop_workgroups_per_cu': occ.value,
           'batch': B, 'parents': NP, 'sigma': SIGMA, 'runs': a.runs, 'lse': a.lse, 'theta_gain': a.theta_gain,
           'timing': 'device events around each call, interleaved rounds', 'shapes': info, 'ms': {}, 'ratios': {}}
    for k, v in ms.items():
        res['ms'][k] = {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v)),
                        'all': [float(x) for x in v]}
    m = {k: res['ms'][k]['median'] for k in ms}
    for count in a.counts:
        for tag in ('plain', 'proportional'):
            fa = 'a_es_fused_%s_%d' % (tag, count)
            for S_ in (2, 4):
                b = 'b_es_coop%d_%s_%d' % (S_, tag, count)
                if b in m:
                    spread = max(res['ms'][b]['max'] - res['ms'][b]['min'], res['ms'][fa]['max'] - res['ms'][fa]['min'])
                    res['ratios'][b] = {'b_over_a': m[b] / m[fa], 'b_over_c': m[b] / m['c_nes_%d' % count],
                                        'a_minus_b_ms': m[fa] - m[b], 'rounds_spread_ms': spread,
                                        'b_beats_a_beyond_spread': bool(m[fa] - m[b] > spread)}
    e.close()
    n_gpu = torch.cuda.device_count()
    if n_gpu >= 2:
        res['generation_wall_time'] = generation_wall_times(n_gpu, a.generations)
    else:
        res['generation_wall_time'] = ('unmeasured: this machine shows one GPU; only the per-share kernel times above stand '
                                       'behind multi-GPU scaling')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps({'ms_median': m, 'ratios': res['ratios'], 'shapes': info}, indent=1))


if __name__ == '__main__':
    main()
