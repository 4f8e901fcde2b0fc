"""Workgroup spans of the screened decode's launch on the flagship shape (pop 512, B 128), from DECODE_PROF=2 builds
(two marks per workgroup: start and end s_memrealtime with HW_REG_XCC_ID / HW_REG_HW_ID; wrong tokens, never the product):

    make -C nes-img-captioning_amd ablate        (its prof2 and prof2r variants: libnicnes_prof2.so, libnicnes_prof2r.so)
    python scripts/step_queue_spans.py nes-img-captioning_amd/build/ablate OUT.json

Per launch (the one-launch kernel in grid order, the same with the members in reverse grid order): the launch span, the
per-CU busy sums, the idle share 1 - mean(busy) / span, and how much of the spread of the workgroup times follows the
member (correlation of a member's time in grid order with its time in reverse order, where it runs on another CU at
another time) and how much the CU (correlation of a CU's mean workgroup time between the two runs) or the XCD (per-XCD
means). Third of three bench-like iterations, as scripts/ablate.py."""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'nes-img-captioning_amd'))
import nicnes  # noqa: E402
import nicnes.synthetic as S  # noqa: E402

POP, B = 512, 128


def marks(seq):
    raw = seq.reshape(-1, 4096).cpu().numpy().astype(np.int64) & 0xffffffff
    on = raw[:, 0] != 0                                        # (rows of workgroups that ran)
    st, en, hw = raw[:, 0], raw[:, 1], raw[:, 2048]
    cu = ((hw >> 16) << 8) | (hw & 0xff)                      # XCC id | SE, SH, CU of HW_ID
    return on, st, en, cu, hw >> 16


def iterate(e, n=3):
    gsum = torch.empty(e.D, dtype=torch.float32, device='cuda')
    seqs = []
    for q in range(n):                                         # bench-like iterations, nothing waits in between
        fit, seq = e.evaluate(50 + q, 0, POP, 0.01, return_seq=True)
        _, w = e.rank_weights(fit)
        e.grad_partial(50 + q, 0, POP, w, 0.01, out=gsum)
        e.adam_step(gsum, POP, 1e-7, 1e-6, sync=False)
        seqs.append(seq)
    torch.cuda.synchronize()
    return seqs[-1]


def summary(seq, reverse=False):
    on, st, en, cu, xcc = marks(seq)
    t0 = st[on].min()
    s = ((st - t0) % (1 << 32)) / 100.0                        # us (100 MHz)
    d = ((en - st) % (1 << 32)) / 100.0
    span = float((s + d)[on].max())
    busy = {}
    for c, v in zip(cu[on], d[on]):
        busy[int(c)] = busy.get(int(c), 0.0) + float(v)
    b = np.array(sorted(busy.values()))
    out = {'workgroups': int(on.sum()), 'cus': len(busy), 'span_us': round(span, 1),
           'cu_busy_mean_us': round(float(b.mean()), 1), 'cu_busy_min_us': round(float(b.min()), 1),
           'cu_busy_max_us': round(float(b.max()), 1), 'idle_share': round(1.0 - float(b.mean()) / span, 4),
           'wg_us': {'mean': round(float(d[on].mean()), 1), 'median': round(float(np.median(d[on])), 1),
                     'min': round(float(d[on].min()), 1), 'max': round(float(d[on].max()), 1)},
           'wgs_per_cu': {str(k): int(v) for k, v in zip(*np.unique(np.unique(cu[on], return_counts=True)[1],
                                                                     return_counts=True))},
           'xcd_wg_mean_us': {str(int(x)): round(float(d[on & (xcc == x)].mean()), 1) for x in np.unique(xcc[on])},
           'cu_busy_us': [round(float(v), 1) for v in b]}
    idx = np.arange(d.size)
    member = (d.size - 1 - idx) if reverse else idx
    by_member = np.zeros(d.size)
    by_member[member] = d
    cu_mean = {int(c): float(d[on & (cu == c)].mean()) for c in np.unique(cu[on])}
    start = np.zeros(d.size)
    start[member] = s
    return out, by_member, cu_mean, start


def main(adir, out_path):
    noise = torch.from_numpy(S.noise_table(1 << 27)).cuda()
    res, keep = {}, {}
    e = nicnes.Engine(max_batch=B, max_members=POP, noise_len=1 << 27)     # the product: it makes the references
    try:
        wl = S.setup_engine_workload(e, B=B, noise=noise)
        keys, vals = nicnes.df_table_arrays(wl['df'])
    finally:
        e.close()
    # (queue off in both: the DECODE_PROF=2 build of the queue kernel is no measure of it, its sweep loop spills:
    # scripts/isa_loop_spills.py counts 7 scratch loads and 2 stores there, none in the product's)
    for name, lib, queue in (('one_launch', 'prof2', False), ('one_launch_reversed', 'prof2r', False)):
        e = nicnes.Engine(max_batch=B, max_members=POP, noise_len=1 << 27,
                          lib_path=os.path.join(adir, 'libnicnes_%s.so' % lib))
        try:
            e.set_noise_table(noise)                           # (timing-only builds decode garbage: the product's refs)
            e.set_theta(wl['theta32'])
            e.set_df_table(keys, vals, np.log(float(wl['ref_len_raw'])))
            e.set_batch(wl['fc'], wl['gts'])
            e.set_decode_queue(queue)
            r, by_member, cu_mean, start = summary(iterate(e), reverse=name.endswith('reversed'))
            assert e.stats()['queue_timeouts'] == 0
            res[name] = r
            keep[name] = (by_member, cu_mean, start)
        finally:
            e.close()
    a, b = keep['one_launch'], keep['one_launch_reversed']
    cus = sorted(set(a[1]) & set(b[1]))
    first_a, first_b = a[2] < 1000.0, b[2] < 1000.0            # the members a run started in its first round
    res['spread'] = {
        'member_corr_grid_vs_reversed': round(float(np.corrcoef(a[0], b[0])[0, 1]), 3),
        'cu_corr_grid_vs_reversed': round(float(np.corrcoef([a[1][c] for c in cus], [b[1][c] for c in cus])[0, 1]), 3),
        'wg_us_first_round_mean': round(float(a[0][first_a].mean()), 1),
        'wg_us_second_round_mean': round(float(a[0][~first_a].mean()), 1),
        'reversed_wg_us_first_round_mean': round(float(b[0][first_b].mean()), 1),
        'reversed_wg_us_second_round_mean': round(float(b[0][~first_b].mean()), 1),
        'wg_us_std': round(float(a[0].std()), 1),
    }
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk != 'cu_busy_us'} for k, v in res.items()}, indent=1))


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
