"""Scratch (spill) traffic inside the loops of one kernel of a gfx950 assembly listing (dev tool).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -x hip --cuda-device-only -S \\
        nes-img-captioning_amd/csrc/decode_kernel.hip -o decode.s
    python scripts/isa_loop_spills.py decode.s _Z33nicnes_decode_steps_screen_kernel

For every backward branch of the kernel whose span (the blocks from the branch target to the branch) holds MFMAs and
is shorter than 60 blocks: the scratch loads and stores, the instructions and the bf16 / fp32 MFMAs in the span. The
screened kernel's sweep is the innermost loop with bf16 MFMAs; a reload in it costs every stage of every step."""
import re
import sys


def kernel_lines(path, prefix):
    on = False
    for line in open(path):
        if re.match(r'^%s\w*:' % re.escape(prefix), line):
            on = True
        if on:
            yield line
            if line.split(';')[0].strip() == 's_endpgm':
                return


def main(path, prefix):
    cur, order, br, cnt = None, [], {}, {}
    for line in kernel_lines(path, prefix):
        m = re.match(r'^(\.LBB\w+):', line)
        if m:
            cur = m.group(1)
            order.append(cur)
            br[cur], cnt[cur] = [], {'ld': 0, 'st': 0, 'n': 0, 'bf': 0, 'f32': 0}
            continue
        t = line.split(';')[0].strip()
        if cur is None or not t or t.startswith('.'):
            continue
        op = t.split()[0]
        c = cnt[cur]
        c['n'] += 1
        if op.startswith('s_cbranch') or op == 's_branch':
            br[cur].append(t.split()[-1])
        c['ld'] += op.startswith('scratch_load')
        c['st'] += op.startswith('scratch_store')
        if 'mfma' in op:
            c['bf16' in op and 'bf' or 'f32'] += 1
    idx = {b: i for i, b in enumerate(order)}
    seen = set()
    for i, b in enumerate(order):
        for t in br[b]:
            if t in idx and idx[t] <= i and (t, b) not in seen:
                seen.add((t, b))
                span = order[idx[t]: i + 1]
                tot = {k: sum(cnt[x][k] for x in span) for k in ('ld', 'st', 'n', 'bf', 'f32')}
                if tot['bf'] + tot['f32'] and len(span) < 60:
                    print('loop %s .. %s: scratch loads %d stores %d, %d instructions, MFMA bf16 %d fp32 %d'
                          % (t, b, tot['ld'], tot['st'], tot['n'], tot['bf'], tot['f32']))


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
