#!/usr/bin/env python3
"""Compare the gfx950 machine code of two builds of libnicnes.so kernel by kernel.

    python scripts/isa_unchanged.py OLD.so NEW.so > profiles/es_isa_unchanged.txt

For every kernel of OLD it prints nicnes.codeobj.kernel_isa_sha256 in both libraries and SAME / MOVED / GONE, then the
kernels only NEW has. Exit status 1 when a kernel of OLD moved or is gone. (A change that adds kernels, such as the
nic_es entries, must leave every committed profile's kernel as it was.)"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'nes-img-captioning_amd'))
from nicnes import codeobj  # noqa: E402


def main(old_so, new_so):
    old, new = codeobj.kernel_listings(old_so), codeobj.kernel_listings(new_so)
    bad = 0
    print('# kernel_isa_sha256 of every kernel of the parent build, in the parent build and in this tree')
    for sym in sorted(old):
        a = codeobj.kernel_isa_sha256(old_so, sym, old)
        b = codeobj.kernel_isa_sha256(new_so, sym, new)
        state = 'SAME' if a == b else ('GONE' if b is None else 'MOVED')
        bad += state != 'SAME'
        print('%s %s %s %s' % (state, a[:16], (b or '-')[:16], sym))
    for sym in sorted(set(new) - set(old)):
        print('NEW  %s %s %s' % ('-' * 16, codeobj.kernel_isa_sha256(new_so, sym, new)[:16], sym))
    print('# %d kernels of the parent build, %d moved or gone, %d new' % (len(old), bad, len(set(new) - set(old))))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
