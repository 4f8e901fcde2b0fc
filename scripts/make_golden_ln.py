#!/usr/bin/env python3
"""tests/golden/decode_layernorm.npz: FCModel._sample of the imported reference with layer_n=True.

    python scripts/make_golden_ln.py

Needs the reference checkout (as scripts/make_golden.py, whose decode replay and theta loading it uses). Cases: V = 67
(V1 = 68), F = 128, B = 16, theta = oracle.make_theta(d, 0, 4.0, 0.1), at (E, R) = (128, 128) and (256, 256), each
without and with layer_n_affine. With affine the six layer-norm tensors follow the nine in the reference's
parameters() order (asserted here, stored as 'ln_names') and are gamma = 1 + 0.1 z, beta = 0.1 z in that order
(tests/ln_ref.py make_tail with the stored seed). Per case: theta itself (tokens, log-probs, per-step top-2 margins) and
two table-perturbed members of both signs (tokens, margins). theta and fc are regenerated from the stored seeds.
Keys are '<case>/<key>'. The smallest live-step margins are printed: re-seed a case whose members sit on a near-tie."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))

import make_golden as G  # noqa: E402  (sets the paths, imports the reference)
import ln_ref as L  # noqa: E402
from oracle import oracle as O  # noqa: E402

# (name, E, R, affine, fc seed, tail seed)
CASES = (('e128_r128', 128, 128, False, 1400, 0), ('e256_r256', 256, 256, False, 1400, 0),
         ('e128_r128_affine', 128, 128, True, 1400, 1410), ('e256_r256_affine', 256, 256, True, 1400, 1411))
NOISE_LEN, TABLE_SEED, NOISE_SEED, ITERATION, SIGMA, MEMBERS = 1 << 21, 123, 7, 3, 0.01, (0, 1)


def live(seq):
    """steps at which the row still decodes: the first, and every one after a non-zero token"""
    return np.concatenate([np.ones((len(seq), 1), bool), seq[:, :-1] > 0], 1)


def main():
    out = {'cases': np.array([c[0] for c in CASES]), 'ln_names': np.array(L.LN_NAMES)}
    for name, E, R, affine, fc_seed, tail_seed in CASES:
        d = O.Dims(vocab_size=67, E=E, R=R, F=128)
        opt = G.Opt(d.vocab_size, d.E, d.R, d.F, False, False, False, True, affine, '', 0.1, '')
        model = G.ref_nets.FCModel(options=opt)
        names = [n for n, _ in model.named_parameters()]
        assert names == [n for n, _ in d.shapes()] + (L.LN_NAMES if affine else []), names
        theta = O.make_theta(d, 0, 4.0, 0.1)
        if affine:
            theta = np.concatenate([theta, L.make_tail(R, tail_seed, 0.1)])
        D = theta.size
        assert D == sum(p.numel() for p in model.parameters())
        fc = np.random.Generator(np.random.PCG64(fc_seed)).standard_normal((16, d.F)).astype(np.float32)
        G.load_theta(model, theta)
        seq, slp, mar = G.ref_decode(model, fc)
        table = O.noise_table(NOISE_LEN, TABLE_SEED)
        pseq, pmar = [], []
        for m in MEMBERS:
            idx = O.noise_index(NOISE_SEED, ITERATION, m, NOISE_LEN, D)
            for sign in (+1, -1):
                G.load_theta(model, O.perturb(theta, table, idx, SIGMA, sign))
                s, _, mm = G.ref_decode(model, fc)
                pseq.append(s)
                pmar.append(mm)
        one = dict(dims=np.array([d.vocab_size, E, R, d.F, d.T], np.int64), affine=np.int64(affine),
                   theta_seed=np.int64(0), gain=np.float64(4.0), bias_std=np.float64(0.1), tail_seed=np.int64(tail_seed),
                   tail_scale=np.float64(0.1), fc_seed=np.int64(fc_seed), B=np.int64(16), D=np.int64(D),
                   seq=seq, logprobs=slp, margins=mar, noise_len=np.int64(NOISE_LEN), table_seed=np.int64(TABLE_SEED),
                   noise_seed=np.int64(NOISE_SEED), iteration=np.int64(ITERATION), sigma=np.float64(SIGMA),
                   members=np.array(MEMBERS, np.int64), member_seq=np.stack(pseq), member_margins=np.stack(pmar))
        out.update({'%s/%s' % (name, k): v for k, v in one.items()})
        lens = (seq > 0).sum(1) + 1
        print(name, 'D', D, 'steps', int(lens.min()), '-', int(min(lens.max(), d.T)), 'min live margin: theta',
              float(mar[live(seq)].min()), 'members', [float(m[live(s)].min()) for s, m in zip(pseq, pmar)])
    np.savez_compressed(os.path.join(G.OUT, 'decode_layernorm.npz'), **out)


if __name__ == '__main__':
    torch.set_num_threads(1)
    main()
