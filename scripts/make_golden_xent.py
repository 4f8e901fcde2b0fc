#!/usr/bin/env python3
"""tests/golden/xent.npz: teacher-forced log-probs of label rows under the imported reference's FCModel.

    python scripts/make_golden_xent.py

Needs the reference checkout (as scripts/make_golden.py, whose theta loading it uses). FCModel has only _sample, so the
forward is self-critical.pytorch's FCModel._forward driven over the reference's own modules: img_embed and core from a
zero state (logits discarded), then per step embed(u_s), core, logit, F.log_softmax(...).gather(target), with u_0 = 0
and u_s = w[s - 1]; LanguageModelCriterion's mask counts target s when s = 0 or w[s - 1] > 0.

Dimensions V = 67 (V1 = 68), F = 128, E = R = 128, B = 16 images of 1..7 label rows (0, 1, 5 and 16 words long),
theta = oracle.make_theta(d, 0, 4.0, 0.1): theta itself and two table-perturbed members of both signs. Stored: the label
rows, their image, per candidate the log-probs [rows, T + 1] (0 where the target does not count), and the torch and numpy
versions. theta, fc and the noise table are regenerated from the stored seeds. Prints the largest difference between
tests/xent_ref.py and the reference over every counted target: tests/test_xent_host.py holds the restatement to twice
that."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))

import make_golden as G  # noqa: E402  (sets the paths, imports the reference)
import xent_ref as X  # noqa: E402
from oracle import oracle as O  # noqa: E402

NOISE_LEN, TABLE_SEED, NOISE_SEED, ITERATION, SIGMA, MEMBERS = 1 << 21, 123, 7, 3, 0.01, (0, 1)
FC_SEED, LABEL_SEED, B = 1500, 1501, 16


def label_rows(d, rng):
    """per image 1..7 rows, lengths cycling through 0, 1, 5, T"""
    gts, r = [], 0
    for i in range(B):
        rows = np.zeros((1 + i % 7, d.T), np.int32)
        for k in range(rows.shape[0]):
            n = (0, 1, 5, d.T)[r % 4]
            rows[k, :n] = rng.integers(1, d.vocab_size + 1, n)
            r += 1
        gts.append(rows)
    return gts


def ref_forced(model, fc_rows, labels):
    """[n, T + 1] fp32 log-probs of the targets under the reference's modules, 0 where the target does not count"""
    fct = torch.from_numpy(np.ascontiguousarray(fc_rows))
    lab = torch.from_numpy(np.ascontiguousarray(labels, np.int64))
    n, T = lab.shape
    tgt = torch.cat([lab, lab.new_zeros(n, 1)], 1)
    state = model.init_hidden(n)
    _, state = model.core(model.img_embed(fct), state)
    out = np.zeros((n, T + 1), np.float32)
    mask = X.counted(labels)
    for s in range(T + 1):
        it = lab.new_zeros(n) if s == 0 else lab[:, s - 1]
        o, state = model.core(model.embed(it), state)
        lp = torch.nn.functional.log_softmax(model.logit(o), dim=1).gather(1, tgt[:, s:s + 1]).squeeze(1)
        out[:, s] = np.where(mask[:, s], lp.numpy(), np.float32(0))
    return out


def main():
    d = O.Dims(vocab_size=67, F=128)
    model = G.ref_model(d)
    theta = O.make_theta(d, 0, 4.0, 0.1)
    fc = np.random.Generator(np.random.PCG64(FC_SEED)).standard_normal((B, d.F)).astype(np.float32)
    gts = label_rows(d, np.random.Generator(np.random.PCG64(LABEL_SEED)))
    fc_rows, labels, row_img = X.rows_of(fc, gts)
    table = O.noise_table(NOISE_LEN, TABLE_SEED)
    cands = [theta]
    for m in MEMBERS:
        idx = O.noise_index(NOISE_SEED, ITERATION, m, NOISE_LEN, d.D)
        cands += [O.perturb(theta, table, idx, SIGMA, sign) for sign in (+1, -1)]
    lps, worst = [], 0.0
    mask = X.counted(labels)
    for th in cands:
        G.load_theta(model, th)
        ref = ref_forced(model, fc_rows, labels)
        mine, _, n_tok = X.forced(d, th, fc_rows, labels)
        assert np.array_equal(n_tok, mask.sum(1))
        worst = max(worst, float(np.abs(mine.astype(np.float64) - ref)[mask].max()))
        lps.append(ref)
    print('rows', labels.shape[0], 'targets', int(mask.sum()), 'largest |xent_ref - reference| over counted targets: %.3g' % worst)
    np.savez_compressed(os.path.join(G.OUT, 'xent.npz'),
                        dims=np.array([d.vocab_size, d.E, d.R, d.F, d.T], np.int64), theta_seed=np.int64(0),
                        gain=np.float64(4.0), bias_std=np.float64(0.1), fc_seed=np.int64(FC_SEED), B=np.int64(B),
                        labels=labels.astype(np.int32), row_img=row_img.astype(np.int32), logprobs=np.stack(lps),
                        noise_len=np.int64(NOISE_LEN), table_seed=np.int64(TABLE_SEED), noise_seed=np.int64(NOISE_SEED),
                        iteration=np.int64(ITERATION), sigma=np.float64(SIGMA), members=np.array(MEMBERS, np.int64),
                        measured_max_diff=np.float64(worst), torch_version=np.array(torch.__version__),
                        numpy_version=np.array(np.__version__))


if __name__ == '__main__':
    torch.set_num_threads(1)
    main()
