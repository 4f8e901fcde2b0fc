"""Test helper: COCOEvalCap's java-free corpus metrics restated from the published algorithms (BLEU: Papineni et
al. 2002 as coco-caption's bleu_scorer computes it with option 'closest'; ROUGE-L: Lin 2004 as coco-caption's rouge
computes it, beta = 1.2), on captions given as lists of word ids. CIDEr-D comes from oracle/cider_ref.py on the same
words. Test infrastructure only; its own known answers are in tests/test_validation.py."""
import math
from collections import Counter

import numpy as np

from oracle import cider_ref as CR


def words(row):
    """decode_sequence: the tokens before the first 0"""
    out = []
    for t in row:
        if int(t) == 0:
            break
        out.append(int(t))
    return out


def ngrams(w, n):
    return Counter(tuple(w[i:i + n]) for i in range(len(w) - n + 1))


def bleu_stats(hyp, refs):
    """one image's (correct[1..4], guess[1..4], testlen, reflen)"""
    testlen = len(hyp)
    reflen = min((len(r) for r in refs), key=lambda l: (abs(l - testlen), l))
    correct, guess = [], []
    for n in range(1, 5):
        ch = ngrams(hyp, n)
        cr = Counter()
        for r in refs:
            for g, c in ngrams(r, n).items():
                cr[g] = max(cr[g], c)
        correct.append(sum(min(c, cr[g]) for g, c in ch.items()))
        guess.append(max(0, testlen - n + 1))
    return correct + guess + [testlen, reflen]


def bleu_from_totals(tot):
    tiny, small = 1e-15, 1e-9
    ratio = (tot[8] + tiny) / (tot[9] + small)
    out, b = [], 1.0
    for k in range(4):
        b *= (tot[k] + tiny) / (tot[4 + k] + small)
        v = b ** (1.0 / (k + 1))
        if ratio < 1:
            v *= math.exp(1 - 1 / ratio)
        out.append(v)
    return out


def lcs(a, b):
    t = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            t[i][j] = t[i - 1][j - 1] + 1 if a[i - 1] == b[j - 1] else max(t[i - 1][j], t[i][j - 1])
    return t[len(a)][len(b)]


def rouge_l(hyp, refs, beta=1.2):
    if not hyp:
        return 0.0
    p = max(lcs(hyp, r) / len(hyp) for r in refs)
    r = max((lcs(hyp, r) / len(r) if r else 0.0) for r in refs)
    if p == 0 or r == 0:
        return 0.0
    return (1 + beta ** 2) * p * r / (r + beta ** 2 * p)


def as_str(w):
    return ' '.join(str(t) for t in w)


def corpus_scorer(gts):
    """CIDEr-D with the corpus df of the references themselves (no end tokens)"""
    df, n = CR.document_frequency_from_refs([[as_str(words(r)) for r in g] for g in gts])
    return CR.CiderDOracle(df, n)


def corpus_metrics(seq, gts, scorer=None):
    """seq [N, T] hypothesis rows, gts per image [n_i, T] reference rows ->
    (totals [10] int, {'Bleu_1'..'CIDEr'}, per-image CIDEr-D [N])"""
    scorer = scorer or corpus_scorer(gts)
    tot = np.zeros(10, np.int64)
    rouge, cider = [], []
    for row, g in zip(seq, gts):
        hyp, refs = words(row), [words(r) for r in g]
        tot += np.asarray(bleu_stats(hyp, refs), np.int64)
        rouge.append(rouge_l(hyp, refs))
        cider.append(scorer.score_one(as_str(hyp), [as_str(r) for r in refs]))
    b = bleu_from_totals([int(t) for t in tot])
    m = {'Bleu_1': b[0], 'Bleu_2': b[1], 'Bleu_3': b[2], 'Bleu_4': b[3], 'ROUGE_L': float(np.mean(rouge)),
         'CIDEr': float(np.mean(cider))}
    return tot, m, np.asarray(cider)
