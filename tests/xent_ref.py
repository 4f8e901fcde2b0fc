"""Host restatement of the teacher-forced cross-entropy (include/nicnes.h NICNES_FITNESS_XENT, DESIGN.md
"Teacher-forced cross-entropy") -- TEST INFRASTRUCTURE ONLY.

The model is tests/ln_ref.py's Model with the normalisation off: the dense products are oracle.gemv (fp32 fma chains
from the bias in nn_kperm order) and the activations oracle.vec_math, in the order of the oracle's decode_core, so
feeding a greedy decode's own tokens back walks the oracle decode's states (tests/test_xent_host.py).

One label row w[0..T-1] (word ids, 0-padded; w[T] := 0) of an image with feature f:
  the image step cell(img_embed(f)) from zero state, logits discarded; then for s = 0..T the cell over embed(u_s),
  u_0 = 0 (BOS), u_s = w[s - 1], and lp_s = fl32(fl32(x[w[s]] - m) - lse) with m the row's largest logit and lse the
  oracle's: the fp64 exp-sum in ascending id order, its log rounded once to fp32 (greedy_pick of
  oracle/nicnes_oracle.c). Target s counts when s = 0 or w[s - 1] > 0. n_tok = the counted targets, lp_sum = the fp64
  sum of the counted lp_s in step order; loss = -sum lp_sum / sum n_tok over rows in row order; fitness = -loss."""
import numpy as np

from oracle import oracle as O
try:
    from tests import ln_ref as L
except ImportError:                      # scripts/make_golden_xent.py puts tests/ itself on the path
    import ln_ref as L

F32 = np.float32


def counted(labels):
    """[n, T] label rows -> bool [n, T + 1]: the targets that count (s = 0, and every s behind a word)"""
    labels = np.asarray(labels)
    return np.concatenate([np.ones((labels.shape[0], 1), bool), labels > 0], 1)


def forced(dims, theta, fc_rows, labels):
    """fc_rows [n, F] (each label row's image feature), labels [n, T] -> (lp f32 [n, T + 1], 0 where the target does
    not count; lp_sum f64 [n]; n_tok int32 [n])"""
    model = L.Model(dims, theta, layer_n=False)
    labels = np.ascontiguousarray(labels, np.int64)
    n, T = labels.shape
    assert T == dims.T
    mask = counted(labels)
    last = np.array([np.flatnonzero(r).max() for r in mask])           # the row's last counted target
    tgt = np.concatenate([labels, np.zeros((n, 1), np.int64)], 1)
    lp = np.zeros((n, T + 1), F32)
    h, c = np.zeros((n, dims.R), F32), np.zeros((n, dims.R), F32)
    h, c = model.cell(model.product(model.Wimg, model.bimg, np.ascontiguousarray(fc_rows, F32)), h, c)
    for s in range(int(last.max()) + 1):
        u = np.zeros(n, np.int64) if s == 0 else labels[:, s - 1]
        h, c = model.cell(model.emb[u], h, c)
        logits = model.product(model.Wl, model.bl, h)
        m = logits.max(1)
        d = (logits - m[:, None]).astype(F32)
        lse = np.log(np.add.accumulate(np.exp(d.astype(np.float64)), axis=1)[:, -1]).astype(F32)
        x = (logits[np.arange(n), tgt[:, s]] - m).astype(F32)
        lp[:, s] = np.where(mask[:, s], (x - lse).astype(F32), F32(0))
    lp_sum = np.zeros(n, np.float64)
    for s in range(T + 1):                                              # step order
        lp_sum = np.where(mask[:, s], lp_sum + lp[:, s].astype(np.float64), lp_sum)
    return lp, lp_sum, mask.sum(1).astype(np.int32)


def loss_of(lp_sum, n_tok):
    """-sum lp_sum / sum n_tok, both sums in row order in fp64"""
    a = np.add.accumulate(np.asarray(lp_sum, np.float64))[-1]
    return float(-a / float(np.asarray(n_tok, np.int64).sum()))


def rows_of(fc, gts):
    """a batch (fc [B, F], gts: per image [n_i, T] label rows) -> (fc_rows [n, F], labels [n, T], row_img [n])"""
    rows = [np.asarray(g, np.int32).reshape(-1, np.asarray(g).shape[-1]) for g in gts]
    row_img = np.concatenate([np.full(r.shape[0], i, np.int64) for i, r in enumerate(rows)])
    return np.asarray(fc, F32)[row_img], np.concatenate(rows, 0), row_img


def fitness(dims, theta, fc, gts):
    """the xent fitness of theta on a batch: -loss over its label rows"""
    fr, lab, _ = rows_of(fc, gts)
    _, lp_sum, n_tok = forced(dims, theta, fr, lab)
    return -loss_of(lp_sum, n_tok)
