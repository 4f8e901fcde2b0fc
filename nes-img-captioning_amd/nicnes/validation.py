"""Validation-split evaluation: the score a run is judged by.

The reference's master waits for an eval result every iteration (nic_nes_master.py:92-120); the score is
NESWorker.accuracy -> CaptPolicy.accuracy_on -> eval_split (captioning/policies.py:130-143,
captioning/eval_utils.py:110-180): a greedy decode of the current theta on the first num_val_items images of
the split, one row per image, scored by COCOEvalCap (eval_utils.py:60-107). Here the split lives on the GPU
(Engine.make_split), is decoded in one call and scored by the engine's BLEU / ROUGE_L / CIDEr kernels.

Deviation, stated plainly: the metrics are computed on the split's LABEL ROWS -- word ids, captions cut to
seq_length words, rare words mapped to UNK -- not on PTB-tokenised raw annotations, so they equal COCOEvalCap's only
where those two coincide. METEOR and SPICE (java) are not computed.
"""
import numpy as np

from .engine import METRIC_KEYS  # noqa: F401  (re-exported)


def corpus_df(gts, seq_length=16):
    """The corpus document frequencies COCOEvalCap's Cider builds from the evaluated split's own references: per
    image, every distinct n-gram (n = 1..4) over its references counts once. gts: per image an int array
    [n_i, seq_length] of zero-padded label rows; a reference is its words before the first 0. Returns (sorted
    uint64 keys as pack_ngram packs them, float64 counts); ref_len_raw of this table is len(gts)."""
    rows = [np.asarray(g, np.int64).reshape(-1, seq_length) for g in gts]
    if not rows:
        return np.zeros(0, np.uint64), np.zeros(0, np.float64)
    refs = np.concatenate(rows, 0)
    img = np.repeat(np.arange(len(rows)), [r.shape[0] for r in rows])
    is0 = refs == 0
    length = np.where(is0.any(1), is0.argmax(1), seq_length)
    pairs = []
    for n in range(1, 5):
        if n > seq_length:
            break
        pos = np.arange(seq_length - n + 1)
        key = np.full((refs.shape[0], pos.size), n << 56, np.uint64)
        for k in range(n):
            key |= (refs[:, k:k + pos.size].astype(np.uint64) & np.uint64(0x3fff)) << np.uint64(42 - 14 * k)
        ok = pos[None, :] + n <= length[:, None]
        pairs.append(np.stack([np.broadcast_to(img[:, None], key.shape)[ok].astype(np.uint64), key[ok]], 1))
    pairs = np.unique(np.concatenate(pairs, 0), axis=0)            # one (image, n-gram) each
    keys, counts = np.unique(pairs[:, 1], return_counts=True)
    return keys.astype(np.uint64), counts.astype(np.float64)


def unpack_ngram(key):
    """The token-id tuple of a packed n-gram key (the inverse of engine.pack_ngram)."""
    key = int(key)
    n = key >> 56
    return tuple((key >> (42 - 14 * k)) & 0x3fff for k in range(n))


def decode_sequence(ix_to_word, seq):
    """captioning/eval_utils.py:13-27: the words of each row up to its first 0, joined by spaces. ix_to_word maps
    str(id) (the json's keys) or int ids to words."""
    out = []
    for row in np.asarray(seq):
        words = []
        for ix in row:
            ix = int(ix)
            if ix <= 0:
                break
            words.append(ix_to_word[str(ix)] if str(ix) in ix_to_word else ix_to_word[ix])
        out.append(' '.join(words))
    return out


class Validator:
    """eval_split of the reference on a resident split: the first `num` images of `split` in split_ix order (num =
    -1: all of them), as eval_split's num cut leaves them.

    loader: nicnes.data.CocoFcDataLoader, or any object with split_ix[split] (image indices), info['images'][ix]['id'],
    ix_to_word, seq_length, fc_feature(ix) -> [F] and labels (a LabelStore: every label row of image ix is
    labels.labels[label_start_ix[ix] - 1 : label_end_ix[ix]], the gts of get_batch).

    beam_size (1..8; None: greedy, the reference's eval during training) decodes with the engine's beam search
    (Split.decode_beam: the sum of log-probs, no length normalisation), as test-time evaluation usually does.

    xent=True adds the validation loss to eval_split's stats: 'val_loss' (the teacher-forced cross-entropy of theta on
    the split's label rows, Split.xent: what self-critical.pytorch's eval_split reports beside the language metrics)
    and 'val_perplexity'."""

    def __init__(self, engine, loader, split='val', num=5000, beam_size=None, xent=False):
        self.xent = bool(xent)
        if beam_size is not None and not 1 <= int(beam_size) <= 8:
            raise ValueError('beam_size must be in 1..8, got %r' % (beam_size,))
        self.beam_size = None if beam_size is None else int(beam_size)
        self.engine = engine
        self.loader = loader
        ixs = list(loader.split_ix[split])
        if num is not None and num >= 0:
            ixs = ixs[:num]
        if not ixs:
            raise ValueError('split %r has no images' % (split,))
        self.ixs = ixs
        self.image_ids = [loader.info['images'][ix]['id'] for ix in ixs]
        L, T = loader.labels, loader.seq_length
        self.gts = [np.asarray(L.labels[int(L.label_start_ix[ix]) - 1: int(L.label_end_ix[ix]), :T], np.int32)
                    for ix in ixs]
        fc = np.stack([np.asarray(loader.fc_feature(ix), np.float32).reshape(-1) for ix in ixs], 0)
        self.split = engine.make_split(fc, self.gts)

    def eval_split(self, incl_gts=False):
        """(lang_stats, predictions): COCOEvalCap's dict and [{'image_id', 'caption'}] in split order; incl_gts adds
        the reference strings as 'gts'."""
        stats, seq = self.split.evaluate(return_seq=True, **self._beam())
        if self.xent:
            x = self.split.xent()
            stats['val_loss'], stats['val_perplexity'] = x['loss'], x['perplexity']
        seq = seq.cpu().numpy() if hasattr(seq, 'cpu') else np.asarray(seq)
        sents = decode_sequence(self.loader.ix_to_word, seq)
        preds = []
        for k, (iid, sent) in enumerate(zip(self.image_ids, sents)):
            entry = {'image_id': iid, 'caption': sent}
            if incl_gts:
                entry['gts'] = decode_sequence(self.loader.ix_to_word, self.gts[k])
            preds.append(entry)
        return stats, preds

    def accuracy(self):
        """CaptPolicy.accuracy_on: the CIDEr of eval_split."""
        return float(self.split.evaluate(**self._beam())['CIDEr'])

    def _beam(self):
        """the decode's keyword: none at all for the greedy path (an engine without a beam decode still validates)"""
        return {} if self.beam_size is None else {'beam_size': self.beam_size}

    def close(self):
        self.split.close()
