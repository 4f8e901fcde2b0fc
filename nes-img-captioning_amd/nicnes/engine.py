"""Engine: a Python owner of one libnicnes handle on one GPU.

PyTorch-ROCm tensors are used for device storage only (their data_ptr() goes through the C ABI);
all arithmetic of the path runs in the HIP kernels of libnicnes.so.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import NicnesConfig, check

SEQ_LENGTH = 16          # FCModel.seq_length, /root/reference/src/captioning/nets.py:147


def pack_ngram(tokens):
    """Exact uint64 key of an n-gram of token ids (n<<56 | t0<<42 | t1<<28 | t2<<14 | t3); the
    word strings of array_to_str (/root/reference/src/algorithm/tools/utils.py:34-40) are the ids."""
    n = len(tokens)
    assert 1 <= n <= 4
    key = n << 56
    for k, t in enumerate(tokens):
        t = int(t)
        assert 0 <= t < 16384
        key |= t << (42 - 14 * k)
    return key


def df_table_arrays(document_frequency):
    """{tuple-of-str-or-int n-gram: df} -> (sorted uint64 keys, float64 df)."""
    items = sorted((pack_ngram(tuple(int(w) for w in g)), float(v)) for g, v in document_frequency.items())
    keys = np.array([k for k, _ in items], dtype=np.uint64)
    vals = np.array([v for _, v in items], dtype=np.float64)
    return keys, vals


def decode_queue_plan(members, slabs=1, n_cu=256, mode=None, workers=0):
    """(queue kernel runs, its workgroups, ring slots) of a screened fused decode of members x slabs member slabs
    (nicnes_decode_queue_plan; needs no GPU). mode None: mode and workers from NICNES_DECODE_QUEUE[_WORKERS]."""
    from ._lib import lib
    out = (ctypes.c_int32 * 3)()
    m = -1 if mode is None else (2 if mode == 'auto' else int(mode))
    check(lib().nicnes_decode_queue_plan(m, int(workers), int(n_cu), int(members), int(slabs), out), None,
          'decode_queue_plan')
    return bool(out[0]), int(out[1]), int(out[2])


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


class Engine:
    """One handle = one GPU. ``device`` is the local cuda index."""

    def __init__(self, vocab_size=9487, input_encoding_size=128, rnn_size=128, fc_feat_size=2048,  # noqa: E501
                 seq_length=SEQ_LENGTH, max_batch=128, max_refs=None, max_members=512, noise_len=1 << 27,
                 noise_seed=0, device=0, lib_path=None, layer_n=False, layer_n_affine=False):
        self.L = _lib.lib(lib_path)
        self.device = torch.device('cuda', device)
        self.cfg = NicnesConfig(vocab_size, input_encoding_size, rnn_size, fc_feat_size, seq_length, max_batch,
                                max_refs or 8 * max_batch, max_members, noise_len, noise_seed,
                                int(bool(layer_n)), int(bool(layer_n_affine)))
        # layer_n_affine without layer_n is ignored, as the reference ignores it
        self.layer_n, self.layer_n_affine = bool(layer_n), bool(layer_n and layer_n_affine)
        self.D = int(self.L.nicnes_param_count(ctypes.byref(self.cfg)))
        off = (ctypes.c_int64 * 10)()
        check(self.L.nicnes_param_offsets(ctypes.byref(self.cfg), off), None, 'nicnes_param_offsets')
        self.offsets = list(off)
        self.ln_offsets = None           # layer_n_affine: the six tail tensors' offsets + D
        if self.layer_n_affine:
            off7 = (ctypes.c_int64 * 7)()
            check(self.L.nicnes_param_offsets_ln(ctypes.byref(self.cfg), off7), None, 'nicnes_param_offsets_ln')
            self.ln_offsets = list(off7)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(self.L.nicnes_create(ctypes.byref(self.cfg), device, ctypes.byref(h)), None, 'nicnes_create')
        self.h = h
        self.n_cu = torch.cuda.get_device_properties(self.device).multi_processor_count
        self.coop_mode = 0 if os.environ.get('NICNES_DECODE_COOP') == '0' else 1
        self._keep = {}
        self.B = 0
        self.fitness_mode = 0
        self.rpi = 1

    # -------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, 'h', None):
            self.L.nicnes_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, a, dtype):
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a)).to(device=self.device, dtype=dtype)

    # ---------------------------------------------------------------- state -------------
    def set_noise_table(self, table):
        t = self._dev(table, torch.float32)
        assert t.numel() == self.cfg.noise_len
        self._keep['noise'] = t
        check(self.L.nicnes_set_noise_table(self.h, _ptr(t), ctypes.c_uint64(t.numel())), self.h, 'set_noise_table')

    def set_theta(self, theta, fp32_origin=None):
        """theta: fp32 (reference start, fp32 first-step semantics) or fp64 vector [D]."""
        if fp32_origin is None:
            fp32_origin = (theta.dtype == np.float32) if isinstance(theta, np.ndarray) else theta.dtype == torch.float32
        t = self._dev(theta, torch.float64)
        assert t.numel() == self.D
        with torch.cuda.device(self.device):
            check(self.L.nicnes_set_theta(self.h, _ptr(t), int(bool(fp32_origin)), self._stream()), self.h, 'set_theta')
        self._keep['theta_in'] = t

    def theta(self):
        t64 = torch.empty(self.D, dtype=torch.float64, device=self.device)
        t32 = torch.empty(self.D, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_get_theta(self.h, _ptr(t64), _ptr(t32), self._stream()), self.h, 'get_theta')
        return t64, t32

    def adam_state(self):
        m = torch.empty(self.D, dtype=torch.float64, device=self.device)
        v = torch.empty(self.D, dtype=torch.float64, device=self.device)
        t = ctypes.c_int64()
        with torch.cuda.device(self.device):
            check(self.L.nicnes_get_adam_state(self.h, _ptr(m), _ptr(v), ctypes.byref(t), self._stream()), self.h,
                  'get_adam_state')
        return m, v, t.value

    def set_adam_state(self, m, v, t):
        m = self._dev(m, torch.float64)
        v = self._dev(v, torch.float64)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_set_adam_state(self.h, _ptr(m), _ptr(v), int(t), self._stream()), self.h,
                  'set_adam_state')
        self._keep['adam_m'], self._keep['adam_v'] = m, v

    def set_df_table(self, keys, df, ref_len_log):
        k = self._dev(np.asarray(keys, np.uint64).view(np.int64), torch.int64)
        d = self._dev(np.asarray(df, np.float64), torch.float64)
        self._keep['df_keys'], self._keep['df_vals'] = k, d
        check(self.L.nicnes_set_df_table(self.h, _ptr(k), _ptr(d), int(k.numel()), float(ref_len_log)), self.h,
              'set_df_table')

    def set_batch(self, fc, gts):
        """fc [B, F] fp32 of unique images; gts: per image an int array [n_i, seq_length] of
        zero-padded label rows (data['gts'], /root/reference/src/captioning/dataloader.py:162)."""
        self.set_batches([(fc, gts)])

    def set_batches(self, batches):
        """Several batches of equal size B at once, [(fc [B, F], gts), ...], for per-member batches
        (single_batch: false, /root/reference/src/algorithm/nic_nes/nic_nes_worker.py:121-128): an
        evaluate's member_batch then names each member's batch."""
        fcs, rows, start = [], [], [0]
        for fc, gts in batches:
            fc_np = fc.detach().cpu().numpy() if isinstance(fc, torch.Tensor) else np.asarray(fc, np.float32)
            if len(gts) != fc_np.shape[0]:
                raise ValueError('gts has %d images, fc has %d rows' % (len(gts), fc_np.shape[0]))
            fcs.append(np.asarray(fc_np, np.float32))
            for g in gts:
                g = np.asarray(g, np.int32).reshape(-1, self.cfg.seq_length)
                rows.append(g)
                start.append(start[-1] + g.shape[0])
        B = fcs[0].shape[0]
        if any(f.shape[0] != B for f in fcs):
            raise ValueError('batches must have the same number of images')
        refs_np = np.concatenate(rows, 0)
        # the scorer packs a token id into 14 bits of the n-gram key: an id outside the vocabulary would alias another word
        if refs_np.size and (refs_np.min() < 0 or refs_np.max() > self.cfg.vocab_size):
            raise ValueError('reference token outside [0, vocab_size = %d]: min %d, max %d'
                             % (self.cfg.vocab_size, refs_np.min(), refs_np.max()))
        fc_t = self._dev(np.concatenate(fcs, 0), torch.float32)
        refs = self._dev(refs_np, torch.int32)
        starts = self._dev(np.array(start, np.int32), torch.int32)
        self._keep['fc'], self._keep['refs'], self._keep['ref_start'] = fc_t, refs, starts
        with torch.cuda.device(self.device):
            check(self.L.nicnes_set_batches(self.h, _ptr(fc_t), len(fcs), B, _ptr(refs), int(refs.shape[0]),
                                            _ptr(starts), self._stream()), self.h, 'set_batches')
        self.B = B
        self.n_batches = len(fcs)

    def make_trainset(self, fc, gts, fc_rows=None):
        """A resident training set (nicnes_trainset_create): fc [N, F] fp32 (a numpy array or memory map, uploaded
        in chunks; or a tensor), gts per image an int array [n_i, seq_length] of zero-padded label rows. fc_rows:
        optional callable (indices) -> host fc rows, for callers that want rows back (mutations.batch_fc); a numpy fc
        serves as its own. Batches are then drawn from it by image index (draw_batches)."""
        return TrainSet(self, fc, gts, fc_rows)

    def draw_batches(self, trainset, image_ix):
        """set_batches for images image_ix ([n_batches, B] or [B] indices into the set) of a resident training set,
        gathered on the device (nicnes_draw_batches): only enqueues; the host sends the indices and nothing else."""
        ix = np.ascontiguousarray(np.asarray(image_ix, np.int32))
        if ix.ndim == 1:
            ix = ix[None]
        if ix.ndim != 2 or ix.shape[1] < 1:
            raise ValueError('image_ix must be [n_batches, B] or [B]')
        if trainset.engine is not self:
            raise ValueError('the training set belongs to another engine')
        with torch.cuda.device(self.device):
            check(self.L.nicnes_draw_batches(self.h, trainset.ts, ix.ctypes.data_as(ctypes.c_void_p), int(ix.shape[0]),
                                             int(ix.shape[1]), self._stream()), self.h, 'draw_batches')
        self.B = int(ix.shape[1])
        self.n_batches = int(ix.shape[0])

    def test_batch_state(self, n_refs=None):
        """Test entry: (fc [n_batches * B, F], reference rows [n_refs, seq_length], starts [n_batches * B + 1]) the
        handle currently reads, whichever call set them; tensors on the GPU. The reference-row buffer is sized from
        the handle's own starts (read back first: synchronises); n_refs, when given, must be that count."""
        n_img = self.B * getattr(self, 'n_batches', 1)
        starts = torch.empty(n_img + 1, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_test_batch_state(self.h, None, None, _ptr(starts), self._stream()), self.h,
                  'test_batch_state')
            held = int(starts[-1].item())
            if n_refs is not None and int(n_refs) != held:
                raise ValueError('the handle holds %d reference rows, not %d' % (held, int(n_refs)))
            fc = torch.empty((n_img, self.cfg.fc_feat_size), dtype=torch.float32, device=self.device)
            refs = torch.empty((held, self.cfg.seq_length), dtype=torch.int32, device=self.device)
            check(self.L.nicnes_test_batch_state(self.h, _ptr(fc), _ptr(refs), None, self._stream()), self.h,
                  'test_batch_state')
        return fc, refs, starts

    def make_split(self, fc, gts=None, df=None, ref_len_raw=None):
        """A resident evaluation split (nicnes_split_create): fc [N, F] fp32, gts per image an int array
        [n_i, seq_length] of zero-padded label rows (None: a decode-only split). df: the split's own document
        frequencies, {n-gram tuple: count} or (sorted uint64 keys, counts); None builds the corpus df from gts (every
        distinct n-gram over an image's references counts once, ref_len_raw = the number of images: what
        COCOEvalCap's Cider does). The training batches, the handle's df table and every setter's state stay as
        they are."""
        return Split(self, fc, gts, df, ref_len_raw)

    # ---------------------------------------------------------------- the hot path -------
    def noise_indices(self, iteration, member_begin, count):
        out = torch.empty(count, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_noise_indices(self.h, ctypes.c_uint64(iteration), member_begin, count, _ptr(out),
                                              self._stream()), self.h, 'noise_indices')
        return out

    def noise_vectors(self, iteration, member_begin, count, sigma, out=None):
        """delta [count, D] fp32 = fp32(sigma * table slice) of members [member_begin, +count) (the
        vectors a reference-format NESResult carries)."""
        o = out if out is not None else torch.empty((count, self.D), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_noise_vectors(self.h, ctypes.c_uint64(iteration), member_begin, count,
                                              ctypes.c_float(sigma), _ptr(o), self._stream()), self.h, 'noise_vectors')
        return o

    MUTATION_MODES = {'plain': 0, 'divide': 1, 'scale': 2}

    def set_mutation(self, mode='plain', vec=None):
        """Per-parameter noise transform of safe / proportional mutations: 'divide' (delta / vec:
        SM-G-SUM, SM-G-ABS, SM-VECTOR with vec = the sensitivity), 'scale' (delta * vec:
        SM-PROPORTIONAL), 'plain' off."""
        code = self.MUTATION_MODES[mode] if isinstance(mode, str) else int(mode)
        v = self._dev(vec, torch.float32) if vec is not None else None
        if v is not None and v.numel() != self.D:
            raise ValueError('mutation vector needs D entries')
        with torch.cuda.device(self.device):
            check(self.L.nicnes_set_mutation(self.h, code, _ptr(v), self._stream()), self.h, 'set_mutation')
        self._keep['mutation'] = v
        self.mutation_mode = code

    def set_mutation_proportional(self, mean_abs):
        """SM-PROPORTIONAL's vector formed on the device from the handle's fp32 theta
        (nicnes_set_mutation_proportional): |theta| with exact zeros replaced by mean_abs, the caller's fp32
        mean of |theta| (nets.py:108-112); then mode 'scale'."""
        with torch.cuda.device(self.device):
            check(self.L.nicnes_set_mutation_proportional(self.h, float(mean_abs), self._stream()), self.h,
                  'set_mutation_proportional')
        self._keep['mutation'] = None
        self.mutation_mode = self.MUTATION_MODES['scale']

    def theta_zeros(self):
        """How many entries of the fp32 theta are exactly zero (nicnes_theta_zeros; synchronises)."""
        out = ctypes.c_int64(0)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_theta_zeros(self.h, ctypes.byref(out), self._stream()), self.h, 'theta_zeros')
        return int(out.value)

    # Fitness enum values the engine implements (src/captioning/policies.py:22-35) -> nicnes.h codes
    FITNESS_MODES = {'greedy': 0, 'greedy_logprob': 1, 'greedy_expprob': 2, 'greedy_linprob': 3,
                     'greedy_avgprob': 4, 'sample': 5, 'self_critical': 6, 'sc_loss': 7,
                     'xent': 8}      # 'xent': the engine's extension (teacher-forced likelihood of the label rows)
    SAMPLED_MODES = (5, 6, 7)
    XENT_MODE = 8

    def set_fitness_mode(self, fitness):
        """Fitness criterion by its experiment-JSON name (policy_options.fitness), or by the nicnes.h code of a member
        of the reference's Fitness enum (0..7). The engine's own extension has no place in that enum and is chosen by
        its name, 'xent', only: an integer beyond the enum stays an error here, as it was before the extension took
        the next code of the C ABI (NICNES_FITNESS_XENT = 8)."""
        if isinstance(fitness, str):
            code = self.FITNESS_MODES.get(fitness, -1)
        else:
            code = int(fitness)
            if code == self.XENT_MODE:
                raise ValueError("set_fitness_mode(%r): integer codes name the reference's Fitness enum (0..7); "
                                 "choose the engine's extension by its name, 'xent'" % (fitness,))
        check(self.L.nicnes_set_fitness_mode(self.h, code), self.h, 'set_fitness_mode(%r)' % (fitness,))
        self.fitness_mode = code

    def evaluate(self, iteration, member_begin, count, sigma, fitness_out=None, return_seq=False, return_lp=False,
                 member_batch=None):
        """Fitness (f+, f-) of members [member_begin, +count): tensor [count, 2] fp64 on the GPU.
        return_seq / return_lp add the greedy tokens [count, 2, B, T] int32 and their per-step
        log-probs (FCModel._sample's seq_logprobs) [count, 2, B, T] fp32. member_batch: per member the
        index of its batch among set_batches' (None: the one batch held)."""
        fit = fitness_out if fitness_out is not None else torch.empty((count, 2), dtype=torch.float64,
                                                                      device=self.device)
        shape = (count, 2, self.rollout_rows(), self.cfg.seq_length)
        seq = torch.empty(shape, dtype=torch.int32, device=self.device) if return_seq else None
        lp = torch.empty(shape, dtype=torch.float32, device=self.device) if return_lp else None
        mb = None
        if member_batch is not None:
            mb_np = np.ascontiguousarray(np.asarray(member_batch, np.int32))
            if mb_np.shape != (count,):
                raise ValueError('member_batch needs one entry per member')
            mb = mb_np.ctypes.data_as(ctypes.c_void_p)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_evaluate_batches(self.h, ctypes.c_uint64(iteration), member_begin, count,
                                                 ctypes.c_float(sigma), mb, _ptr(fit), _ptr(seq), _ptr(lp),
                                                 self._stream()), self.h, 'evaluate')
        out = (fit,) + ((seq,) if return_seq else ()) + ((lp,) if return_lp else ())
        return out if len(out) > 1 else fit

    def xent_batch_rows(self, batch=0):
        """Label rows (reference rows) of batch `batch` of the batches held: the rows an 'xent' evaluate runs."""
        out = ctypes.c_int32(0)
        check(self.L.nicnes_xent_batch_rows(self.h, int(batch), ctypes.byref(out)), self.h, 'xent_batch_rows')
        return int(out.value)

    def xent_rows(self, cand=0, batch=0):
        """After an evaluate in 'xent' mode: candidate cand's (member k sign s: 2 k + s; evaluate_theta: 0) per-row
        (lp_sum [rows] fp64, n_tok [rows] int32) over the label rows of its batch `batch`; tensors on the GPU."""
        rows = self.xent_batch_rows(batch)
        lp = torch.empty(rows, dtype=torch.float64, device=self.device)
        nt = torch.empty(rows, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_xent_rows(self.h, int(cand), rows, _ptr(lp), _ptr(nt), self._stream()), self.h, 'xent_rows')
        return lp, nt

    def test_xent_steps(self, iteration=0, member_begin=0, count=1, sigma=0.0, member_batch=None, theta_batch=None):
        """Test entry: the 'xent' evaluate returning every counted target's log-prob, 0 elsewhere. Members: (fitness
        [count, 2], lp [count, 2, stride, T + 1]) with stride = the largest batch's label rows; theta_batch = b: theta
        itself on batch b, (fitness [1], lp [rows of b, T + 1]). Tensors on the GPU (synchronises)."""
        T1 = self.cfg.seq_length + 1
        mb = None
        if theta_batch is not None:
            fit = torch.empty(1, dtype=torch.float64, device=self.device)
            lp = torch.empty((self.xent_batch_rows(theta_batch), T1), dtype=torch.float32, device=self.device)
        else:
            stride = max(self.xent_batch_rows(b) for b in range(getattr(self, 'n_batches', 1)))
            fit = torch.empty((count, 2), dtype=torch.float64, device=self.device)
            lp = torch.empty((count, 2, stride, T1), dtype=torch.float32, device=self.device)
            if member_batch is not None:
                mb_np = np.ascontiguousarray(np.asarray(member_batch, np.int32))
                if mb_np.shape != (count,):
                    raise ValueError('member_batch needs one entry per member')
                mb = mb_np.ctypes.data_as(ctypes.c_void_p)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_test_xent_steps(self.h, ctypes.c_uint64(iteration), int(member_begin), int(count),
                                                ctypes.c_float(sigma), mb, -1 if theta_batch is None else int(theta_batch),
                                                _ptr(fit), _ptr(lp), self._stream()), self.h, 'test_xent_steps')
            torch.cuda.current_stream().synchronize()
        return fit, lp

    def set_rows_per_image(self, n=1):
        """Sampled modes: decode n rows per image of the batch (the reference's seq_per_img copies, each with
        its own draws); greedy modes always decode one."""
        check(self.L.nicnes_set_rows_per_image(self.h, int(n)), self.h, 'set_rows_per_image')
        self.rpi = int(n)

    def rollout_rows(self):
        """Rows of one rollout: the batch's images, times rows_per_image in the sampled modes."""
        return self.B * (getattr(self, 'rpi', 1) if self.fitness_mode in self.SAMPLED_MODES else 1)

    def set_sample_draws(self, u=None):
        """Test hook: the uniforms [count, 2, B, T] fp64 the next sampled evaluates use (None: the engine's
        own counter-based draws)."""
        if u is None:
            check(self.L.nicnes_set_sample_draws(self.h, None, 0), self.h, 'set_sample_draws')
            self._keep.pop('draws', None)
            return
        a = np.ascontiguousarray(np.asarray(u, np.float64))
        check(self.L.nicnes_set_sample_draws(self.h, a.ctypes.data_as(ctypes.c_void_p), a.size), self.h,
              'set_sample_draws')
        self._keep['draws'] = a

    def evaluate_theta(self, batch=0, return_seq=False, return_lp=False, iteration=0):
        """Fitness of theta itself on the batch held (or batch `batch` of set_batches'): the sigma = 0
        rollout (CaptPolicy.rollout) decoded once, sign + over the first half of the images and sign -
        over the rest. Tensor [1] fp64 on the GPU; return_seq / return_lp add [B, T] tokens / log-probs.
        iteration: the draw stream of the sampled modes (each eval rollout its own)."""
        fit = torch.empty(1, dtype=torch.float64, device=self.device)
        shape = (self.rollout_rows(), self.cfg.seq_length)
        seq = torch.empty(shape, dtype=torch.int32, device=self.device) if return_seq else None
        lp = torch.empty(shape, dtype=torch.float32, device=self.device) if return_lp else None
        with torch.cuda.device(self.device):
            check(self.L.nicnes_evaluate_theta(self.h, int(batch), int(iteration), _ptr(fit), _ptr(seq), _ptr(lp),
                                               self._stream()),
                  self.h, 'evaluate_theta')
        out = (fit,) + ((seq,) if return_seq else ()) + ((lp,) if return_lp else ())
        return out if len(out) > 1 else fit

    def rank_weights(self, fitness_all):
        """fitness [P, 2] fp64 (whole population) -> (centred ranks [P, 2] fp64, weights [P] fp32)."""
        P = fitness_all.shape[0]
        cr = torch.empty((P, 2), dtype=torch.float64, device=self.device)
        w = torch.empty(P, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_rank_weights(self.h, _ptr(fitness_all), P, _ptr(cr), _ptr(w), self._stream()), self.h,
                  'rank_weights')
        return cr, w

    def grad_partial(self, iteration, member_begin, count, w_shard, sigma, out=None):
        g = out if out is not None else torch.empty(self.D, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_grad_partial(self.h, ctypes.c_uint64(iteration), member_begin, count, _ptr(w_shard),
                                             ctypes.c_float(sigma), _ptr(g), self._stream()), self.h, 'grad_partial')
        return g

    def grad_partial_range(self, iteration, member_begin, count, w_shard, sigma, j0, j1, out):
        """grad_partial on parameters [j0, j1) of `out` (j0 a multiple of 64)."""
        with torch.cuda.device(self.device):
            check(self.L.nicnes_grad_partial_range(self.h, ctypes.c_uint64(iteration), member_begin, count,
                                                   _ptr(w_shard), ctypes.c_float(sigma), int(j0), int(j1), _ptr(out),
                                                   self._stream()), self.h, 'grad_partial_range')
        return out

    def adam_step(self, gsum, P, l2coeff, stepsize, beta1=0.9, beta2=0.999, epsilon=1e-08, sync=True):
        """Adam on the engine's theta. sync=True returns the update ratio (one host sync); sync=False
        only enqueues the step and returns None (read the ratio later with last_ratio())."""
        ratio = ctypes.c_double()
        with torch.cuda.device(self.device):
            check(self.L.nicnes_adam_step(self.h, _ptr(gsum), P, l2coeff, stepsize, beta1, beta2, epsilon,
                                          ctypes.byref(ratio) if sync else None, self._stream()), self.h, 'adam_step')
        return ratio.value if sync else None

    def last_ratio(self):
        """Update ratio of the newest optimizer step (synchronising)."""
        ratio = ctypes.c_double()
        with torch.cuda.device(self.device):
            check(self.L.nicnes_last_ratio(self.h, ctypes.byref(ratio), self._stream()), self.h, 'last_ratio')
        return ratio.value

    def sgd_step(self, gsum, P, l2coeff, stepsize, momentum=0.9):
        ratio = ctypes.c_double()
        with torch.cuda.device(self.device):
            check(self.L.nicnes_sgd_step(self.h, _ptr(gsum), P, l2coeff, stepsize, momentum, ctypes.byref(ratio),
                                         self._stream()), self.h, 'sgd_step')
        return ratio.value

    def optimizer_update(self, globalg, kind='adam', stepsize=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-08):
        """Optimizer.update(globalg) form: globalg [D] fp32 or fp64 -> update ratio."""
        is32 = (globalg.dtype == torch.float32) if isinstance(globalg, torch.Tensor) else \
            (np.asarray(globalg).dtype == np.float32)
        g = self._dev(globalg, torch.float64)
        ratio = ctypes.c_double()
        with torch.cuda.device(self.device):
            check(self.L.nicnes_optimizer_update(self.h, {'adam': 0, 'sgd': 1}[kind], _ptr(g), int(is32), stepsize,
                                                 beta1, beta2, epsilon, ctypes.byref(ratio), self._stream()), self.h,
                  'optimizer_update')
        return ratio.value

    def set_timing(self, on=True):
        check(self.L.nicnes_set_timing(self.h, int(bool(on))), self.h, 'set_timing')

    def kernel_times(self):
        """(decode_ms, cider_ms) of the last evaluate() (HIP events on its stream)."""
        out = (ctypes.c_float * 2)()
        check(self.L.nicnes_kernel_times(self.h, out), self.h, 'kernel_times')
        return float(out[0]), float(out[1])

    def decode_phase_times(self):
        """Per-kernel split of the last timed decode (HIP events between its launches): img_ms,
        step_ms / step_launches (fused path: the steps kernel, every step t = -1..T in one launch; one
        launch per step in DECODE_PROF timing builds, whose first two, cell-only, launches are also in
        cell_only_ms), logit_ms / logit_launches and cell_ms / cell_launches (split path)."""
        out = (ctypes.c_float * 8)()
        check(self.L.nicnes_decode_phase_times(self.h, out), self.h, 'decode_phase_times')
        return {'img_ms': float(out[0]), 'cell_only_ms': float(out[1]), 'step_ms': float(out[2]),
                'step_launches': int(out[3]), 'logit_ms': float(out[4]), 'logit_launches': int(out[5]),
                'cell_ms': float(out[6]), 'cell_launches': int(out[7])}

    def set_decode_split(self, S=0, G=0):
        """Force the decode shape (S logit workgroups per member slab, G = 4 / 2 row groups per slab);
        0 = automatic. Tokens do not depend on it."""
        check(self.L.nicnes_set_decode_split(self.h, int(S), int(G)), self.h, 'set_decode_split')

    def set_decode_streams(self, n=0):
        """Split the evaluate's members over n streams (0 = automatic: 2 on the split path, 1 fused).
        Tokens do not depend on it."""
        check(self.L.nicnes_set_decode_streams(self.h, int(n)), self.h, 'set_decode_streams')

    def sum_sensitivity(self, rows, underflow=0.0, out=None):
        """SM-G-SUM sensitivity (Sensitivity.calc_sensitivity, safe_mutations.py:34-117) of the current theta
        on the first `rows` images of the batch held: fp32 [D] on the GPU, clamped and scaled by
        `underflow` when it is > 0 (the vector set_mutation('divide', ...) takes)."""
        v = out if out is not None else torch.empty(self.D, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_sum_sensitivity(self.h, int(rows), ctypes.c_float(underflow), _ptr(v), self._stream()),
                  self.h, 'sum_sensitivity')
        return v

    SENS_PATH_BITS = ('logit_fast', 'bwd_fused', 'gates_bsq', 'emb_two_pass')

    def sens_paths(self):
        """The kernels the last sensitivity run of this handle chose (sum_sensitivity, or es_sensitivity's last slot):
        {'logit_fast', 'bwd_fused', 'gates_bsq', 'emb_two_pass': bool (False: the general tile / range kernel),
        'gemm_v4', 'gemm_scalar': the run's tile products with 16-byte and with scalar operand loads}. Host
        bookkeeping (nicnes_sens_paths): no kernel runs. Raises before the first run."""
        out = (ctypes.c_int32 * 3)()
        check(self.L.nicnes_sens_paths(self.h, out), self.h, 'sens_paths')
        d = {name: bool(out[0] >> i & 1) for i, name in enumerate(self.SENS_PATH_BITS)}
        d.update(gemm_v4=int(out[1]), gemm_scalar=int(out[2]))
        return d

    def set_decode_coop(self, mode=1):
        """1 (default): the split shape (128-row slabs, S = 2 or 4, every workgroup resident) runs as one
        persistent launch whose workgroups hand partial states and h' to each other; 0: two launches per
        step. Tokens do not depend on it."""
        check(self.L.nicnes_set_decode_coop(self.h, int(mode)), self.h, 'set_decode_coop')
        self.coop_mode = int(mode)

    def last_decode_bounded(self):
        """True when the last greedy decode enqueued used the pair-bounded lse (the steps kernel's PAIRS instantiation)."""
        out = ctypes.c_int32()
        check(self.L.nicnes_last_decode_lse(self.h, ctypes.byref(out)), self.h, 'last_decode_lse')
        return bool(out.value)

    def set_decode_screen(self, on):
        """The bf16-screened logit loop of the fused greedy-only decode on (True), off (False) or 'auto' (the default:
        on when members x slabs reach the CU count). Tokens do not depend on it."""
        mode = 2 if (isinstance(on, str) and on == 'auto') else int(bool(on))
        check(self.L.nicnes_set_decode_screen(self.h, mode), self.h, 'set_decode_screen')

    def set_decode_queue(self, mode='auto', workers=0):
        """The screened decode's step queue on (True), off (False) or 'auto' (the default: on when the decode has more
        member slabs than workers); workers 0: one per CU. Tokens do not depend on it."""
        m = 2 if (isinstance(mode, str) and mode == 'auto') else int(bool(mode))
        check(self.L.nicnes_set_decode_queue(self.h, m, int(workers)), self.h, 'set_decode_queue')

    def test_logit_chain(self, iteration, member, sigma, sign, h_rows):
        """Test entry: the logits of one (member, sign) over h_rows [32, 128] by the exact pass's MFMA tile path and by
        the fmaf chain in the MFMA's k order; two [32, vocab_size + 1] fp32 tensors, equal bit for bit."""
        hr = torch.as_tensor(h_rows, dtype=torch.float32, device=self.device).contiguous()
        assert hr.shape == (32, self.cfg.rnn_size)
        om = torch.empty((32, self.cfg.vocab_size + 1), dtype=torch.float32, device=self.device)
        oc = torch.empty_like(om)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_test_logit_chain(self.h, ctypes.c_uint64(iteration), int(member), ctypes.c_float(sigma),
                                                 int(sign), _ptr(hr), _ptr(om), _ptr(oc), self._stream()), self.h,
                  'test_logit_chain')
            torch.cuda.current_stream().synchronize()   # hr stays alive until the kernel has read it
        return om, oc

    def test_certify_items(self, iteration, member, sigma, sign, h_rows, items, owner_by_id=False):
        """Test entry: items [n, 2] of (row < 128, vocabulary id) over h_rows [128, 128] through the screened decode's
        tile certify; an fp32 tensor [n] of their exact logits. An id or row out of range raises. owner_by_id: an item
        belongs to the lane half its id's bit 2 names, as in a decode (default: to lane half 0 of its row)."""
        hr = torch.as_tensor(h_rows, dtype=torch.float32, device=self.device).contiguous()
        assert hr.shape == (128, self.cfg.rnn_size)
        it = np.ascontiguousarray(np.asarray(items, dtype=np.int32).reshape(-1, 2))
        n = int(it.shape[0])
        out = torch.empty((max(n, 1),), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_test_certify_items_owned(self.h, ctypes.c_uint64(iteration), int(member),
                                                         ctypes.c_float(sigma), int(sign), int(bool(owner_by_id)), _ptr(hr),
                                                         it.ctypes.data_as(ctypes.c_void_p), n, _ptr(out),
                                                         self._stream()), self.h, 'test_certify_items')
        return out[:n]

    def test_score_rows(self, seq, member_batch=None, lp=None, base=None):
        """Test entry: the evaluate's scorer on given token rows. seq [n_cand, rows, seq_length] int; member_batch
        (n_cand / 2 batch indices), lp [n_cand, rows, seq_length] fp32 and base [n_cand, rows / rows_per_image] fp64
        are optional. Uses the fitness mode, rows per image, batches and df table the handle holds. Returns
        (scores [n_cand, rows], fitness [n_cand]), fp64 tensors on the GPU (synchronises)."""
        sq = self._dev(seq, torch.int32)
        if sq.dim() != 3 or sq.shape[2] != self.cfg.seq_length:
            raise ValueError('seq must be [n_cand, rows, seq_length]')
        n_cand, rows = int(sq.shape[0]), int(sq.shape[1])
        lp_t = self._dev(lp, torch.float32) if lp is not None else None
        if lp_t is not None and lp_t.shape != sq.shape:
            raise ValueError('lp must have the shape of seq')
        base_t = self._dev(base, torch.float64) if base is not None else None
        if base_t is not None and (base_t.dim() != 2 or base_t.shape[0] != n_cand or base_t.shape[1] < 1 or
                                   rows % base_t.shape[1]):
            raise ValueError('base must be [n_cand, rows / rows_per_image]')
        mb = None
        if member_batch is not None:
            mb_np = np.ascontiguousarray(np.asarray(member_batch, np.int32))
            if mb_np.ndim != 1 or mb_np.shape[0] < n_cand // 2:
                raise ValueError('member_batch needs one entry per member (two candidates each)')
            mb = mb_np.ctypes.data_as(ctypes.c_void_p)
        scores = torch.empty((n_cand, rows), dtype=torch.float64, device=self.device)
        fit = torch.empty(n_cand, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_test_score_rows(self.h, _ptr(sq), n_cand, rows, mb, _ptr(lp_t), _ptr(base_t),
                                                _ptr(scores), _ptr(fit), self._stream()), self.h, 'test_score_rows')
            torch.cuda.current_stream().synchronize()   # the inputs stay alive until the kernels have read them
        return scores, fit

    def set_beam_waves(self, waves=0):
        """The beam decode's workgroup shape: 4 or 8 waves, 0 the launch's own rule (results do not depend on it)."""
        check(self.L.nicnes_set_beam_waves(self.h, int(waves)), self.h, 'set_beam_waves')

    def test_beam_select(self, lp, score, live):
        """Test entry: the beam decode's own top-K and selection code on given rows. lp [n_img, K, V1] fp32 log-probs,
        score [n_img, K] fp64, live [n_img, K] (0: dead). Returns int32 [n_img, K, 2] on the GPU: every image's
        selected (b, v) pairs in selection order, (-1, -1) where fewer than K candidates exist (synchronises)."""
        lp_t = self._dev(lp, torch.float32)
        if lp_t.dim() != 3:
            raise ValueError('lp must be [n_img, K, V1]')
        n_img, K, V1 = (int(x) for x in lp_t.shape)
        sc_t = self._dev(score, torch.float64)
        lv_t = self._dev(live, torch.int32)
        if tuple(sc_t.shape) != (n_img, K) or tuple(lv_t.shape) != (n_img, K):
            raise ValueError('score and live must be [n_img, K]')
        out = torch.empty((n_img, K, 2), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_test_beam_select(self.h, _ptr(lp_t), _ptr(sc_t), _ptr(lv_t), n_img, K, V1, _ptr(out),
                                                 self._stream()), self.h, 'test_beam_select')
            torch.cuda.current_stream().synchronize()   # the inputs stay alive until the kernel has read them
        return out

    def decode_path(self, B=None, count=1):
        """'fused', 'split', 'coop', 'wide' or 'ln': the decode path an evaluate of `count` members would take ('wide': a
        model with rnn_size or input_encoding_size above 128, 'ln': a layer_n model, both whatever B and count)."""
        out = ctypes.c_int32()
        check(self.L.nicnes_decode_path(self.h, int(B or self.B), int(count), ctypes.byref(out)), self.h, 'decode_path')
        return ('fused', 'split', 'coop', 'wide', 'ln')[out.value]

    def test_ln_cell(self, x, h, c):
        """One layer-norm LSTM cell of theta itself on rows x [rows, E], h, c [rows, R] (rows <= 128) by the decode's
        device function (nicnes_test_ln_cell) -> (h', c') as numpy. No decode may run beside it."""
        xr, hr, cr = (self._dev(np.asarray(a, np.float32), torch.float32) for a in (x, h, c))
        rows = int(xr.shape[0])
        assert xr.shape == (rows, self.cfg.input_encoding_size)
        assert hr.shape == (rows, self.cfg.rnn_size) and cr.shape == hr.shape
        ho, co = torch.empty_like(hr), torch.empty_like(cr)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_test_ln_cell(self.h, _ptr(xr), _ptr(hr), _ptr(cr), rows, _ptr(ho), _ptr(co),
                                             self._stream()), self.h, 'test_ln_cell')
        torch.cuda.synchronize(self.device)
        return ho.cpu().numpy(), co.cpu().numpy()

    def decode_shape(self, B=None, count=1):
        """(G, slabs, S) an evaluate of `count` members would use."""
        out = (ctypes.c_int32 * 3)()
        check(self.L.nicnes_decode_shape(self.h, int(B or self.B), int(count), out), self.h, 'decode_shape')
        return tuple(int(v) for v in out)

    # ---------------------------------------------------------------- nic_es (nicnes_es_*) -----
    ES_TABLES = {'parents': 0, 'elites': 1}

    def es_create(self, max_parents, max_elites=1):
        """The ES state on this handle: two parent tables of max_parents rows and an elite table."""
        with torch.cuda.device(self.device):
            check(self.L.nicnes_es_create(self.h, int(max_parents), int(max_elites)), self.h, 'es_create')

    def es_free(self):
        check(self.L.nicnes_es_free(self.h), self.h, 'es_free')

    def es_set_mutation(self, mode='plain'):
        """'plain' or 'scale' (SM-PROPORTIONAL over each pair's own parent); anything else is not supported ('divide',
        which needs the parents' sensitivities, is es_set_mutation_divide)."""
        code = self.MUTATION_MODES[mode] if isinstance(mode, str) else int(mode)
        check(self.L.nicnes_es_set_mutation(self.h, code), self.h, 'es_set_mutation')

    def es_set_mutation_divide(self):
        """SM-G-SUM / SM-VECTOR: each pair's noise over its own parent's sensitivity (es_sensitivity, es_set_sensitivity).
        es_evaluate, es_offspring and es_advance then raise, before anything is enqueued, when a parent they name has
        no valid sensitivity. es_set_mutation('plain' / 'scale') leaves the mode."""
        check(self.L.nicnes_set_mutation_divide_es(self.h), self.h, 'es_set_mutation_divide')

    def es_sensitivity(self, slots, rows, underflow):
        """The SM-G-SUM sensitivity (sum_sensitivity's kernels, clamp included) of each parent slot named, on the first
        `rows` images of the batch held, into the handle's sensitivity table: one pass per slot, in order, on the
        current stream. The rows stay valid until es_set_parent (that slot) or es_advance (all of them)."""
        sl = self._host_i32(slots, len(slots), 'slots')
        with torch.cuda.device(self.device):
            check(self.L.nicnes_sensitivity_es(self.h, sl.ctypes.data_as(ctypes.c_void_p), int(sl.size), int(rows),
                                               ctypes.c_float(underflow), self._stream()), self.h, 'es_sensitivity')

    def es_set_sensitivity(self, vec, slot=None):
        """slot None: `vec` [D] is the one sensitivity every parent shares (SM-VECTOR; it stays valid over advances).
        slot >= 0: that parent's row (tests, resuming)."""
        t = self._dev(vec, torch.float32)
        if t.numel() != self.D:
            raise ValueError('a sensitivity needs D entries')
        with torch.cuda.device(self.device):
            check(self.L.nicnes_set_sensitivity_es(self.h, -1 if slot is None else int(slot), _ptr(t), self._stream()),
                  self.h, 'es_set_sensitivity')
            torch.cuda.current_stream().synchronize()    # t stays alive until the copy has run

    def es_sensitivity_row(self, slot):
        """The sensitivity the divide mutation uses for parent `slot` (its row, or the shared vector): fp32 [D], GPU."""
        out = torch.empty(self.D, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_get_sensitivity_es(self.h, int(slot), _ptr(out), self._stream()), self.h,
                  'es_get_sensitivity')
        return out

    def es_set_parent(self, slot, theta):
        t = self._dev(theta, torch.float32)
        if t.numel() != self.D:
            raise ValueError('a parent needs D entries')
        with torch.cuda.device(self.device):
            check(self.L.nicnes_es_set_parent(self.h, int(slot), _ptr(t), self._stream()), self.h, 'es_set_parent')
            torch.cuda.current_stream().synchronize()    # t stays alive until the copy has run

    def es_set_parents(self, thetas):
        """Parent slots 0 .. len(thetas) - 1 and the parent count."""
        for i, t in enumerate(thetas):
            self.es_set_parent(i, t)
        self.es_set_parent_count(len(thetas))

    def es_set_parent_count(self, n):
        check(self.L.nicnes_es_set_parent_count(self.h, int(n)), self.h, 'es_set_parent_count')

    def es_row(self, slot, table='parents'):
        """Row `slot` of the current parent table or of the elite table: fp32 [D] on the GPU."""
        out = torch.empty(self.D, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_es_get_row(self.h, self.ES_TABLES[table], int(slot), _ptr(out), self._stream()), self.h,
                  'es_get_row')
        return out

    def es_row_stats(self, slot, table='parents'):
        """(fp32 mean|theta|, exact zeros) of a row, as SM-PROPORTIONAL uses them (synchronises)."""
        m, z = ctypes.c_float(), ctypes.c_int64()
        with torch.cuda.device(self.device):
            check(self.L.nicnes_es_row_stats(self.h, self.ES_TABLES[table], int(slot), ctypes.byref(m), ctypes.byref(z),
                                             self._stream()), self.h, 'es_row_stats')
        return np.float32(m.value), int(z.value)

    @staticmethod
    def _host_i32(a, n, what):
        a = np.ascontiguousarray(np.asarray(a, np.int32))
        if a.shape != (n,):
            raise ValueError('%s needs %d entries' % (what, n))
        return a

    def es_evaluate(self, generation, pair_begin, count, sigma, parent_of, fitness_out=None, return_seq=False,
                    return_lp=False, member_batch=None):
        """Fitness of the offspring of pairs [pair_begin, +count) of `generation`: [count, 2] fp64 on the GPU (offspring
        2k = parent_of[k] + delta'_k, 2k + 1 = parent_of[k] - delta'_k). parent_of: the parent slot of each pair of
        the slice (host ints). return_seq / return_lp / member_batch as evaluate()."""
        fit = fitness_out if fitness_out is not None else torch.empty((count, 2), dtype=torch.float64,
                                                                      device=self.device)
        shape = (count, 2, self.B, self.cfg.seq_length)
        seq = torch.empty(shape, dtype=torch.int32, device=self.device) if return_seq else None
        lp = torch.empty(shape, dtype=torch.float32, device=self.device) if return_lp else None
        po = self._host_i32(parent_of, count, 'parent_of')
        mb = self._host_i32(member_batch, count, 'member_batch') if member_batch is not None else None
        with torch.cuda.device(self.device):
            check(self.L.nicnes_es_evaluate(self.h, ctypes.c_uint64(generation), int(pair_begin), int(count),
                                            ctypes.c_float(sigma), po.ctypes.data_as(ctypes.c_void_p),
                                            mb.ctypes.data_as(ctypes.c_void_p) if mb is not None else None, _ptr(fit),
                                            _ptr(seq), _ptr(lp), self._stream()), self.h, 'es_evaluate')
        out = (fit,) + ((seq,) if return_seq else ()) + ((lp,) if return_lp else ())
        return out if len(out) > 1 else fit

    ES_DECODE_MODES = {'fused': 0, 'auto': 1, 'coop': 2}

    def es_set_decode(self, mode='fused', S=0):
        """The decode path of es_evaluate: 'fused' (the default), 'auto' (the coop path where the engine's shape rule
        picks 128-row slabs with S = 2 or 4 and the grid fits the GPU at once, else fused) or 'coop' with S = 2 or 4 (an
        evaluate that does not fit raises before anything is enqueued). Tokens do not depend on it."""
        code = self.ES_DECODE_MODES[mode] if isinstance(mode, str) else int(mode)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_set_decode_es(self.h, code, int(S)), self.h, 'es_set_decode')

    def es_decode_path(self, B=None, count=1):
        """'fused' or 'coop': the path an es_evaluate of `count` pairs would take under the current es_set_decode."""
        out = ctypes.c_int32()
        check(self.L.nicnes_decode_path_es(self.h, int(B or self.B), int(count), ctypes.byref(out)), self.h,
              'es_decode_path')
        return ('fused', 'split', 'coop')[out.value]

    def es_allgather_fitness(self, fit_local, n_pairs, fit_all=None):
        """fit_all [n_pairs, 2] in pair order <- every rank's shard fit_local [count, 2] of nicnes.es.es_shard, over the
        communicator of comm_init (shards may differ by one pair)."""
        if fit_all is None:
            fit_all = torch.empty((int(n_pairs), 2), dtype=torch.float64, device=self.device)
        assert fit_local.dtype == torch.float64 and fit_local.is_contiguous() and fit_all.is_contiguous()
        with torch.cuda.device(self.device):
            check(self.L.nicnes_allgather_fitness_es(self.h, _ptr(fit_local), int(fit_local.shape[0]), int(n_pairs),
                                                     _ptr(fit_all), self._stream()), self.h, 'es_allgather_fitness')
        return fit_all

    def es_offspring(self, generation, pair, sign, sigma, parent):
        """fp32 theta [D] (GPU) of offspring (pair, sign: 0 +, 1 -) of `generation` over parent slot `parent`."""
        out = torch.empty(self.D, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_es_offspring(self.h, ctypes.c_uint64(generation), int(pair), int(sign),
                                             ctypes.c_float(sigma), int(parent), _ptr(out), self._stream()), self.h,
                  'es_offspring')
        return out

    def es_select(self, fitness, n_keep):
        """The first n_keep offspring ids (2 pair + sign) in descending fitness (ties to the lower id, NaN last):
        int32 [n_keep] on the GPU. fitness: any fp64 GPU tensor of n values ([pairs, 2] ravelled)."""
        f = fitness.reshape(-1)
        assert f.dtype == torch.float64 and f.is_contiguous()
        out = torch.empty(max(int(n_keep), 1), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_es_select(self.h, _ptr(f), int(f.numel()), int(n_keep), _ptr(out), self._stream()),
                  self.h, 'es_select')
        return out[:n_keep]

    def es_advance(self, generation, sigma, parent_of, order, n_front=0):
        """The next parents: elite rows [0, n_front) + the offspring `order` names (int32 GPU tensor, es_select's);
        parent_of: the parent slots of ALL pairs of the generation (host ints). The tables swap."""
        po = self._host_i32(parent_of, len(parent_of), 'parent_of')
        assert order.dtype == torch.int32 and order.is_contiguous()
        with torch.cuda.device(self.device):
            check(self.L.nicnes_es_advance(self.h, ctypes.c_uint64(generation), ctypes.c_float(sigma),
                                           po.ctypes.data_as(ctypes.c_void_p), int(po.size), _ptr(order),
                                           int(order.numel()), int(n_front), self._stream()), self.h, 'es_advance')

    def es_set_elite(self, elite_slot, slot, table='parents'):
        with torch.cuda.device(self.device):
            check(self.L.nicnes_es_set_elite(self.h, int(elite_slot), self.ES_TABLES[table], int(slot), self._stream()),
                  self.h, 'es_set_elite')

    def es_load_theta(self, slot, table='parents'):
        """The handle's theta <- a parent or elite row (device copy): Split.evaluate / evaluate_theta then score it."""
        with torch.cuda.device(self.device):
            check(self.L.nicnes_es_load_theta(self.h, self.ES_TABLES[table], int(slot), self._stream()), self.h,
                  'es_load_theta')

    # ---------------------------------------------------------------- multi-GPU (RCCL) ----------
    @staticmethod
    def comm_unique_id():
        """128-byte RCCL id, made by rank 0 and sent to the other ranks out of band."""
        buf = (ctypes.c_uint8 * _lib.COMM_ID_BYTES)()
        check(_lib.lib().nicnes_comm_unique_id(buf), None, 'comm_unique_id')
        return bytes(buf)

    def comm_init(self, nranks, rank, uid):
        """Join the RCCL communicator `uid` as `rank` of `nranks` (collective over the ranks)."""
        buf = (ctypes.c_uint8 * _lib.COMM_ID_BYTES).from_buffer_copy(uid)
        with torch.cuda.device(self.device):
            check(self.L.nicnes_comm_init(self.h, int(nranks), int(rank), buf), self.h, 'comm_init')
        self.comm_ranks = int(nranks)

    def comm_destroy(self):
        check(self.L.nicnes_comm_destroy(self.h), self.h, 'comm_destroy')
        self.comm_ranks = 1

    def comm_count(self):
        """(ranks, this rank) as RCCL reports them for the bound communicator ((1, 0) with none)."""
        n, r = ctypes.c_int32(), ctypes.c_int32()
        check(self.L.nicnes_comm_count(self.h, ctypes.byref(n), ctypes.byref(r)), self.h, 'comm_count')
        return int(n.value), int(r.value)

    def allgather_fitness(self, fit_local, fit_all):
        """fit_all [P_local * nranks, 2] <- every rank's fit_local [P_local, 2] (rank order)."""
        with torch.cuda.device(self.device):
            check(self.L.nicnes_allgather_fitness(self.h, _ptr(fit_local), int(fit_local.shape[0]), _ptr(fit_all),
                                                  self._stream()), self.h, 'allgather_fitness')
        return fit_all

    def allreduce_grad(self, gsum):
        """gsum [D] fp32 summed in place over the ranks."""
        with torch.cuda.device(self.device):
            check(self.L.nicnes_allreduce_grad(self.h, _ptr(gsum), self._stream()), self.h, 'allreduce_grad')
        return gsum

    def clear_faults(self):
        """Clear a contained decode fault (nicnes_clear_faults): returns the fault counters it found
        {'coop_timeouts', 'sample_slot_timeouts'}; the handle evaluates again afterwards."""
        out = (ctypes.c_int64 * 2)()
        with torch.cuda.device(self.device):
            check(self.L.nicnes_clear_faults(self.h, out), self.h, 'clear_faults')
        return {'coop_timeouts': int(out[0]), 'sample_slot_timeouts': int(out[1])}

    def stats(self):
        out = (ctypes.c_int64 * 8)()
        check(self.L.nicnes_stats(self.h, out), self.h, 'stats')
        sc = (ctypes.c_int64 * 2)()
        check(self.L.nicnes_screen_stats(self.h, sc), self.h, 'screen_stats')
        sr = (ctypes.c_int64 * 16)()
        check(self.L.nicnes_screen_reasons(self.h, sr), self.h, 'screen_reasons')
        d = {'tie_fallbacks': out[0], 'sample_stage_fallbacks': out[1], 'coop_timeouts': out[2],
             'sample_slot_timeouts': out[3], 'screen_candidates': sc[0], 'screen_fallback_rows': sc[1],
             'screen_rows_over_cap': sr[0], 'screen_rows_undecided': sr[1], 'screen_rows_evicted': sr[2],
             'screen_rows_nonfinite': sr[3], 'screen_rows_settled_later': sr[4], 'screen_resweep_rows': sr[5],
             'screen_resweep_steps': sr[6], 'screen_resweep_waves': sr[15],
             'queue_steps': out[4], 'queue_timeouts': out[5], 'queue_finished': out[6], 'queue_pending': out[7]}
        # over-cap rows by the certify rounds their fuller lane needs at least (the last: 9 or more); plain integers,
        # so that callers can subtract two stats() key by key
        d.update({'screen_over_cap_rounds_%d' % (k + 2): sr[7 + k] for k in range(8)})
        return d


METRIC_KEYS = ('Bleu_1', 'Bleu_2', 'Bleu_3', 'Bleu_4', 'ROUGE_L', 'CIDEr')   # COCOEvalCap's keys (no java scorers)


class Split:
    """N images held on the GPU for validation: one-call greedy decode of theta and COCOEvalCap's BLEU / ROUGE_L /
    CIDEr on the label rows (nicnes_split_*; Engine.make_split)."""

    def __init__(self, engine, fc, gts=None, df=None, ref_len_raw=None):
        from .validation import corpus_df
        e = self.engine = engine
        T = e.cfg.seq_length
        fc_np = fc.detach().cpu().numpy() if isinstance(fc, torch.Tensor) else np.asarray(fc)
        fc_np = np.ascontiguousarray(fc_np, np.float32)
        if fc_np.ndim != 2 or fc_np.shape[1] != e.cfg.fc_feat_size or fc_np.shape[0] < 1:
            raise ValueError('fc must be [N >= 1, fc_feat_size]')
        self.N = int(fc_np.shape[0])
        self.has_refs = gts is not None
        refs_np = np.zeros((0, T), np.int32)
        start = np.zeros(self.N + 1, np.int32)
        keys = np.zeros(0, np.uint64)
        vals = np.zeros(0, np.float64)
        ref_len_log = 0.0
        if self.has_refs:
            if len(gts) != self.N:
                raise ValueError('gts has %d images, fc has %d rows' % (len(gts), self.N))
            rows = [np.asarray(g, np.int32).reshape(-1, T) for g in gts]
            start = np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])]).astype(np.int32)
            refs_np = np.ascontiguousarray(np.concatenate(rows, 0))
            self._row_start = start
            # as set_batches: an id outside the vocabulary would alias another word in the 14-bit key fields
            if refs_np.size and (refs_np.min() < 0 or refs_np.max() > e.cfg.vocab_size):
                raise ValueError('reference token outside [0, vocab_size = %d]: min %d, max %d'
                                 % (e.cfg.vocab_size, refs_np.min(), refs_np.max()))
            if df is None:
                keys, vals = corpus_df(rows, T)
                ref_len_raw = self.N if ref_len_raw is None else ref_len_raw
            elif isinstance(df, dict):
                keys, vals = df_table_arrays(df)
            else:
                keys, vals = np.asarray(df[0], np.uint64), np.asarray(df[1], np.float64)
            if ref_len_raw is None:
                raise ValueError('a given df table needs its ref_len_raw')
            ref_len_log = float(np.log(float(ref_len_raw)))
        keys = np.ascontiguousarray(keys, np.uint64)
        vals = np.ascontiguousarray(vals, np.float64)
        sp = ctypes.c_void_p()
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)     # noqa: E731  (host arrays: the call copies them)
        with torch.cuda.device(e.device):
            check(e.L.nicnes_split_create(e.h, vp(fc_np), self.N, vp(refs_np), int(refs_np.shape[0]), vp(start),
                                          vp(keys), vp(vals), int(keys.size), ref_len_log, ctypes.byref(sp),
                                          e._stream()), e.h, 'split_create')
        self.sp = sp

    def close(self):
        if getattr(self, 'sp', None) and getattr(self.engine, 'h', None):
            self.engine.L.nicnes_split_destroy(self.engine.h, self.sp)
        self.sp = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _range(self, first, count):
        first = int(first)
        count = self.N - first if count is None else int(count)
        if first < 0 or count < 1 or first + count > self.N:
            raise ValueError('range [%d, %d) outside the split\'s %d images' % (first, first + count, self.N))
        return first, count

    def decode(self, first=0, count=None, return_lp=False):
        """Greedy tokens [count, T] int32 of the engine's current theta on images [first, first + count), in one
        enqueue; return_lp adds each token's log-prob (0 after a row's end token)."""
        e = self.engine
        first, count = self._range(first, count)
        seq = torch.empty((count, e.cfg.seq_length), dtype=torch.int32, device=e.device)
        lp = torch.empty((count, e.cfg.seq_length), dtype=torch.float32, device=e.device) if return_lp else None
        with torch.cuda.device(e.device):
            check(e.L.nicnes_split_decode(e.h, self.sp, first, count, _ptr(seq), _ptr(lp), e._stream()), e.h,
                  'split_decode')
        return (seq, lp) if return_lp else seq

    @staticmethod
    def _beam(beam_size):
        beam = int(beam_size)
        if beam < 1 or beam > 8:
            raise ValueError('beam_size must be in 1..8, got %r' % (beam_size,))
        return beam

    def decode_beam(self, first=0, count=None, beam_size=3, return_score=False):
        """Beam-search tokens [count, T] int32 (zero-padded) of the engine's current theta on images [first, first +
        count), in one enqueue: the finished hypothesis with the largest sum of log-probs, beam_size in 1..8, NO
        length normalisation (nicnes_split_decode_beam). return_score adds that sum, [count] fp64. beam_size = 1 is
        the greedy decode."""
        e = self.engine
        beam = self._beam(beam_size)
        first, count = self._range(first, count)
        seq = torch.empty((count, e.cfg.seq_length), dtype=torch.int32, device=e.device)
        score = torch.empty(count, dtype=torch.float64, device=e.device) if return_score else None
        with torch.cuda.device(e.device):
            check(e.L.nicnes_split_decode_beam(e.h, self.sp, first, count, beam, _ptr(seq), _ptr(score), e._stream()),
                  e.h, 'split_decode_beam')
        return (seq, score) if return_score else seq

    def xent(self, first=0, count=None):
        """The teacher-forced cross-entropy of the engine's current theta on the label rows of images [first, first +
        count) (nicnes_split_xent; the definition is NICNES_FITNESS_XENT's): {'loss': the per-token mean of -log p,
        'perplexity': exp(loss), 'tokens': the targets counted (each row's words plus one end token), 'lp_sum' [rows]
        fp64 and 'n_tok' [rows] int32 per label row, tensors on the GPU}. One enqueue, then one read-back of the three
        scalars; the fitness mode, df table, batches and mutation stay as they are."""
        e = self.engine
        first, count = self._range(first, count)
        rows = int(self._row_start[first + count] - self._row_start[first]) if self.has_refs else 0
        out2 = torch.empty(2, dtype=torch.float64, device=e.device)
        tok = torch.empty(1, dtype=torch.int64, device=e.device)
        lp = torch.empty(rows, dtype=torch.float64, device=e.device)
        nt = torch.empty(rows, dtype=torch.int32, device=e.device)
        with torch.cuda.device(e.device):
            check(e.L.nicnes_split_xent(e.h, self.sp, first, count, _ptr(out2), _ptr(tok), _ptr(lp), _ptr(nt),
                                        e._stream()), e.h, 'split_xent')
        o = out2.cpu().numpy()
        return {'loss': float(o[0]), 'perplexity': float(o[1]), 'tokens': int(tok.item()), 'lp_sum': lp, 'n_tok': nt}

    def _outputs(self, count, rows):
        e = self.engine
        return (torch.empty(10, dtype=torch.int64, device=e.device), torch.empty(6, dtype=torch.float64, device=e.device),
                torch.empty(count, dtype=torch.float64, device=e.device) if rows else None)

    @staticmethod
    def _result(totals, metrics, rows, detail):
        m = metrics.cpu().numpy()
        out = {k: float(v) for k, v in zip(METRIC_KEYS, m)}
        if not detail:
            return out
        return out, totals.cpu().numpy(), (rows.cpu().numpy() if rows is not None else None)

    def score(self, seq, first=0, detail=False):
        """The metrics of GIVEN token rows seq [count, T] as the captions of images [first, first + count):
        {'Bleu_1'..'Bleu_4', 'ROUGE_L', 'CIDEr'}; detail=True adds the ten BLEU totals (int64: correct[1..4],
        guess[1..4], testlen, reflen) and every image's CIDEr-D."""
        e = self.engine
        sq = e._dev(seq, torch.int32)
        if sq.dim() != 2 or sq.shape[1] != e.cfg.seq_length:
            raise ValueError('seq must be [count, seq_length]')
        if sq.numel() and (int(sq.min()) < 0 or int(sq.max()) > e.cfg.vocab_size):
            raise ValueError('token outside [0, vocab_size = %d]' % e.cfg.vocab_size)
        first, count = self._range(first, int(sq.shape[0]))
        totals, metrics, rows = self._outputs(count, detail)
        with torch.cuda.device(e.device):
            check(e.L.nicnes_split_score(e.h, self.sp, first, count, _ptr(sq), _ptr(totals), _ptr(metrics), _ptr(rows),
                                         e._stream()), e.h, 'split_score')
            torch.cuda.current_stream().synchronize()    # sq stays alive until the kernels have read it
        return self._result(totals, metrics, rows, detail)

    def evaluate(self, first=0, count=None, detail=False, return_seq=False, beam_size=None):
        """decode + score in one call: COCOEvalCap's dict for the engine's current theta on the split. beam_size
        (1..8) decodes with decode_beam instead of greedily; None is the greedy path itself."""
        e = self.engine
        beam = None if beam_size is None else self._beam(beam_size)
        first, count = self._range(first, count)
        totals, metrics, rows = self._outputs(count, detail)
        seq = torch.empty((count, e.cfg.seq_length), dtype=torch.int32, device=e.device) if return_seq else None
        with torch.cuda.device(e.device):
            if beam is None:
                check(e.L.nicnes_split_evaluate(e.h, self.sp, first, count, _ptr(totals), _ptr(metrics), _ptr(rows),
                                                _ptr(seq), e._stream()), e.h, 'split_evaluate')
            else:
                check(e.L.nicnes_split_evaluate_beam(e.h, self.sp, first, count, beam, _ptr(totals), _ptr(metrics),
                                                     _ptr(rows), _ptr(seq), e._stream()), e.h, 'split_evaluate_beam')
        res = self._result(totals, metrics, rows, detail)
        return (res, seq) if return_seq else res


class TrainSet:
    """The training split's fc rows and label rows held on the GPU (nicnes_trainset_*; Engine.make_trainset):
    Engine.draw_batches gathers an iteration's batches from it by image index."""

    CHUNK_ROWS = 4096      # rows of one upload (32 MB at F = 2048)

    def __init__(self, engine, fc, gts, fc_rows=None):
        e = self.engine = engine
        T, F = e.cfg.seq_length, e.cfg.fc_feat_size
        if tuple(fc.shape[1:]) != (F,) or fc.shape[0] < 1:
            raise ValueError('fc must be [N >= 1, fc_feat_size]')
        self.N = int(fc.shape[0])
        if len(gts) != self.N:
            raise ValueError('gts has %d images, fc has %d rows' % (len(gts), self.N))
        rows = [np.asarray(g, np.int32).reshape(-1, T) for g in gts]
        self.counts = np.array([r.shape[0] for r in rows], np.int32)
        start = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int32)
        refs_np = np.ascontiguousarray(np.concatenate(rows, 0))
        self._rows = fc_rows
        fc_t = None
        if isinstance(fc, torch.Tensor):       # the caller's tensor is copied: it holds the rows a second time
            fc_t = fc.to(device=e.device, dtype=torch.float32).contiguous()
        elif fc_rows is None:
            self._rows = lambda ix, a=fc: np.asarray(a[np.asarray(ix, np.int64)], np.float32)
        ts = ctypes.c_void_p()
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)     # noqa: E731  (host arrays: the call copies them)
        with torch.cuda.device(e.device):
            torch.cuda.current_stream().synchronize()
            check(e.L.nicnes_trainset_create(e.h, _ptr(fc_t), self.N, vp(refs_np), int(refs_np.shape[0]), vp(start),
                                             ctypes.byref(ts), e._stream()), e.h, 'trainset_create')
            self.ts = ts
            # host rows go straight into the set's own buffer, a chunk at a time: the split is never whole on the
            # host, and never twice on the device
            for c0 in range(0, self.N if fc_t is None else 0, self.CHUNK_ROWS):
                part = np.ascontiguousarray(fc[c0:c0 + self.CHUNK_ROWS], np.float32)
                check(e.L.nicnes_trainset_write_fc(e.h, ts, c0, int(part.shape[0]), vp(part), e._stream()), e.h,
                      'trainset_write_fc')

    def fc_rows(self, image_ix):
        """Host fc rows [len(image_ix), F] fp32 of images of the set, read on demand from the source given at creation."""
        if self._rows is None:
            raise ValueError('this training set was made without a host source of its fc rows')
        return np.ascontiguousarray(self._rows(np.asarray(image_ix, np.int64)), np.float32)

    def close(self):
        if getattr(self, 'ts', None) and getattr(self.engine, 'h', None):
            self.engine.L.nicnes_trainset_destroy(self.engine.h, self.ts)
        self.ts = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
