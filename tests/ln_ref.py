"""Host restatement of the layer-norm greedy decode (include/nicnes.h nicnes_config.layer_n, DESIGN.md "Layer-norm
models") -- TEST INFRASTRUCTURE ONLY.

The dense products are oracle.gemv (fp32 fma chains from the bias in nn_kperm order, one chain per product) and the
activations oracle.vec_math, taken in the order of the oracle's decode_core. With the normalisation switched off the
decode is the oracle's bit for bit (tests/test_layernorm_host.py), which pins this restatement to it.

The normalisation is include/nicnes_math.h's (nn_ln_*), in numpy float32, every operation rounded on its own. The N
values of a batch row sit in two lanes: lane half hh owns unit u when ((u >> 2) & 1) == hh. Per lane the values are
summed sequentially in ascending unit order from 0; the two lane sums are added once; mean = total / float32(N);
d = a - mean; per lane the sequential sum of d * d in the same order, the two added; var = that / float32(N);
den = sqrt(var + 1e-5); y = d / den; with affine y * gamma + beta as a rounded product then a rounded sum.

The greedy pick and its fragile flag follow greedy_pick of oracle/nicnes_oracle.c: an fp64 exp-sum in ascending id
order rounded once to fp32, the first id whose log-prob equals the maximum, fragile when moving the lse by +-1 or 2 ulp
changes that id.

A flat theta holds the nine tensors of oracle.Dims.shapes(), or those and the six layer-norm tensors behind them
(LN_NAMES, the reference's registration order): Model takes either."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import oracle as O

LN_NAMES = ['core.i2h_ln.weight', 'core.i2h_ln.bias', 'core.h2h_ln.weight', 'core.h2h_ln.bias',
            'core.c_ln.weight', 'core.c_ln.bias']
F32 = np.float32
EPS = F32(1e-5)
_pool = ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))     # oracle.gemv releases the GIL


def tail_size(R):
    return 22 * R


def tail_offsets(dims):
    """offsets of the six tail tensors + the affine D (nicnes_param_offsets_ln)"""
    R, o, out = dims.R, dims.D, []
    for name in LN_NAMES:
        out.append(o)
        o += R if '.c_ln.' in name else 5 * R
    return out + [o]


def make_tail(R, seed=None, scale=0.1):
    """the tail of a fresh theta (weight 1, bias 0), or gamma = 1 + scale z, beta = scale z in registration order"""
    rng = np.random.Generator(np.random.PCG64(seed)) if seed is not None else None
    parts = []
    for name in LN_NAMES:
        n = R if '.c_ln.' in name else 5 * R
        base = F32(1.0) if name.endswith('weight') else F32(0.0)
        z = rng.standard_normal(n).astype(F32) * F32(scale) if rng is not None else np.zeros(n, F32)
        parts.append((base + z).astype(F32))
    return np.concatenate(parts)


def lane_sum(a, half):
    """[rows, N] -> the sequential fp32 sum, from 0, of lane half `half`'s values of each row in ascending unit order"""
    u = np.arange(a.shape[1])
    v = a[:, ((u >> 2) & 1) == half]
    z = np.zeros((a.shape[0], 1), F32)
    return np.add.accumulate(np.concatenate([z, v], 1), axis=1, dtype=F32)[:, -1]


def layer_norm(a, gamma=None, beta=None):
    """nn.LayerNorm over the last axis of a [rows, N] in the engine's arithmetic"""
    a = np.ascontiguousarray(a, F32)
    n = F32(a.shape[1])
    mean = ((lane_sum(a, 0) + lane_sum(a, 1)) / n).astype(F32)
    d = (a - mean[:, None]).astype(F32)
    dd = (d * d).astype(F32)
    var = ((lane_sum(dd, 0) + lane_sum(dd, 1)) / n).astype(F32)
    den = np.sqrt((var + EPS).astype(F32)).astype(F32)
    y = (d / den[:, None]).astype(F32)
    if gamma is not None:
        y = ((y * gamma[None, :]).astype(F32) + beta[None, :]).astype(F32)
    return y


def greedy_pick(logits):
    """greedy_pick of oracle/nicnes_oracle.c on one row -> (token, log-prob, fragile)"""
    logits = np.asarray(logits, F32)
    m = logits.max()
    d = (logits - m).astype(F32)
    s = np.add.accumulate(np.exp(d.astype(np.float64)))[-1]               # ascending ids, fp64
    lse = F32(np.log(s))
    best = F32(-lse)
    hit = np.flatnonzero((d - lse).astype(F32) == best)
    tok = int(hit[0]) if hit.size else -1
    near = d >= F32(-1e-5)
    up1 = np.nextafter(lse, F32(np.inf)); up2 = np.nextafter(up1, F32(np.inf))
    dn1 = np.nextafter(lse, F32(-np.inf)); dn2 = np.nextafter(dn1, F32(-np.inf))
    fragile = 0
    for l2 in (up1, up2, dn1, dn2):
        h2 = np.flatnonzero(near & ((d - l2).astype(F32) == F32(-l2)))
        if (int(h2[0]) if h2.size else -1) != tok:
            fragile = 1
    return tok, best, fragile


class Model:
    """dims: oracle.Dims. theta: flat fp32 [dims.D] or [dims.D + 22 R]. layer_n False: the oracle's cell."""

    def __init__(self, dims, theta, layer_n=True):
        self.dims, self.layer_n = dims, layer_n
        th = np.ascontiguousarray(theta, F32)
        if th.size not in (dims.D, dims.D + tail_size(dims.R)):
            raise ValueError('theta has %d entries, expected %d or %d' % (th.size, dims.D, dims.D + tail_size(dims.R)))
        self.affine = th.size != dims.D
        if self.affine and not layer_n:
            raise ValueError('a theta with the layer-norm tail needs layer_n')
        off = dims.offsets()

        def get(name):
            o, shp = off[name]
            return th[o:o + int(np.prod(shp))].reshape(shp)
        self.Wimg, self.bimg = get('img_embed.weight'), get('img_embed.bias')
        self.emb = get('embed.weight')
        self.Wl, self.bl = get('logit.weight'), get('logit.bias')
        self.Wi, self.bi = get('core.i2h.weight'), get('core.i2h.bias')
        self.Wh, self.bh = get('core.h2h.weight'), get('core.h2h.bias')
        self.ln = [None] * 6
        if self.affine:
            to = tail_offsets(dims)
            self.ln = [th[to[i]:to[i + 1]] for i in range(6)]

    @staticmethod
    def product(W, b, X):
        """rows of X through one chain each"""
        return np.stack(list(_pool.map(lambda x: O.gemv(W, b, x), X)))

    def cell(self, x, h, c):
        """LSTMCore.forward (nets.py:98-134) on rows x [n, E], h, c [n, R] -> (h', c')"""
        R = self.dims.R
        si, sh = self.product(self.Wi, self.bi, x), self.product(self.Wh, self.bh, h)
        if self.layer_n:
            si, sh = layer_norm(si, self.ln[0], self.ln[1]), layer_norm(sh, self.ln[2], self.ln[3])
        s = (si + sh).astype(F32)
        sig = O.vec_math('sigmoid', s[:, :3 * R])
        ig, fg, og = sig[:, :R], sig[:, R:2 * R], sig[:, 2 * R:]
        g1, g2 = s[:, 3 * R:4 * R], s[:, 4 * R:]
        g = np.where(g1 > g2, g1, g2)
        cn = ((fg * c).astype(F32) + (ig * g).astype(F32)).astype(F32)
        act = layer_norm(cn, self.ln[4], self.ln[5]) if self.layer_n else cn
        return (og * O.vec_math('tanh', act)).astype(F32), cn

    def decode(self, fc):
        """Greedy decode of the rows of fc [B, F] -> (seq int32 [B, T], lp f32 [B, T], fragile u8 [B, T]), as
        oracle.decode reports them (lp and fragile 0 after the step at which every row has finished)."""
        d = self.dims
        fc = np.ascontiguousarray(fc, F32)
        B, T = fc.shape[0], d.T
        seq, lp, fr = np.zeros((B, T), np.int32), np.zeros((B, T), F32), np.zeros((B, T), np.uint8)
        h, c = np.zeros((B, d.R), F32), np.zeros((B, d.R), F32)
        h, c = self.cell(self.product(self.Wimg, self.bimg, fc), h, c)
        it = np.zeros(B, np.int64)
        unfinished = np.ones(B, bool)
        last = T
        for t in range(1, T + 1):
            h, c = self.cell(self.emb[it], h, c)
            logits = self.product(self.Wl, self.bl, h)
            picks = list(_pool.map(greedy_pick, logits))
            tok = np.array([p[0] for p in picks], np.int64)
            unfinished = unfinished & (tok > 0)
            it = tok * unfinished
            seq[:, t - 1] = it
            lp[:, t - 1] = [p[1] for p in picks]
            fr[:, t - 1] = [p[2] for p in picks]
            if not unfinished.any():
                last = t
                break
        lp[:, last:] = 0
        fr[:, last:] = 0
        return seq, lp, fr
