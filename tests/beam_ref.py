"""Host restatement of the beam-search decode's definition (include/nicnes.h nicnes_split_decode_beam, DESIGN.md
"Beam-search decode") -- TEST INFRASTRUCTURE ONLY.

The dense products are oracle.gemv (fp32 fma chains from the bias in nn_kperm order) and the activations
oracle.vec_math, taken in the order of the oracle's decode_core, so the chains are the oracle's bit for bit. The
log-softmax is lp[v] = fl32(fl32(x_v - m) - lse) with lse = fl32(log(sum exp((double)fl32(x_v - m)))): an fp64 exp-sum
rounded once. Scores are fp64: score_b + (double)lp_b[v], one addition. No length normalisation.

select() is the definition's step rule on given log-prob rows; beam_search() runs it from an image to the result and
reports what the tests need to know about the image: whether it is fragile, whether its winner finished after another
hypothesis had finished and whether it reached step T. It stops an image where the definition allows a kernel to (the
best finished score is >= every live one), and also calls the image fragile where that comparison is within the gap.

The shared workloads of tests/test_beam_ref.py (CPU: the inputs are not vacuous, at most FRAGILE_CAP fragile) and
tests/test_gpu_beam.py (GPU: tokens and scores) are defined here and computed once per process."""
import functools

import numpy as np

from oracle import oracle as O

# Two candidates (or two finished scores) closer than this may swap between two correct implementations: the project's
# bar on a log-prob is 1e-5 per step (tests/test_gpu_reference.py), on both sides, accumulated over at most 16 steps:
# 2 x 16 x 1e-5.
FRAGILE_GAP = 3.2e-4
SCORE_TOL = 16 * 1e-5


class Model:
    def __init__(self, dims, theta):
        self.dims = dims
        th = np.ascontiguousarray(theta, np.float32)
        off = dims.offsets()

        def get(name):
            o, shp = off[name]
            return th[o:o + int(np.prod(shp))].reshape(shp)
        self.Wimg, self.bimg = get('img_embed.weight'), get('img_embed.bias')
        self.emb = get('embed.weight')
        self.Wl, self.bl = get('logit.weight'), get('logit.bias')
        self.Wi, self.bi = get('core.i2h.weight'), get('core.i2h.bias')
        self.Wh, self.bh = get('core.h2h.weight'), get('core.h2h.bias')

    def cell(self, x, h, c):
        """LSTMCore.forward as decode_core restates it: (b_i2h + Wi.x) + (b_h2h + Wh.h), then nn_lstm_cell."""
        R = self.dims.R
        s = O.gemv(self.Wi, self.bi, x) + O.gemv(self.Wh, self.bh, h)
        ig = O.vec_math('sigmoid', s[0:R])
        fg = O.vec_math('sigmoid', s[R:2 * R])
        og = O.vec_math('sigmoid', s[2 * R:3 * R])
        g = np.maximum(s[3 * R:4 * R], s[4 * R:5 * R])
        cn = fg * c + ig * g                       # fp32 arrays: every product and the sum rounded on its own
        return og * O.vec_math('tanh', cn), cn

    def start(self, fc_row):
        """the image step and the BOS step (FCModel._sample t = 0, t = 1): the root's (h, c)"""
        R = self.dims.R
        h, c = np.zeros(R, np.float32), np.zeros(R, np.float32)
        h, c = self.cell(O.gemv(self.Wimg, self.bimg, fc_row), h, c)
        return self.cell(self.emb[0], h, c)

    def logprobs(self, h):
        x = O.gemv(self.Wl, self.bl, h)
        d = x - x.max()                            # fp32
        lse = np.float32(np.log(np.exp(d.astype(np.float64)).sum()))
        return d - lse                             # fp32


def select(lp_rows, scores, live, K):
    """The step rule on given rows: lp_rows [n, V1] fp32, scores [n] fp64, live [n] bool. Returns the ordered
    candidates [(score, b, v)], the first min(K, candidates) of which are selected, with one more (the K + 1-th) kept
    for the fragility rule."""
    cand = []
    for b in range(len(scores)):
        if not live[b]:
            continue
        lp = np.asarray(lp_rows[b], np.float32)
        order = np.argsort(-lp.astype(np.float64), kind='stable')[:K + 1]     # (lp descending, v ascending)
        cand += [(float(np.float64(scores[b]) + np.float64(lp[v])), b, int(v)) for v in order]
    cand.sort(key=lambda t: (-t[0], t[1], t[2]))
    return cand[:K + 1]


def close_neighbours(cand, gap=FRAGILE_GAP):
    return any(cand[i][0] - cand[i + 1][0] < gap for i in range(len(cand) - 1))


def run_steps(K, T, step_lp, advance):
    """The definition from the root to the result over abstract hypotheses. step_lp(state) -> log-prob row;
    advance(state, v) -> the state after word v. `root` state is advance(None, None). Returns a dict: tokens, score,
    fragile, late_winner (the winner finished after another hypothesis had finished), reached_T, finished (every
    finished hypothesis as (score, step, order, tokens))."""
    live = [(advance(None, None), [], 0.0)]
    finished = []
    fragile = False
    for s in range(1, T + 1):
        if not live:
            break
        rows = [step_lp(st) for st, _, _ in live]
        cand = select(rows, [sc for _, _, sc in live], [True] * len(live), K)
        fragile |= close_neighbours(cand)
        nxt = []
        for order, (sc, b, v) in enumerate(cand[:K]):
            st, toks, _ = live[b]
            if v == 0:
                finished.append((sc, s, order, toks + [0] * (T - len(toks))))
            elif s == T:
                finished.append((sc, s, order, toks + [v]))
            else:
                nxt.append((b, v, sc))
        if finished and nxt:
            # the stop the definition allows (and the kernel takes): nothing live can still beat the best finished one.
            # Where the two scores are within the gap, two correct implementations may stop at different steps.
            lead = max(f[0] for f in finished) - nxt[0][2]          # nxt[0]: the first live selection, the largest
            fragile |= abs(lead) < FRAGILE_GAP
            if lead >= 0:
                break
        live = [(advance(live[b][0], v), live[b][1] + [v], sc) for b, v, sc in nxt]
    ranked = sorted(finished, key=lambda f: (-f[0], f[1], f[2]))
    best = ranked[0]
    if len(ranked) > 1 and ranked[0][0] - ranked[1][0] < FRAGILE_GAP:
        fragile = True
    return {'tokens': np.asarray(best[3], np.int32), 'score': best[0], 'fragile': fragile,
            'late_winner': any(f[1] < best[1] for f in finished), 'reached_T': best[1] == T and best[3][T - 1] != 0,
            'finished': finished}


def beam_search(model, fc_row, K):
    def advance(state, v):
        if state is None:
            return model.start(np.ascontiguousarray(fc_row, np.float32))
        h, c = state
        return model.cell(model.emb[v], h, c)
    return run_steps(K, model.dims.T, lambda st: model.logprobs(st[0]), advance)


def table_search(tables, K, T):
    """run_steps over a hand-made log-prob table: tables(prefix tuple) -> log-prob row"""
    return run_steps(K, T, lambda st: np.asarray(tables(st), np.float32),
                     lambda st, v: () if st is None else st + (v,))


# ------------------------------------------------------------------ the shared workloads -----------------------------
# A case is (K, first, count): count images from `first` decoded at width K. Counts 1, 7, 33 and one past an 8-wave
# workgroup's images (8 floor(32 / K) + 1), first > 0. At most FRAGILE_CAP of a case's images may be fragile
# (tests/test_beam_ref.py checks it on the CPU, every case on its own): a condition on the inputs. Change a seed or
# theta's gain and biases, never the cap.
FRAGILE_CAP = 0.10          # the project's cap (tests/test_gpu_es.py)

# theta: O.make_theta(seed, gain, bias_std), then end_bias added to the end token's logit bias. 'end_logit' instead
# builds the end token: its logit row is zeroed and its bias set, so its logit is that constant in every state, and
# the other logit rows are scaled by 'logit_scale' so that the best word stays far above the rest. At full size that
# gives images where the end token is taken second or third at an early step while the leading hypothesis goes on
# cheaply and wins later (a random logit row at V1 = 9,488 is almost never among the three best).
END_LOGIT_FULL = 23.44       # 8 below the median best logit of the full workload's images at step 1 (31.44)
WORKLOADS = {
    'v8': dict(V=7, F=128, T=16, tseed=21, gain=6.0, bias_std=0.5, end_bias=0.0, fseed=900, N=40,
               cases=[(1, 0, 33), (2, 3, 7), (3, 0, 33), (5, 1, 7), (8, 0, 33)]),
    'v68_t3': dict(V=67, F=128, T=3, tseed=12, gain=6.0, bias_std=0.5, end_bias=1.0, fseed=901, N=40,
                   cases=[(1, 2, 1), (2, 0, 33), (3, 0, 33), (5, 0, 33), (8, 4, 7)]),
    'v128': dict(V=127, F=128, T=16, tseed=13, gain=6.0, bias_std=0.5, end_bias=2.0, fseed=902, N=260,
                 cases=[(1, 3, 257), (2, 1, 129), (3, 2, 81), (5, 5, 49), (8, 7, 33), (3, 0, 1)]),
    'v128_t1': dict(V=127, F=128, T=1, tseed=14, gain=6.0, bias_std=0.5, end_bias=0.0, fseed=903, N=40,
                    cases=[(1, 0, 7), (3, 1, 33), (8, 0, 33)]),
    'full': dict(V=9487, F=2048, T=16, tseed=15, gain=4.0, bias_std=0.1, logit_scale=30.0, end_logit=END_LOGIT_FULL,
                 fseed=904, N=40, cases=[(3, 1, 33)]),
}


def workload_inputs(name):
    w = WORKLOADS[name]
    dims = O.Dims(vocab_size=w['V'], F=w['F'], T=w['T'])
    theta = O.make_theta(dims, w['tseed'], w['gain'], w['bias_std'])
    off = dims.offsets()
    if 'end_logit' in w:
        o = off['logit.weight'][0]
        theta[o:o + dims.V1 * dims.R] *= np.float32(w['logit_scale'])
        theta[o:o + dims.R] = 0
        theta[off['logit.bias'][0]] = np.float32(w['end_logit'])
    else:
        theta[off['logit.bias'][0]] += np.float32(w['end_bias'])
    fc = np.random.Generator(np.random.PCG64(w['fseed'])).standard_normal((w['N'], w['F'])).astype(np.float32)
    return dims, theta, fc, w['cases']


@functools.lru_cache(maxsize=None)
def workload(name):
    """(dims, theta, fc, cases, ref) with ref[(K, image)] = beam_search's dict for every image a case decodes"""
    dims, theta, fc, cases = workload_inputs(name)
    model = Model(dims, theta)
    ref = {}
    for K, first, count in cases:
        for i in range(first, first + count):
            if (K, i) not in ref:
                ref[(K, i)] = beam_search(model, fc[i], K)
    return dims, theta, fc, cases, ref
