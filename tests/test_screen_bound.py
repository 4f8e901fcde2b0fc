"""The bf16 screening bound of include/nicnes_math.h (nn_screen_eps / nn_screen_norm), CPU only.

A screened logit is the logit sum taken with both operands rounded to bf16 and accumulated in fp32 in an order
the matrix core does not document; nn_screen_eps must bound its distance from the engine's exact logit, the fp32
fmaf chain in nn_kperm order. Here the header is compiled into a small host helper with the system compiler, bf16
rounding is emulated in numpy, and the bound is checked on the bench theta, on the trained-like theta (gain 4,
bias std 0.1) and on adversarial rows, under three accumulation models (one fp64 sum rounded once, a sequential
fp32 sum truncated at every add, and that with subnormal operands flushed). The candidate rule of a screened decode
(every id with l~ >= m~ - 2 eps - hu_out) must then keep every id of the fp32 tie window."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CC = shutil.which('cc') or shutil.which('gcc')

HELPER = r'''
#include "nicnes_math.h"
float screen_eps(float hn, float wn, float babs, float scale) { return nn_screen_eps(hn, wn, babs, scale); }
float screen_norm(float ss) { return nn_screen_norm(ss); }
/* the engine's logit: acc = fmaf(w[k], h[k], acc) from the bias, k in nn_kperm order */
void chain_logits(const float* w, const float* b, const float* h, int V, float* out) {
    for (int v = 0; v < V; ++v) {
        float acc = b[v];
        for (int pos = 0; pos < 128; ++pos) { int k = nn_kperm(pos); acc = fmaf(w[128 * v + k], h[k], acc); }
        out[v] = acc;
    }
}
/* worst accumulation model: every product (exact: operands hold 8 significant bits) added in turn, each sum
 * truncated toward zero to fp32 */
void trunc_logits(const float* w, const float* b, const float* h, int V, float* out) {
    for (int v = 0; v < V; ++v) {
        float acc = b[v];
        for (int k = 0; k < 128; ++k) {
            double s = (double)acc + (double)w[128 * v + k] * (double)h[k];
            float f = (float)s;
            if (fabs((double)f) > fabs(s)) f = nextafterf(f, 0.0f);
            acc = f;
        }
        out[v] = acc;
    }
}
'''


@pytest.fixture(scope='module')
def helper(tmp_path_factory):
    if not CC:
        pytest.fail('no system C compiler')
    d = tmp_path_factory.mktemp('screen_helper')
    src, so = str(d / 'helper.c'), str(d / 'helper.so')
    open(src, 'w').write(HELPER)
    subprocess.check_call([CC, '-O2', '-ffp-contract=off', '-shared', '-fPIC', '-I', os.path.join(REPO, 'include'),
                           src, '-o', so, '-lm'])
    L = ctypes.CDLL(so)
    L.screen_eps.restype = ctypes.c_float
    L.screen_eps.argtypes = [ctypes.c_float] * 4
    L.screen_norm.restype = ctypes.c_float
    L.screen_norm.argtypes = [ctypes.c_float]
    for f in (L.chain_logits, L.trunc_logits):
        f.restype = None
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    return L


def bf16(x):
    """fp32 -> bf16 by round-to-nearest-even (v_cvt_pk_bf16_f32), returned as fp32"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000
    return b.astype(np.uint32).view(np.float32)


def flush(x):
    return np.where(np.abs(x) < np.float32(2.0 ** -126), np.float32(0), x).astype(np.float32)


def _call(fn, W, b, h):
    W, b, h = (np.ascontiguousarray(a, np.float32) for a in (W, b, h))
    out = np.empty(W.shape[0], np.float32)
    fn(W.ctypes.data, b.ctypes.data, h.ctypes.data, W.shape[0], out.ctypes.data)
    return out


def eps_of(L, W, b, h, scale=1.0):
    """eps of (row h, matrix W, bias b) from fp32 sums of squares, as a kernel would form them"""
    ss_h = np.float32(0)
    for x in h.astype(np.float32):
        ss_h = np.float32(ss_h + np.float32(x * x))
    with np.errstate(under='ignore', over='ignore'):
        ss_w = (W.astype(np.float32) ** 2).astype(np.float32).sum(axis=1, dtype=np.float32).max()
    return float(L.screen_eps(L.screen_norm(ss_h), L.screen_norm(ss_w), float(np.abs(b).max()), scale))


def screened(L, W, b, h):
    """the screened logits under the three accumulation models, [3, V]"""
    Wb, hb = bf16(W), bf16(h)
    with np.errstate(under='ignore'):
        one = (b.astype(np.float64) + Wb.astype(np.float64) @ hb.astype(np.float64)).astype(np.float32)
    return np.stack([one, _call(L.trunc_logits, Wb, b, hb), _call(L.trunc_logits, flush(Wb), b, flush(hb))])


def check_bound(L, W, b, h, what):
    exact = _call(L.chain_logits, W, b, h)
    true = b.astype(np.float64) + W.astype(np.float64) @ h.astype(np.float64)
    eps = eps_of(L, W, b, h)
    assert np.isfinite(eps) and eps > 0, what
    lt = screened(L, W, b, h)
    err = np.abs(lt.astype(np.float64) - exact.astype(np.float64)).max()
    print('%s: eps %.3e, max |l~ - L| %.3e (%.3f eps), max |L - true| %.3e' % (
        what, eps, err, err / eps, np.abs(exact - true).max()))
    assert err <= eps, what
    return exact, lt, eps


def half_ulp_binade(a):
    """decode_kernel.hip binade_half_ulp: 2^(E - 24) for a in [2^E, 2^(E + 1))"""
    ex = int(np.float32(a).view(np.uint32)) >> 23
    return float(np.uint32((ex - 24) << 23).view(np.float32)) if ex > 24 else 0.0


def check_candidates(exact, lt, eps, what, margin=2e-3):
    """every id of the fp32 tie window of `exact` is a candidate of each screened row"""
    M = exact.max()
    d = (exact - M).astype(np.float32)
    lse64 = np.log(np.exp(d.astype(np.float64)).sum())
    window = np.zeros(exact.size, bool)
    for lse in (np.float32(lse64), np.nextafter(np.float32(lse64), np.float32(np.inf)),
                np.nextafter(np.float32(lse64), np.float32(-np.inf))):    # (no fp32 sum order pins lse's last bit)
        window |= (d - lse).astype(np.float32) == -lse
    assert window[np.argmax(exact)]
    for l in lt:
        mt = l.max()
        q = np.maximum(l[0::2], l[1::2])                                 # the pair-bounded exp-sum over screened logits
        s = np.float32(np.exp((q - mt).astype(np.float64)).sum())
        hi = np.float32(np.log(s)) + np.float32(0.69314718 + margin + 2 * eps)
        thr = np.float32(np.float32(2 * eps) + np.float32(half_ulp_binade(hi)))
        cand = (mt - l).astype(np.float32) <= thr
        assert not (window & ~cand).any(), what
    return int(cand.sum())


def theta_parts(gain, bias_std, sigma=0.01, member=0):
    dims = O.Dims()
    theta = O.make_theta(dims, 0, gain, bias_std)
    table = O.noise_table(1 << 23, 123)
    off = dims.offsets()
    (wo, ws), (bo, _) = off['logit.weight'], off['logit.bias']
    for sign in (+1, -1):
        th = O.perturb(theta, table, O.noise_index(1, 1, member, table.size, dims.D), sigma, sign)
        yield sign, th[wo: wo + ws[0] * ws[1]].reshape(ws), th[bo: bo + ws[0]]


@pytest.mark.parametrize('gain,bias_std', [(1.0, 0.0), (4.0, 0.1)])
def test_bound_and_candidates_on_model_theta(helper, gain, bias_std):
    rng = np.random.Generator(np.random.PCG64(7))
    # h = o * tanh(c) lies in (-1, 1); small rows as at the xavier theta, full-range rows as a trained cell gives
    hs = [rng.uniform(-1, 1, 128), 0.05 * rng.standard_normal(128), rng.uniform(-1, 1, 128) ** 3]
    worst = 0
    for sign, W, b in theta_parts(gain, bias_std):
        for i, h in enumerate(hs):
            h = h.astype(np.float32)
            what = 'gain %g sign %+d h%d' % (gain, sign, i)
            exact, lt, eps = check_bound(helper, W, b, h, what)
            worst = max(worst, check_candidates(exact, lt, eps, what))
    print('gain %g: at most %d candidates per row' % (gain, worst))


def adversarial():
    rng = np.random.Generator(np.random.PCG64(11))
    V = 64
    h = rng.uniform(-1, 1, 128).astype(np.float32)
    zb = np.zeros(V, np.float32)
    yield 'same sign', np.abs(rng.standard_normal((V, 128))).astype(np.float32), zb, np.abs(h)
    # operands one ulp under a bf16 rounding boundary: every product errs the same way
    edge = np.float32(1.00390625) - np.float32(2.0 ** -23)
    yield 'same sign, half-way operands', np.full((V, 128), edge, np.float32), zb, np.full(128, edge, np.float32)
    mag = (2.0 ** rng.uniform(-20, 4, (V, 128)) * rng.choice([-1, 1], (V, 128))).astype(np.float32)
    yield 'magnitudes 2^-20 .. 2^4', mag, rng.standard_normal(V).astype(np.float32), h
    yield 'magnitudes in h too', mag, zb, (2.0 ** rng.uniform(-20, 4, 128) * rng.choice([-1, 1], 128)).astype(np.float32)
    den = rng.standard_normal((V, 128)).astype(np.float32)
    den[:, ::3] = np.float32(1e-40) * rng.integers(1, 9000, (V, 43)).astype(np.float32)
    hd = h.copy()
    hd[1::5] = np.float32(3e-41)
    yield 'subnormal entries', den, zb, hd
    tiny = (np.float32(1e-42) * rng.integers(1, 9000, (V, 128))).astype(np.float32)
    yield 'all-subnormal rows', tiny, (np.float32(1e-41) * rng.integers(-9, 9, V)).astype(np.float32), h
    yield 'subnormal products', (np.float32(2.0 ** -80) * rng.standard_normal((V, 128))).astype(np.float32), zb, \
        (np.float32(2.0 ** -60) * rng.standard_normal(128)).astype(np.float32)
    yield '|bias| >> |w||h|', (1e-3 * rng.standard_normal((V, 128))).astype(np.float32), \
        (1e4 + rng.standard_normal(V)).astype(np.float32), h
    yield 'negative bias, cancelling', np.abs(rng.standard_normal((V, 128))).astype(np.float32), \
        np.full(V, -50.0, np.float32), np.abs(h)


def test_bound_and_candidates_on_adversarial_rows(helper):
    for what, W, b, h in adversarial():
        with np.errstate(under='ignore'):
            exact, lt, eps = check_bound(helper, W, b, h, what)
            check_candidates(exact, lt, eps, what)


def test_scale_widens_and_non_finite_inputs_give_non_finite_eps(helper):
    e1, e32 = helper.screen_eps(3.0, 2.0, 0.5, 1.0), helper.screen_eps(3.0, 2.0, 0.5, 32.0)
    assert 31.9 * e1 < e32 < 32.1 * e1
    for bad in (np.inf, np.nan):
        assert not np.isfinite(helper.screen_eps(bad, 2.0, 0.5, 1.0))
        assert not np.isfinite(helper.screen_eps(3.0, helper.screen_norm(bad), 0.5, 1.0))
        assert not np.isfinite(helper.screen_eps(3.0, 2.0, bad, 1.0))
