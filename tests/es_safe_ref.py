"""Host restatement of nic_es's divide mutation (SM-G-SUM, SM-VECTOR), beside tests/es_ref.py: an offspring of parent p is
theta_p + delta' or theta_p - delta' in fp32 with delta' = fp32(fp32(sigma z) / s_p), IEEE division, s_p the parent's
sensitivity (its own SM-G-SUM vector, or the one vector SM-VECTOR shares). The other modes go to tests/es_ref.py."""
import numpy as np

from tests import es_ref as R


def delta(theta_p, table, idx, sigma, mode, s=None):
    if mode != 'divide':
        return R.delta(theta_p, table, idx, sigma, mode)
    d = (np.float32(sigma) * table[idx: idx + theta_p.size]).astype(np.float32)
    return (d / np.asarray(s, np.float32)).astype(np.float32)


def offspring(theta_p, table, idx, sigma, sign, mode, s=None):
    """sign 0: +, 1: - (offspring id = 2 pair + sign)."""
    d = delta(theta_p, table, idx, sigma, mode, s)
    return (theta_p - d) if sign else (theta_p + d)


def oracle_sensitivity(dims, theta, fc_rows, underflow):
    """oracle/sensitivity_ref.py's SM-G-SUM vector of theta on fc_rows with calc_sensitivity's clamp: fp32 numpy [D]."""
    from nicnes import mutations
    from oracle import sensitivity_ref as SR
    raw = SR.sum_sensitivity((dims.vocab_size + 1, dims.E, dims.R, dims.F), theta, fc_rows, fc_rows.shape[0])
    return mutations.clamp_calc(raw, underflow).numpy()


SENS_RTOL = 5e-5     # the bar of tests/test_gpu_mutations.py: fp32 sums in another order


def sens_close(gpu, ref):
    """elementwise |gpu - ref| <= SENS_RTOL * |ref| + 1e-6 * max|ref|, and the worst excess over the bound."""
    gpu, ref = np.asarray(gpu, np.float64), np.asarray(ref, np.float64)
    err = np.abs(gpu - ref)
    bound = SENS_RTOL * np.abs(ref) + 1e-6 * np.abs(ref).max()
    return bool((err <= bound).all()), float((err / bound).max())
