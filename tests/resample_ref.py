"""Float64 numpy restatement of the resampler definition resample.py pins.

A test helper, independent of the package:

    half = zeros max(p, q), fc = rolloff / (2 max(p, q))
    h[t] = kaiser(2 half + 1, beta)[t + half] 2 fc sinc(2 fc t), t = -half .. half, normalised to unit sum
    y[m] = p sum_n h[m q - n p + half] x[n], m = 0 .. ceil(L p / q) - 1, taps and samples outside their ranges zero

``resample`` also returns ``sum_n |h[.] x[n]|`` per output, the scale of the rounding bound the GPU tests use.
"""
import math

import numpy as np


def ratio(fs_in, fs_out):
    g = math.gcd(int(fs_in), int(fs_out))
    return int(fs_out) // g, int(fs_in) // g


def design(p, q, zeros=16, beta=8.6, rolloff=0.94):
    big = max(p, q)
    half = zeros * big
    fc = rolloff / (2 * big)
    t = np.arange(-half, half + 1)
    h = np.kaiser(2 * half + 1, beta) * 2 * fc * np.sinc(2 * fc * t)
    return h / np.sum(h), half


def taps_per_output(p, half):
    return -(-(2 * half + 1) // p)


def resample(x, p, q, h=None, block=1 << 13):
    """-> (y, a): y[m] as above in float64 and a[m] = sum_n |h[m q - n p + half] x[n]|"""
    x = np.asarray(x, dtype=np.float64)
    if h is None:
        h, half = design(p, q)
    else:
        h = np.asarray(h, dtype=np.float64)
        half = (h.shape[0] - 1) // 2
    L = x.shape[0]
    M = -(-L * p // q)
    K = taps_per_output(p, half)
    xp = np.concatenate([x, [0.0]])                  # index L: a zero for the taps that fall outside x
    y, a = np.empty(M), np.empty(M)
    k = np.arange(K)[None, :]
    for m0 in range(0, M, block):
        m = np.arange(m0, min(M, m0 + block), dtype=np.int64)
        nmax = (m * q + half) // p
        t = (m * q + half - nmax * p)[:, None] + p * k
        n = nmax[:, None] - k
        ok = (t <= 2 * half) & (n >= 0) & (n < L)
        prod = np.where(ok, h[np.minimum(t, 2 * half)] * xp[np.where(ok, n, L)], 0.0)
        y[m0:m0 + m.shape[0]] = p * np.sum(prod, axis=1)
        a[m0:m0 + m.shape[0]] = np.sum(np.abs(prod), axis=1)
    return y, a


def bound(a, p, half):
    """|y_fp32 - y| <= (K + 3) 2^-24 p sum |h x|: K fp32 additions, the rounding of each tap to fp32, of each product's
    fused multiply-add and of the final scaling by p"""
    return (taps_per_output(p, half) + 3) * 2.0 ** -24 * p * a
