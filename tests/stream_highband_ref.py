"""Float64 numpy restatement of the stream pool's band above 8 kHz (stream_highband.py).  A test
helper, independent of the package; the resampler and the "keep" join are tests/highband_ref.py's.

    lo = D(x), ys16 = the 16 kHz pool's result for lo, up_y = U(ys16)[:L], up_x = U(lo)[:L]
    "keep":   up_y + (x - up_x)
    "follow": up_y[n] + G[n] (x[n] - up_x[n]) with the causal gain
        hp = highband_ref.highpass(); a[n] = sum_{k = 0 .. 62} hp[k] lo[n - k], b the same on ys16 (zeros at negative indices)
        E_x[j], E_y[j] = sum of a^2, b^2 over [128 j, min(128 j + 128, L16)), j < J = ceil(L16 / 128)
        g_c[j] = clamp(sqrt((sum_{i = max(j - 3, 0) .. j} E_y[i] + 1e-10) / (sum_i E_x[i] + 1e-10)), 10^(floor_db / 20), 1)
        s = n pd, D = 128 qd, j = s // D, c = s % D:  G[n] = ((D - c) g_c[max(j - 1, 0)] + c g_c[j]) / D

``block_gains`` also returns the rounding bound of an fp32 evaluation of g_c, derived as highband_ref.gains derives its
own: 63 taps, at most 512 squares in a window of four blocks, a 1-Lipschitz clamp.
"""
import numpy as np

import highband_ref as HR
import resample_ref as RR

HOP, TAPS, EPS, U32 = HR.HOP, HR.TAPS, HR.EPS, HR.U32


def n_blocks(L16):
    return -(-L16 // HOP)


def causal(h, x):
    """(h * x)[n] = sum_k h[k] x[n - k], zeros left of x -> (the convolution, sum_k |h[k] x[.]|), both of x's length"""
    x = np.asarray(x, dtype=np.float64)
    return np.convolve(x, h)[:x.shape[0]], np.convolve(np.abs(x), np.abs(h))[:x.shape[0]]


def trailing_energy(v, beta=None):
    """e[j] = sum of v^2 over blocks max(j - 3, 0) .. j -> (e, its fp32 bound sum(2 |v| beta + beta^2) + (|W| + 4) u e)"""
    L16 = v.shape[0]
    J = n_blocks(L16)
    e, d = np.zeros(J), np.zeros(J)
    for j in range(J):
        a, b = HOP * max(j - 3, 0), min(HOP * (j + 1), L16)
        e[j] = np.sum(v[a:b] ** 2)
        if beta is not None:
            d[j] = np.sum(2 * np.abs(v[a:b]) * beta[a:b] + beta[a:b] ** 2) + (b - a + 4) * U32 * e[j]
    return e, (d if beta is not None else None)


def block_gains(lo, ys16, floor_db=-30.0, g_min=None):
    """-> (g_c, bound of |g_c computed in fp32 - g_c|).  The fp32 filter output carries beta[n] = 64 u sum_k |h_k x_k|
    (63 fused multiply-adds), a window energy sum(2 |v| beta + beta^2) + (|W| + 4) u e (|W| <= 512 squares: two per lane,
    six levels of the wave's tree, three additions of blocks and eps -- far fewer roundings than |W| + 4), and g_c half
    the sum of the two relative energy errors plus 3 u (the additions of eps, the division, the square root); the clamp
    is 1-Lipschitz.  g_min: the clamp's lower end if it is not 10^(floor_db / 20) itself."""
    hp = HR.highpass()
    a, sa = causal(hp, lo)
    b, sb = causal(hp, ys16)
    ex, dx = trailing_energy(a, 64 * U32 * sa)
    ey, dy = trailing_energy(b, 64 * U32 * sb)
    g_min = HR.floor_gain(floor_db) if g_min is None else g_min
    raw = np.sqrt((ey + EPS) / (ex + EPS))
    bound = raw * (0.5 * (dx / (ex + EPS) + dy / (ey + EPS)) + 3 * U32)
    return np.clip(raw, g_min, 1.0), bound


def gain_index(n, pd, qd):
    """samples n (int64) -> (j, c, D)"""
    s = np.asarray(n, dtype=np.int64) * pd
    D = HOP * qd
    return s // D, s % D, D


def sample_gains(g, L, pd, qd):
    j, c, D = gain_index(np.arange(L, dtype=np.int64), pd, qd)
    assert j.max() <= g.shape[0] - 1
    return ((D - c) * g[np.maximum(j - 1, 0)] + c * g[j]) / D


def rejoin(x, lo, ys16, fs, mode="follow", floor_db=-30.0):
    x = np.asarray(x, dtype=np.float64)
    L = x.shape[0]
    pd, qd = RR.ratio(fs, 16000)
    up_y = HR.up(ys16, fs, L)
    if mode == "drop":
        return up_y
    up_x = HR.up(lo, fs, L)
    if mode == "keep":
        return HR.join(up_y, up_x, x)
    assert mode == "follow"
    g, _ = block_gains(lo, ys16, floor_db)
    return HR.join(up_y, up_x, x, sample_gains(g, L, pd, qd))
