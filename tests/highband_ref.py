"""Float64 numpy restatement of what highband.py pins: the band above 8 kHz carried around a 16 kHz
enhancement.  A test helper, independent of the package; the resampler is tests/resample_ref.py's.

    D = resample(., fs, 16000), U = resample(., 16000, fs) cut to L samples
    lo = D(x), y16 = the enhanced lo, up_y = U(y16), up_x = U(lo), hb = x - up_x
    "drop": up_y      "keep": up_y + hb      "follow": up_y[n] + G[n] hb[n]
    hp = delta - h_lp, h_lp[t] = kaiser(63, 8.6)[t + 31] 0.5 sinc(0.5 t), t = -31 .. 31, unit sum
    a = hp * lo, b = hp * y16 ("same", zeros outside [0, L16))
    e_x[t], e_y[t] = sum of a^2, b^2 over [128 t - 256, 128 t + 256) n [0, L16), t < T = 1 + L16 // 128
    g[t] = clamp(sqrt((e_y[t] + 1e-10) / (e_x[t] + 1e-10)), 10^(floor_db / 20), 1)
    s = n pd, (pd, qd) = ratio(fs, 16000): t0 = s // (128 qd), al = (s % (128 qd)) / (128 qd)
    G[n] = (1 - al) g[t0] + al g[min(t0 + 1, T - 1)]

``gains`` also returns the rounding bound of an fp32 evaluation of g, the scale the GPU test holds the kernel to.
"""
import numpy as np

import resample_ref as RR

HOP, HALF, TAPS = 128, 31, 63
EPS = 1e-10
U32 = 2.0 ** -24


def highpass():
    t = np.arange(-HALF, HALF + 1)
    h = np.kaiser(TAPS, 8.6) * 0.5 * np.sinc(0.5 * t)
    hp = -h / np.sum(h)
    hp[HALF] += 1.0
    return hp


def floor_gain(floor_db):
    return 10.0 ** (floor_db / 20.0)


def n_frames(L16):
    return 1 + L16 // HOP


def same(h, x):
    """(h * x)[n] = sum_k h[k] x[n + 31 - k], zeros outside x -> (the convolution, sum_k |h[k] x[.]|)"""
    x = np.asarray(x, dtype=np.float64)
    return np.convolve(x, h)[HALF:HALF + x.shape[0]], np.convolve(np.abs(x), np.abs(h))[HALF:HALF + x.shape[0]]


def frame_energy(v, beta=None):
    """e[t] = sum of v^2 over W_t -> (e, its fp32 bound sum(2 |v| beta + beta^2) + (|W_t| + 4) u e, or None)"""
    L16 = v.shape[0]
    T = n_frames(L16)
    e, d = np.zeros(T), np.zeros(T)
    for t in range(T):
        a, b = max(HOP * t - 2 * HOP, 0), min(HOP * t + 2 * HOP, L16)
        e[t] = np.sum(v[a:b] ** 2)
        if beta is not None:
            d[t] = np.sum(2 * np.abs(v[a:b]) * beta[a:b] + beta[a:b] ** 2) + (b - a + 4) * U32 * e[t]
    return e, (d if beta is not None else None)


def gains(lo, y16, floor_db=-30.0, g_min=None):
    """-> (g, bound): the frame gains and the bound of |g_fp32 - g|.  The fp32 filter output carries
    beta[n] = 64 u sum_k |h_k x_k| (63 additions and the rounding of each tap), a frame energy
    sum(2 |v| beta + beta^2) + (|W| + 4) u e, and g half the sum of the two relative energy errors plus 3 u (the two
    additions of eps, the division, the square root); the clamp is 1-Lipschitz.  g_min: the clamp's lower end if it is
    not 10^(floor_db / 20) itself (the kernel clamps to that value rounded to fp32)."""
    hp = highpass()
    a, sa = same(hp, lo)
    b, sb = same(hp, y16)
    ex, dx = frame_energy(a, 64 * U32 * sa)
    ey, dy = frame_energy(b, 64 * U32 * sb)
    g_min = floor_gain(floor_db) if g_min is None else g_min
    raw = np.sqrt((ey + EPS) / (ex + EPS))
    bound = raw * (0.5 * (dx / (ex + EPS) + dy / (ey + EPS)) + 3 * U32)
    return np.clip(raw, g_min, 1.0), bound


def gain_index(n, pd, qd):
    """samples n (int64) -> (t0, al)"""
    s = np.asarray(n, dtype=np.int64) * pd
    D = HOP * qd
    return s // D, (s % D) / D


def sample_gains(g, L, pd, qd):
    t0, al = gain_index(np.arange(L, dtype=np.int64), pd, qd)
    T = g.shape[0]
    assert t0.max() <= T - 1
    return (1 - al) * g[t0] + al * g[np.minimum(t0 + 1, T - 1)]


def down(x, fs):
    pd, qd = RR.ratio(fs, 16000)
    return RR.resample(x, pd, qd)[0]


def up(v, fs, L):
    pd, qd = RR.ratio(fs, 16000)
    y = RR.resample(v, qd, pd)[0]
    assert y.shape[0] >= L
    return y[:L]


def join(up_y, up_x, x, G=None):
    """up_y + G (x - up_x); G None: 1"""
    hb = np.asarray(x, dtype=np.float64) - up_x
    return up_y + (hb if G is None else G * hb)


def rejoin(x, lo, y16, fs, mode="follow", floor_db=-30.0):
    x = np.asarray(x, dtype=np.float64)
    L = x.shape[0]
    pd, qd = RR.ratio(fs, 16000)
    up_y = up(y16, fs, L)
    if mode == "drop":
        return up_y
    up_x = up(lo, fs, L)
    if mode == "keep":
        return join(up_y, up_x, x)
    assert mode == "follow"
    g, _ = gains(lo, y16, floor_db)
    return join(up_y, up_x, x, sample_gains(g, L, pd, qd))
