"""Float64 numpy statement of the room simulator trunet_rir_ism computes.

A test helper, independent of the package, and the only yardstick: the reference project has no room simulation.  One row
describes one room (18 float32 values, read as exact numbers):

    Lx Ly Lz | sx sy sz | rx ry rz | bx0 bx1 by0 by1 bz0 bz1 | rt60 | seed_lo seed_hi      (x0: the wall at x = 0, x1: at x = Lx)

Global parameters fs, c, tw, n_c = round(ism_ms fs / 1000), max_rir_sec; fs, c and max_rir_sec pass through float32 like the
arguments of the C entry point.  K_b = clamp(round(min(rt60, max_rir_sec) fs), 1, Kmax).

Image-source part, taps 0 <= n < min(n_c, K_b): for p = (q, j, k) in {0,1}^3 and m in Z^3

    I = ((1-2q) sx + 2 mx Lx, (1-2j) sy + 2 my Ly, (1-2k) sz + 2 mz Lz),   d = |I - r|,   d0 = |s - r|,   tau = (d - d0) fs / c
    gain = bx0^|mx-q| bx1^|mx| by0^|my-j| by1^|my| bz0^|mz-k| bz1^|mz| d0 / d
    h[n] += gain 0.5 (1 + cos(2 pi (n - tau) / tw)) sinc(n - tau)      for the integers n with |n - tau| < tw / 2

Diffuse tail, n_c <= n < K_b, with W = max(round(0.010 fs), 1):

    sigma_c^2 = mean h[n]^2 over max(n_c - W, 0) <= n < n_c
    h[n] = sigma_c g(seed, n) exp(-6.9078 (n - n_c + W/2) / (rt60 fs))

g(seed, n), seed = seed_lo + 65536 seed_hi, all integer arithmetic modulo 2^32:

    mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
    key = mix(seed + 0x9E3779B9);   word(c) = mix(mix(c ^ key) + seed);   a = word(2n),  b = word(2n + 1)
    u1 = ((a >> 8) + 1) / 2^24  in (0, 1];   u2 = (b >> 8) / 2^24  in [0, 1);   g = sqrt(-2 ln u1) cos(2 pi u2)

Taps in [K_b, Kmax) are zero.  A malformed row (``valid``) has length 0 and a zero RIR.
"""
import numpy as np

ROW = 18
M32 = np.uint64(0xFFFFFFFF)


def valid(row):
    """what the kernel accepts: finite values, dimensions >= 2 m, both points strictly inside and >= 1 mm apart, |beta| <= 1,
    rt60 > 0, seed halves integers in [0, 65535]"""
    v = np.asarray(row, dtype=np.float64).reshape(-1)
    if v.size != ROW or not np.all(np.isfinite(v)):
        return False
    L, s, r = v[0:3], v[3:6], v[6:9]
    if np.any(L < 2.0) or np.any(s <= 0) or np.any(s >= L) or np.any(r <= 0) or np.any(r >= L):
        return False
    if np.any(np.abs(v[9:15]) > 1.0) or not v[15] > 0:
        return False
    if np.any(v[16:18] < 0) or np.any(v[16:18] > 65535) or np.any(v[16:18] != np.floor(v[16:18])):
        return False
    return float(np.sqrt(np.sum((s - r) ** 2))) >= 1e-3


def mix(x):
    """lowbias32 on uint64 arrays holding 32-bit values"""
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & M32
    x ^= x >> np.uint64(16)
    return x


def words(seed, n):
    """the two 32-bit words (a, b) of tap n -> uint64 arrays"""
    seed = np.uint64(int(seed) & 0xFFFFFFFF)
    key = mix((seed + np.uint64(0x9E3779B9)) & M32)
    n = np.asarray(n, dtype=np.uint64)
    a = mix((mix((np.uint64(2) * n) ^ key) + seed) & M32)
    b = mix((mix((np.uint64(2) * n + np.uint64(1)) ^ key) + seed) & M32)
    return a, b


def normal(seed, n):
    a, b = words(seed, n)
    u1 = ((a >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0
    u2 = (b >> np.uint64(8)).astype(np.float64) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def sabine(dim, rt60):
    lx, ly, lz = (float(v) for v in dim)
    alpha = min(0.161 * lx * ly * lz / (2.0 * (lx * ly + ly * lz + lx * lz) * float(rt60)), 0.99)
    return float(np.sqrt(1.0 - alpha))


def images(row, d_max):
    """every image with d < d_max -> (d, gain without the d0 / d factor), float64, vectorised over the lattice"""
    v = np.asarray(row, dtype=np.float64)
    L, s, r, beta = v[0:3], v[3:6], v[6:9], v[9:15]
    axes = []
    for a in range(3):
        N = int(np.floor(d_max / (2.0 * L[a]))) + 1                 # |x_I - r| > 2 L (|m| - 1)
        m = np.arange(-N, N + 1, dtype=np.float64)[:, None]
        p = np.array([0.0, 1.0])[None, :]
        off = ((1.0 - 2.0 * p) * s[a] + 2.0 * m * L[a] - r[a]).reshape(-1)
        g = (beta[2 * a] ** np.abs(m - p) * beta[2 * a + 1] ** np.abs(m + 0.0 * p)).reshape(-1)
        keep = np.abs(off) < d_max
        axes.append((off[keep], g[keep]))
    (ox, gx), (oy, gy), (oz, gz) = axes
    ds, gs = [], []
    yz2 = oy[:, None] ** 2 + oz[None, :] ** 2
    gyz = gy[:, None] * gz[None, :]
    for x, g in zip(ox, gx):
        d2 = x * x + yz2
        k = d2 < d_max * d_max
        ds.append(np.sqrt(d2[k]))
        gs.append(g * gyz[k])
    return np.concatenate(ds), np.concatenate(gs)


def ism(row, n_ism, fs, c=343.0, tw=81):
    """the image-source taps 0 .. n_ism - 1 of a valid row -> (h float64, number of images with a non-zero gain that touch a kept tap)"""
    v = np.asarray(row, dtype=np.float64)
    fs, c = float(np.float32(fs)), float(np.float32(c))
    d0 = float(np.sqrt(np.sum((v[3:6] - v[6:9]) ** 2)))
    d_max = d0 + (n_ism + tw / 2.0 + 1.0) * c / fs
    d, g = images(v, d_max)
    tau = (d - d0) * fs / c
    keep = (tau - tw / 2.0 < n_ism - 1) & (g != 0.0)
    d, g, tau = d[keep], g[keep] * d0 / d[keep], tau[keep]
    h = np.zeros(n_ism, dtype=np.float64)
    first = np.ceil(tau - tw / 2.0)
    ks = np.arange(0, tw + 1, dtype=np.float64)
    for i in range(0, len(tau), 20000):
        t0, f0, g0 = tau[i:i + 20000, None], first[i:i + 20000, None], g[i:i + 20000, None]
        n = f0 + ks[None, :]
        t = n - t0
        ok = (np.abs(t) < tw / 2.0) & (n >= 0) & (n < n_ism)
        sinc = np.where(t == np.rint(t), (t == 0.0).astype(np.float64), np.sinc(t))    # exact at the integers
        val = g0 * 0.5 * (1.0 + np.cos(2.0 * np.pi * t / tw)) * sinc
        h += np.bincount(n[ok].astype(np.int64), weights=val[ok], minlength=n_ism)
    return h, int(len(tau))


def rir(row, fs=16000, ism_ms=80.0, max_rir_sec=1.0, Kmax=None, tw=81, c=343.0):
    """-> dict(h (Kmax,) float64, K, n_c, n_ism, sigma, env (Kmax,): sigma_c exp(.) on the tail taps and 0 elsewhere, images)"""
    fs32, mx32 = float(np.float32(fs)), float(np.float32(max_rir_sec))
    n_c = int(round(ism_ms * fs / 1000.0))
    Kmax = int(round(max_rir_sec * fs)) if Kmax is None else int(Kmax)
    out = {"h": np.zeros(Kmax), "K": 0, "n_c": n_c, "n_ism": 0, "sigma": 0.0, "env": np.zeros(Kmax), "images": 0}
    if not valid(row):
        return out
    v = np.asarray(row, dtype=np.float64)
    rt60 = float(v[15])
    K = int(min(max(np.rint(min(rt60, mx32) * fs32), 1), Kmax))
    n_ism = min(n_c, K)
    h, env = out["h"], out["env"]
    h[:n_ism], out["images"] = ism(v, n_ism, fs, c, tw)
    out["K"], out["n_ism"] = K, n_ism
    if K > n_c:
        W = max(int(np.rint(0.010 * fs32)), 1)
        w0 = max(n_c - W, 0)
        sigma = float(np.sqrt(np.mean(h[w0:n_c] ** 2)))
        n = np.arange(n_c, K)
        env[n_c:K] = sigma * np.exp(-6.9078 * (n - n_c + W / 2.0) / (rt60 * fs32))
        h[n_c:K] = env[n_c:K] * normal(int(v[16]) + 65536 * int(v[17]), n)
        out["sigma"] = sigma
    return out


def schroeder_rt60(h, fs, lo_db=-5.0, hi_db=-25.0):
    """RT60 from the slope of the backward-integrated energy decay between lo_db and hi_db (a T20 fit, extrapolated)"""
    e = np.cumsum(np.asarray(h, dtype=np.float64)[::-1] ** 2)[::-1]
    db = 10.0 * np.log10(e / e[0] + 1e-300)
    i0, i1 = int(np.argmax(db <= lo_db)), int(np.argmax(db <= hi_db))
    slope = np.polyfit(np.arange(i0, i1) / float(fs), db[i0:i1], 1)[0]
    return -60.0 / slope
