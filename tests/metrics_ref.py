"""Float64 numpy restatement of the metric definition evaluate.py pins (STOI, ESTOI, SI-SDR).

A test helper, independent of the package: resampling by the polyphase closed form, silent-frame removal, STFT,
third-octave bands, segments.  ``stoi_ref`` also reports the smallest distance of any frame energy to the silence
threshold, which the GPU tests keep above 1e-3 dB so that an fp32 / fp64 difference cannot flip a frame.
"""
import math

import numpy as np

FS = 10000
N_FRAME = 256
HOP = 128
NFFT = 512
NUMBAND = 15
MINFREQ = 150
N = 30
BETA = -15.0
DYN_RANGE = 40.0
EPS = np.finfo(np.float64).eps
WINDOW = np.hanning(N_FRAME + 2)[1:-1]


def ratio(fs):
    g = math.gcd(FS, int(fs))
    return FS // g, int(fs) // g


def kaiser_filter(p, q):
    """the Octave-compatible anti-alias filter, normalised to unit sum -> (hn, L)"""
    fc = 1.0 / (2 * max(p, q))
    L = math.ceil((60 - 8) / (28.714 * fc / 10))
    t = np.arange(-L, L + 1)
    h = np.kaiser(2 * L + 1, 0.1102 * (60 - 8.7)) * 2 * p * fc * np.sinc(2 * fc * t)
    return h / np.sum(h), L


def resample(x, fs, block=1 << 15):
    """y[m] = p sum_n hn[m q - n p + L] x[n] (taps outside [0, 2L] are zero), ceil(len p / q) outputs"""
    x = np.asarray(x, dtype=np.float64)
    p, q = ratio(fs)
    if p == 1 and q == 1:
        return x.copy()
    hn, L = kaiser_filter(p, q)
    M = -(-x.shape[0] * p // q)
    K = -(-(2 * L + 1) // p) + 1
    xp = np.concatenate([x, [0.0]])                  # index len: a zero for the taps that fall outside x
    y = np.empty(M)
    for m0 in range(0, M, block):
        m = np.arange(m0, min(M, m0 + block), dtype=np.int64)
        nmax = (m * q + L) // p
        t = (m * q + L - nmax * p)[:, None] + p * np.arange(K)[None, :]
        n = nmax[:, None] - np.arange(K)[None, :]
        ok = (t <= 2 * L) & (n >= 0) & (n < x.shape[0])
        y[m0:m0 + m.shape[0]] = p * np.sum(np.where(ok, hn[np.minimum(t, 2 * L)] * xp[np.where(ok, n, x.shape[0])], 0.0),
                                           axis=1)
    return y


def band_edges():
    """16 bin indices: band k covers bins [edges[k], edges[k+1])"""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    k = np.arange(NUMBAND)
    lo = MINFREQ * 2.0 ** ((2 * k - 1) / 6)
    hi = MINFREQ * 2.0 ** ((2 * k + 1) / 6)
    ilo = [int(np.argmin((f - e) ** 2)) for e in lo]
    ihi = [int(np.argmin((f - e) ** 2)) for e in hi]
    assert ilo[1:] == ihi[:-1]
    return np.array(ilo + [ihi[-1]], dtype=np.int64)


def _frames(n):
    return list(range(0, n - N_FRAME, HOP))


def remove_silent_frames(x, y):
    """-> (x_sil, y_sil, kept frame indices, smallest |e - threshold| in dB (inf without frames))"""
    starts = _frames(x.shape[0])
    if not starts:
        return np.zeros(0), np.zeros(0), [], math.inf
    fx = np.array([WINDOW * x[i:i + N_FRAME] for i in starts])
    fy = np.array([WINDOW * y[i:i + N_FRAME] for i in starts])
    e = 20 * np.log10(np.linalg.norm(fx, axis=1) + EPS)
    thr = np.max(e) - DYN_RANGE
    keep = np.nonzero(e > thr)[0]
    K = keep.shape[0]
    xs = np.zeros((K - 1) * HOP + N_FRAME)
    ys = np.zeros_like(xs)
    for j, i in enumerate(keep):
        xs[j * HOP:j * HOP + N_FRAME] += fx[i]
        ys[j * HOP:j * HOP + N_FRAME] += fy[i]
    return xs, ys, keep.tolist(), float(np.min(np.abs(e - thr)))


def tob(sig):
    """(frames, 15) third-octave band magnitudes of rfft(w * frame, 512) over range(0, len - 256, 128)"""
    starts = _frames(sig.shape[0])
    if not starts:
        return np.zeros((0, NUMBAND))
    spec = np.fft.rfft(np.array([WINDOW * sig[i:i + N_FRAME] for i in starts]), NFFT, axis=1)
    pw = np.abs(spec) ** 2
    ed = band_edges()
    return np.sqrt(np.stack([pw[:, ed[k]:ed[k + 1]].sum(axis=1) for k in range(NUMBAND)], axis=1))


def _stoi_segment(xs, ys):
    """xs, ys: (15, 30) -> sum over bands of d"""
    c = 10 ** (-BETA / 20)
    tot = 0.0
    for k in range(NUMBAND):
        x, y = xs[k], ys[k]
        y = y * np.linalg.norm(x) / (np.linalg.norm(y) + EPS)
        y = np.minimum(y, x * (1 + c))
        x = x - x.mean()
        y = y - y.mean()
        x = x / (np.linalg.norm(x) + EPS)
        y = y / (np.linalg.norm(y) + EPS)
        tot += float(np.dot(x, y))
    return tot


def _row_col_normalize(a):
    a = a - a.mean(axis=1, keepdims=True)
    a = a / (np.linalg.norm(a, axis=1, keepdims=True) + EPS)
    a = a - a.mean(axis=0, keepdims=True)
    return a / (np.linalg.norm(a, axis=0, keepdims=True) + EPS)


def stoi_ref(x, y, fs):
    """-> dict(stoi, estoi, segments, kept, margin_db) for one clean / estimate pair at ``fs``"""
    x = resample(x, fs)
    y = resample(y, fs)
    xs, ys, keep, margin = remove_silent_frames(x, y)
    X, Y = tob(xs), tob(ys)
    nseg = X.shape[0] - N + 1
    if X.shape[0] < N:
        return dict(stoi=1e-5, estoi=1e-5, segments=0, kept=len(keep), margin_db=margin)
    st, es = 0.0, 0.0
    for m in range(N, X.shape[0] + 1):
        xs_, ys_ = X[m - N:m].T, Y[m - N:m].T
        st += _stoi_segment(xs_, ys_)
        es += float(np.sum(_row_col_normalize(xs_) * _row_col_normalize(ys_))) / N
    return dict(stoi=st / (nseg * NUMBAND), estoi=es / nseg, segments=nseg, kept=len(keep), margin_db=margin)


def si_sdr_ref(s, e):
    s = np.asarray(s, dtype=np.float64)
    e = np.asarray(e, dtype=np.float64)
    s = s - s.mean() if s.shape[0] else s
    e = e - e.mean() if e.shape[0] else e
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.dot(e, s) / np.dot(s, s)
        t = a * s
        return float(10 * np.log10(np.dot(t, t) / np.dot(t - e, t - e)))


def metrics_ref(clean, estimate, fs):
    """all three metrics of one pair"""
    r = stoi_ref(clean, estimate, fs)
    r["si_sdr"] = si_sdr_ref(clean, estimate)
    return r
