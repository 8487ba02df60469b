"""Float64 numpy statement of the reverberation stage trunet_reverb_mix computes.

A test helper, independent of the package.  Per row: clean ``x`` (L samples), augmented noise ``v`` (L samples or None),
RIR ``h`` (K taps, ``h[0]`` the direct path; K = 0: the row does not reverberate), ``E`` early taps (0: dry target),
``snr`` in dB or None, ``peak``:

    wet[n] = sum_{k < K, k <= n} h[k] x[n-k]                 (K = 0: wet = x)
    tgt    = x if E = 0 or K = 0 else sum_{k < min(E, K)} h[k] x[n-k]
    g      = sqrt(Ps / (Pv 10^(snr/10))), Ps = mean(wet^2), Pv = mean(v^2);  g = 1 without snr or when Ps or Pv < 1e-20
    noisy  = wet + g v;  m = max|noisy| > peak > 0  =>  noisy, tgt *= peak / m

``conv32_partitioned`` restates the partitioned overlap-save convolution in fp32 (pocketfft through scipy.fft, complex64
accumulation): its distance to the float64 direct convolution is the yardstick the GPU tests scale their bound from.
"""
import numpy as np

PARTITION = 1024
POWER_FLOOR = 1e-20


def conv64(x, h, L=None):
    """direct (time-domain) float64 convolution, causal, truncated to L = len(x)"""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    L = len(x) if L is None else L
    if len(h) == 0:
        return x[:L].copy()
    return np.convolve(x, h)[:L]


def gain(wet, v, snr):
    if v is None or snr is None:
        return 1.0
    ps = float(np.mean(np.asarray(wet, np.float64) ** 2))
    pv = float(np.mean(np.asarray(v, np.float64) ** 2))
    if ps < POWER_FLOOR or pv < POWER_FLOOR:
        return 1.0
    return float(np.sqrt(ps / (pv * 10.0 ** (float(snr) / 10.0))))


def reverb_row(x, v, h, E=0, snr=None, peak=0.99):
    """-> dict(noisy, target, wet, g, scale), float64"""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    K = len(h)
    wet = conv64(x, h)
    tgt = x.copy() if (E == 0 or K == 0) else conv64(x, h[:min(E, K)])
    g = gain(wet, v, snr)
    noisy = wet if v is None else wet + g * np.asarray(v, dtype=np.float64)
    scale = 1.0
    m = float(np.max(np.abs(noisy)))
    if peak > 0 and m > peak:
        scale = peak / m
    return {"noisy": noisy * scale, "target": tgt * scale, "wet": wet, "g": g, "scale": scale}


def reverb_mix(clean, noise, rirs, E=0, snr_db=None, peak=0.99):
    """clean, noise: (B, L) arrays (noise may be None); rirs: list of B 1-D arrays; snr_db: list of B or None"""
    rows = [reverb_row(clean[b], None if noise is None else noise[b], rirs[b], E,
                       None if snr_db is None else snr_db[b], peak) for b in range(len(clean))]
    return np.stack([r["noisy"] for r in rows]), np.stack([r["target"] for r in rows]), rows


def conv32_partitioned(x, h, P=PARTITION):
    """the same convolution as the kernel organises it, in fp32: partitions of P taps, transforms of 2P points over
    windows of P old + P new samples, spectra multiplied and summed per output block, the second half of the inverse kept"""
    import scipy.fft as sf
    x = np.asarray(x, dtype=np.float32)
    h = np.asarray(h, dtype=np.float32)
    L, K = len(x), len(h)
    if K == 0:
        return x.copy()
    nJ, nP = -(-L // P), -(-K // P)
    xp = np.zeros((nJ + 1) * P, dtype=np.float32)
    xp[P:P + L] = x
    hp = np.zeros(nP * P, dtype=np.float32)
    hp[:K] = h
    X = [sf.rfft(xp[j * P:(j + 2) * P]) for j in range(nJ)]
    H = [sf.rfft(np.concatenate([hp[p * P:(p + 1) * P], np.zeros(P, dtype=np.float32)])) for p in range(nP)]
    assert X[0].dtype == np.complex64 and H[0].dtype == np.complex64
    out = np.zeros(nJ * P, dtype=np.float32)
    for j in range(nJ):
        acc = np.zeros(P + 1, dtype=np.complex64)
        for p in range(min(nP - 1, j) + 1):
            acc += X[j - p] * H[p]
        out[j * P:(j + 1) * P] = sf.irfft(acc, n=2 * P)[P:]
    return out[:L]


def rel_err(got, ref):
    """max|got - ref| / max|ref| per row -> 1-D float64 (every sample of every row)"""
    got = np.asarray(got, dtype=np.float64).reshape(-1, np.shape(ref)[-1])
    ref = np.asarray(ref, dtype=np.float64).reshape(got.shape)
    return np.max(np.abs(got - ref), axis=1) / np.maximum(np.max(np.abs(ref), axis=1), 1e-300)


def snr_of(wet, noisy):
    """the SNR in dB of noisy = wet + noise-part, float64"""
    wet = np.asarray(wet, np.float64)
    n = np.asarray(noisy, np.float64) - wet
    return 10.0 * np.log10(np.mean(wet ** 2) / np.mean(n ** 2))
