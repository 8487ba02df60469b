"""The band above 8 kHz around a 16 kHz enhancement.

``enhance(net, xs, fs=48000)`` resamples to 16 kHz, enhances and resamples back; the resampler's low-pass removes what
lies above 8 kHz.  ``rejoin`` carries that band around the network.  With ``D`` = resample(., fs, 16000) and ``U`` =
resample(., 16000, fs) cut to the input's length,

    lo = D(x),  y16 = the enhanced lo,  up_y = U(y16),  up_x = U(lo),  hb = x - up_x

Both filters are symmetric and centred, so ``up_x`` is a zero-phase low-pass of ``x`` and ``hb`` its exact complement: no
delay line.  The modes: ``"drop"`` out = up_y (what ``enhance`` returns without this module), ``"keep"`` out = up_y + hb,
``"follow"`` out[n] = up_y[n] + G[n] hb[n], where G is the suppression the network applied just below the band edge:

    hp = delta - h_lp, h_lp[t] = kaiser(63, 8.6)[t + 31] 0.5 sinc(0.5 t), unit sum     (4 kHz at 16 kHz; ``highpass``)
    a = hp * lo, b = hp * y16                                 ("same" convolutions, zeros outside [0, L16))
    e_x[t], e_y[t] = sum of a^2, b^2 over [128 t - 256, 128 t + 256) n [0, L16),  t < T = 1 + L16 // 128  (the net's frames)
    g[t] = clamp(sqrt((e_y[t] + 1e-10) / (e_x[t] + 1e-10)), 10^(floor_db / 20), 1)
    G[n] = (1 - al) g[t0] + al g[min(t0 + 1, T - 1)],  s = n pd,  t0 = s // (128 qd),  al = (s % (128 qd)) / (128 qd)

with pd / qd = 16000 / fs in lowest terms.  Silence gives 1, an enhancement that amplifies is capped at 1.  One call of
``rejoin`` is one two-plane launch of the cached ``Resampler`` (up_y and up_x), ``trunet_highband_gains`` (not for
``"keep"``) and ``trunet_highband_join`` (highband.hip), with one host -> device copy of the int64 prefix tables; nothing
is read back.  Each utterance's result is bit for bit independent of its batch-mates and their order.  No gradients.
"""
import numpy as np
import torch

from . import _lib as L
from ._lib import check, ptr

MODES = ("drop", "keep", "follow")
SAMPLE_RATE = 16000
HOP = 128
TAPS, HALF, KAISER_BETA, CUTOFF = 63, 31, 8.6, 0.25       # trunet_hip.h: TRUNET_HB_TAPS; cut-off in cycles per sample
KEEP, FOLLOW = 1, 2                                       # trunet_hip.h: TRUNET_HB_KEEP, TRUNET_HB_FOLLOW
RUN, JOIN_TILE = 16, 4096                                 # TRUNET_HB_RUN (hop blocks), TRUNET_HB_JOIN_TILE (samples)
FLOOR_DB = -30.0
INT32_MAX = 2 ** 31 - 1


def highpass():
    """the 63 float64 taps of hp = delta - h_lp: ``resample.design``'s form with half = 31 and fc = 0.25"""
    t = np.arange(-HALF, HALF + 1)
    h = np.kaiser(TAPS, KAISER_BETA) * 2 * CUTOFF * np.sinc(2 * CUTOFF * t)
    hp = -h / np.sum(h)
    hp[HALF] += 1.0
    return hp


def check_args(highband, floor_db):
    """ValueError for a mode outside ``MODES`` and for a floor that is not in (-inf, 0]; host only -> (mode, floor)"""
    if highband not in MODES:
        raise ValueError("highband must be one of %s, got %r" % (MODES, highband))
    if isinstance(floor_db, bool) or not isinstance(floor_db, (int, float, np.integer, np.floating)) or \
            not (-float("inf") < float(floor_db) <= 0.0):
        raise ValueError("highband_floor_db must be a finite number of at most 0 dB, got %r" % (floor_db,))
    return highband, float(floor_db)


def floor_gain(floor_db):
    """g_min = 10^(floor_db / 20) as the fp32 value the kernel clamps to; a floor below fp32's range is its smallest normal"""
    return float(max(np.float32(10.0 ** (float(floor_db) / 20.0)), np.finfo(np.float32).tiny))


def n_frames(n):
    return 1 + int(n) // HOP


_HP = {}


def _taps(dev):
    key = str(dev)
    if key not in _HP:
        _HP[key] = torch.from_numpy(highpass().astype(np.float32)).to(dev).contiguous()
    return _HP[key]


def _signals(name, xs, dev=None):
    """a list of 1-D cuda tensors -> (device, lengths); raises before anything reaches the device"""
    if not isinstance(xs, (list, tuple)):
        raise ValueError("%s: expected a list of 1-D tensors, got %s" % (name, type(xs).__name__))
    for b, t in enumerate(xs):
        if not torch.is_tensor(t) or t.dim() != 1:
            raise ValueError("%s[%d]: expected a 1-D tensor, got %s"
                             % (name, b, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
        if not t.is_cuda or (dev is not None and t.device != dev):
            raise L.TrunetHipError("tinyrecurrentunet_amd runs on MI355X only: %s[%d] is a %s tensor" % (name, b, t.device))
        if t.shape[0] < 1:
            raise ValueError("%s[%d] is empty" % (name, b))
        dev = t.device
    return dev, [int(t.shape[0]) for t in xs]


def _cat(xs):
    return torch.cat([t.to(dtype=torch.float32) for t in xs]).contiguous()


def _gains(lo, y16, so_d, fo_d, B, nS, nT, floor_db):
    """packed lo, y16 (nS) and their device prefix tables -> packed frame gains (nT)"""
    dev = lo.device
    g = torch.empty(nT, device=dev, dtype=torch.float32)
    energy = torch.empty((nT, 2), device=dev, dtype=torch.float32)
    check(L.lib().trunet_highband_gains(ptr(lo), ptr(y16), so_d.data_ptr(), fo_d.data_ptr(), ptr(_taps(dev)), ptr(energy),
                                        ptr(g), B, nS, nT, floor_gain(floor_db), L.stream()), "highband_gains")
    return g


@torch.no_grad()
def gains(lo, y16, floor_db=FLOOR_DB):
    """lo, y16: lists of 1-D cuda tensors at 16 kHz, utterance by utterance of equal lengths -> the list of their frame
    gains g (1 + L16 // 128 each)"""
    _, floor_db = check_args("follow", floor_db)
    dev, lens = _signals("lo", lo)
    _, lens_y = _signals("y16", y16, dev)
    if lens_y != lens:
        raise ValueError("y16 must have the lengths of lo: %s against %s" % (lens_y, lens))
    if not lens:
        return []
    frames = [n_frames(n) for n in lens]
    offs = np.zeros((2, len(lens) + 1), dtype=np.int64)
    offs[0, 1:] = np.cumsum(lens)
    offs[1, 1:] = np.cumsum(frames)
    if int(offs[0, -1]) > INT32_MAX:
        raise ValueError("%d samples: a call packs fewer than 2^31" % int(offs[0, -1]))
    offs_d = torch.from_numpy(offs).to(dev)
    g = _gains(_cat(lo), _cat(y16), offs_d[0], offs_d[1], len(lens), int(offs[0, -1]), int(offs[1, -1]), floor_db)
    return list(torch.split(g, frames))


@torch.no_grad()
def rejoin(x, lo, y16, fs, mode="follow", floor_db=FLOOR_DB):
    """x: the recordings at ``fs`` > 16 kHz; lo = resample(x, fs, 16000); y16: the enhanced lo (lists of 1-D cuda tensors)
    -> the list of results at ``fs``, each of its x's length: U(y16) for "drop", + the band above 8 kHz as it was ("keep")
    or attenuated by the frame gains ("follow", see the module docstring)."""
    from . import resample as R
    mode, floor_db = check_args(mode, floor_db)
    pd, qd = R.ratio(fs, SAMPLE_RATE)
    if pd >= qd:
        raise ValueError("rejoin is for audio above %d Hz (nothing lies above the network's band at %d Hz)"
                         % (SAMPLE_RATE, int(fs)))
    dev, lens = _signals("x", x)
    _, lens_lo = _signals("lo", lo, dev)
    _, lens_y = _signals("y16", y16, dev)
    lens16 = [R.out_length(n, pd, qd) for n in lens]
    if lens_lo != lens16 or lens_y != lens16:
        raise ValueError("lo and y16 must have the lengths of resample(x, %d, %d): %s, got %s and %s"
                         % (int(fs), SAMPLE_RATE, lens16, lens_lo, lens_y))
    if not lens:
        return []
    B = len(lens)
    up = R.resampler(SAMPLE_RATE, fs, dev)
    _, plan = up.plan(lens16)                           # rows: samples at 16 kHz, samples of U(.), the resampler's tiles
    frames = [n_frames(n) for n in lens16]
    offs = np.zeros((5, B + 1), dtype=np.int64)
    offs[:3] = plan
    offs[3, 1:] = np.cumsum(lens)
    offs[4, 1:] = np.cumsum(frames)
    nS, nU, nF, nT = int(offs[0, -1]), int(offs[1, -1]), int(offs[3, -1]), int(offs[4, -1])
    offs_d = torch.from_numpy(offs).to(dev)             # ONE copy
    lo_p, y_p = _cat(lo), _cat(y16)
    ups = up.packed(torch.stack([y_p, lo_p]), plan, 2, offs_d)          # (2, nU): up_y, up_x
    if mode == "drop":
        return [ups[0, o:o + n] for o, n in zip(offs[1, :-1].tolist(), lens)]
    g = _gains(lo_p, y_p, offs_d[0], offs_d[4], B, nS, nT, floor_db) if mode == "follow" else None
    out = torch.empty(nF, device=dev, dtype=torch.float32)
    check(L.lib().trunet_highband_join(ptr(ups[0]), ptr(ups[1]), ptr(_cat(x)), ptr(g), ptr(out), offs_d[3].data_ptr(),
                                       offs_d[1].data_ptr(), offs_d[4].data_ptr(), B, nF, nU, nT, pd, qd,
                                       FOLLOW if mode == "follow" else KEEP, L.stream()), "highband_join")
    return list(torch.split(out, lens))
