"""MI355X-native ``dataset`` module with the reference's names and signatures (``/root/reference/dataset.py``):

* the STFT feature front-end ``ProcessAudio`` / ``pcenfunc`` (:56-76, :130-298) on the HIP kernels of fft.hip;
* the input pipeline: ``DataAugment`` (:79-126), ``CleanNoisyPairDataset`` (:301-390) and
  ``load_CleanNoisyPairDataset`` (:393-412).  The reference augments and mixes inside CPU DataLoader workers through
  torchaudio; here the workers only read and crop (host I/O), the batch goes to the GPU through pinned memory one step
  ahead on a side stream, and gain + both biquads + the clean/noise mix are ONE HIP launch on the whole batch
  (``trunet_augment_mix``, augment.hip).  ``load_CleanNoisyPairDataset`` yields ``(clean, noisy, fileid)`` like the
  reference's loader (train.py:121), already resident in HBM (the ``.cuda()`` of train.py:124-125 is then a no-op);
* an extension for the dereverberation half of TRU-Net: ``Reverb`` and the ``reverb=`` / ``snr_db=`` keywords of the
  dataset and the loader convolve every pair with a room impulse response, mix at a drawn SNR and guard the peak, as one
  more GPU stage of the loader (``trunet_reverb_mix``, reverb.hip); ``RoomSim`` simulates the impulse responses on the GPU
  as well (``trunet_rir_ism``, roomsim.hip: image sources and a diffuse tail), so the stage needs no RIR corpus.
"""
import math
import os
import random

import numpy as np
import torch
import torch.nn as nn
from torch.utils.data import Dataset
from torch.utils.data.distributed import DistributedSampler

from . import _lib as L
from ._lib import check, ptr

N_FFT, HOP, BINS = 512, 128, 257


def _need_gpu(x):
    if not x.is_cuda:
        raise L.TrunetHipError("tinyrecurrentunet_amd.dataset runs on MI355X only (got %s)" % x.device)


def stft_features(audio_BL, pcen=False, _frames_last=False):
    """(B, L) audio -> (B*T, C, 257) features, C = 4 with PCEN (R2 order) else 3.  One launch per batch
    (the reference loops per utterance, D11).

    _frames_last (internal, util.loss_fn): the same values as a ``_lib.FramesLast`` hand-off, [C][257][NP] with zero
    padding columns -- the layout the network's first layer reads, so the network needs no transpose pass."""
    _need_gpu(audio_BL)
    audio_BL = audio_BL.contiguous().float()
    B, Ln = audio_BL.shape
    T = 1 + Ln // HOP
    C = 4 if pcen else 3
    if _frames_last:
        NP = L.frames_padded(B * T)
        x = torch.empty((C, BINS, NP), device=audio_BL.device, dtype=torch.float32)
        mag = torch.empty((BINS, NP), device=audio_BL.device, dtype=torch.float32) if pcen else None
        tw = L.twiddles(N_FFT, audio_BL.device)
        check(L.lib().trunet_stft_features_fl(ptr(audio_BL), ptr(x), ptr(mag), ptr(tw), B, Ln, T, C, NP, L.stream()),
              "stft_features_fl")
        if pcen:
            check(L.lib().trunet_pcen_fl(ptr(mag), ptr(x[1]), B, T, NP, 1e-6, 0.025, 0.98, 2.0, 0.5, L.stream()), "pcen_fl")
        return L.FramesLast(x, B * T)
    feat = torch.empty((B * T, C, BINS), device=audio_BL.device, dtype=torch.float32)
    mag = torch.empty((B, T, BINS), device=audio_BL.device, dtype=torch.float32) if pcen else None
    tw = L.twiddles(N_FFT, audio_BL.device)
    check(L.lib().trunet_stft_features(ptr(audio_BL), ptr(feat), ptr(mag), ptr(tw), B, Ln, T, C, L.stream()),
          "stft_features")
    if pcen:
        out = feat.view(-1)[BINS:]          # channel 1 of frame 0
        check(L.lib().trunet_pcen(ptr(mag), out.data_ptr(), B, T, C * BINS, 1e-6, 0.025, 0.98, 2.0, 0.5,
                                  L.stream()), "pcen")
    return feat


def pcenfunc(x, eps=1e-6, s=0.025, alpha=0.98, delta=2, r=0.5, training=False):
    """dataset.py:56-76 on a (B, T, F=257) magnitude tensor (out of place in both modes)."""
    _need_gpu(x)
    x = x.contiguous().float()
    B, T, F = x.shape
    assert F == BINS
    out = torch.empty_like(x)
    check(L.lib().trunet_pcen(ptr(x), ptr(out), B, T, BINS, eps, s, alpha, float(delta), r, L.stream()), "pcen")
    return out


def unwrap(p, axis=-1):
    """dataset.py:37-51 as it behaves on the tensors the reference passes (>= 3 dims): the phase itself, leading dim
    squeezed (D13: the correction term is identically zero because ``diff`` :24-34 slices only dims 0 and 1)."""
    if p.dim() < 3:
        raise ValueError("unwrap: the reference's diff() only works for >= 3-D tensors (dataset.py:24-34)")
    return p.squeeze(0)


# ----------------------------------------------------------------------------- input pipeline
def _biquad(kind, sr, cutoff, Q=0.7):
    """RBJ cookbook biquad as torchaudio.functional.lowpass_biquad / highpass_biquad build it (the calls of
    dataset.py:124-125), normalised by a0: (b0, b1, b2, a1, a2) in float64."""
    w0 = 2.0 * math.pi * float(cutoff) / float(sr)
    alpha = math.sin(w0) / 2.0 / Q
    c = math.cos(w0)
    b = ((1 - c) / 2, 1 - c, (1 - c) / 2) if kind == "lowpass" else ((1 + c) / 2, -1 - c, (1 + c) / 2)
    a0 = 1 + alpha
    return (b[0] / a0, b[1] / a0, b[2] / a0, -2 * c / a0, (1 - alpha) / a0)


class DataAugment:
    """dataset.py:79-126: gain in [-12, -5) dB, low-pass biquad 7-10 kHz, high-pass biquad 0.8-1.2 kHz (Q = 0.7) on the
    noise signal.  ``draw()`` picks the three parameters with the reference's ``random.choice`` calls in the reference's
    order; ``__call__`` applies them to a (..., L) tensor on the GPU (one launch for all leading rows).  The biquads keep
    their fixed 48 kHz design (``self.sr``), as in the reference, whatever rate the signal has: also after the loader's
    ``resample_to``."""

    def __init__(self):
        self.min_gain, self.max_gain = -12.0, -5.0
        self.lp_min, self.lp_max = 7000, 10000
        self.hp_min, self.hp_max = 800, 1200
        self.sr = 48000
        self.gains = torch.arange(self.min_gain, self.max_gain, 0.033)
        self.lp_freqs = torch.arange(self.lp_min, self.lp_max, 100)
        self.hp_freqs = torch.arange(self.hp_min, self.hp_max, 50)

    def draw(self):
        """(lp_cutoff, hp_cutoff, gain_db) -- dataset.py:118-120."""
        lp_cutoff = random.choice(self.lp_freqs)
        hp_cutoff = random.choice(self.hp_freqs)
        gain = random.choice(self.gains)
        return float(lp_cutoff), float(hp_cutoff), float(gain)

    def params(self, lp_cutoff, hp_cutoff, gain_db):
        """the 11 numbers trunet_augment_mix takes per signal: linear gain, low-pass and high-pass biquad"""
        return np.array((10.0 ** (gain_db / 20.0),) + _biquad("lowpass", self.sr, lp_cutoff) +
                        _biquad("highpass", self.sr, hp_cutoff), dtype=np.float32)

    def __call__(self, x, params=None):
        _need_gpu(x)
        x = x.contiguous().float()
        rows = x.reshape(-1, x.shape[-1])
        if params is None:
            params = np.stack([self.params(*self.draw())] * rows.shape[0]) if rows.shape[0] else None
        par = torch.as_tensor(params, dtype=torch.float32).reshape(-1, 11).to(x.device).contiguous()
        out = torch.empty_like(rows)
        check(L.lib().trunet_augment_mix(ptr(rows), None, ptr(par), ptr(out), None, rows.shape[0], rows.shape[1],
                                         L.stream()), "augment_mix")
        return out.reshape(x.shape)


def _read_wav(path):
    """mono float32 in [-1, 1) like torchaudio.load(normalize=True) (dataset.py:359-360)"""
    from scipy.io.wavfile import read as wavread
    sr, data = wavread(path)
    if data.ndim > 1:
        data = data[:, 0]
    if data.dtype == np.int16:
        data = data.astype(np.float32) / 32768.0
    elif data.dtype == np.int32:
        data = data.astype(np.float32) / 2147483648.0
    elif data.dtype == np.uint8:
        data = (data.astype(np.float32) - 128.0) / 128.0
    return torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)), sr


class RoomSim:
    """Shoebox room simulator (an extension): image-source RIRs up to ``ism_ms`` and a stochastic diffuse
    tail after it, one room per row, on the GPU (``trunet_rir_ism``, roomsim.hip).  ``draw()`` picks a room, a source and
    a microphone on the host (Python's ``random``) and returns them as ONE row of ``ROW`` floats; ``__call__`` turns a
    batch of rows into RIRs whose direct path is a unit tap at 0, the alignment ``Reverb.prepare`` gives measured RIRs.
    The object holds parameters only (the GPU workspace is dropped on pickling), so it travels to DataLoader workers.

    Row layout: Lx Ly Lz | sx sy sz | rx ry rz | six wall reflection coefficients x0 x1 y0 y1 z0 z1 | rt60 | seed_lo seed_hi."""

    ROW = 18
    MAX_ISM_TAPS, MAX_TW, MAX_TAPS, MAX_ORDER, MAX_SPAN_M, MIN_DIM = 8192, 129, 65536, 96, 360.0, 2.0

    def __init__(self, sample_rate=16000, room_dim=((3, 10), (3, 8), (2.4, 4)), rt60=(0.2, 1.0), wall_margin=0.5,
                 distance=(0.3, 3.0), ism_ms=80.0, max_rir_sec=1.0, tw=81, c=343.0):
        self.sample_rate = int(sample_rate)
        self.room_dim = tuple((float(lo), float(hi)) for lo, hi in room_dim)
        self.rt60 = (float(rt60[0]), float(rt60[1]))
        self.wall_margin = float(wall_margin)
        self.distance = (float(distance[0]), float(distance[1]))
        self.ism_ms, self.max_rir_sec, self.tw, self.c = float(ism_ms), float(max_rir_sec), int(tw), float(c)
        if self.sample_rate <= 0 or not self.c > 0 or not self.max_rir_sec > 0:
            raise ValueError("RoomSim: sample_rate, c and max_rir_sec must be positive")
        if len(self.room_dim) != 3 or any(not (self.MIN_DIM <= lo <= hi < float("inf")) for lo, hi in self.room_dim):
            raise ValueError("RoomSim: room_dim is three (lo, hi) ranges in metres with lo >= %g" % self.MIN_DIM)
        if not 0 < self.rt60[0] <= self.rt60[1] < float("inf"):
            raise ValueError("RoomSim: rt60 is a (lo, hi) range of positive seconds")
        inner = [lo - 2 * self.wall_margin for lo, _ in self.room_dim]
        if self.wall_margin < 0 or min(inner) <= 0:
            raise ValueError("RoomSim: wall_margin leaves no space in the smallest room")
        if not 1e-3 < self.distance[0] <= self.distance[1] or self.distance[0] >= math.sqrt(sum(v * v for v in inner)):
            raise ValueError("RoomSim: the distance range does not fit the smallest room")
        if self.tw < 1 or self.tw % 2 == 0 or self.tw > self.MAX_TW:
            raise ValueError("RoomSim: tw must be odd and at most %d" % self.MAX_TW)
        if not 1 <= self.n_c <= self.MAX_ISM_TAPS:
            raise ValueError("RoomSim: ism_ms * sample_rate = %d taps, outside [1, %d]" % (self.n_c, self.MAX_ISM_TAPS))
        if not 1 <= self.max_taps <= self.MAX_TAPS:
            raise ValueError("RoomSim: RIRs of %d taps are out of range (at most %d)" % (self.max_taps, self.MAX_TAPS))
        span = (self.n_c + self.tw // 2 + 1) * self.c / self.sample_rate
        diag = math.sqrt(sum(hi * hi for _, hi in self.room_dim))
        if span > self.MAX_SPAN_M or 1 + (diag + span) / (2 * min(lo for lo, _ in self.room_dim)) > self.MAX_ORDER:
            raise ValueError("RoomSim: images %.0f m away exceed the kernel's caps (%g m, order %d per axis)"
                             % (span, self.MAX_SPAN_M, self.MAX_ORDER))
        self._ws = {}

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_ws"] = {}
        return d

    @property
    def n_c(self):
        """the crossover tap: image sources before it, the diffuse tail from it on"""
        return int(round(self.ism_ms * self.sample_rate / 1000.0))

    @property
    def max_taps(self):
        return int(round(self.max_rir_sec * self.sample_rate))

    @staticmethod
    def sabine(dim, rt60):
        """one reflection coefficient for all six walls from Sabine's formula: alpha = min(0.161 V / (S rt60), 0.99)"""
        lx, ly, lz = (float(v) for v in dim)
        alpha = min(0.161 * lx * ly * lz / (2.0 * (lx * ly + ly * lz + lx * lz) * float(rt60)), 0.99)
        return math.sqrt(1.0 - alpha)

    @classmethod
    def row(cls, dim, src, mic, beta, rt60, seed):
        """a row from explicit values; ``beta`` is one coefficient or six (x0, x1, y0, y1, z0, z1), ``seed`` in [0, 2^32)"""
        beta = [float(beta)] * 6 if np.ndim(beta) == 0 else [float(v) for v in beta]
        seed = int(seed)
        if len(beta) != 6 or len(dim) != 3 or len(src) != 3 or len(mic) != 3 or not 0 <= seed < 2 ** 32:
            raise ValueError("RoomSim.row: three dimensions, two points, one or six coefficients, a 32-bit seed")
        vals = [float(v) for v in dim] + [float(v) for v in src] + [float(v) for v in mic] + beta
        return torch.tensor(vals + [float(rt60), float(seed & 0xFFFF), float(seed >> 16)], dtype=torch.float32)

    @classmethod
    def fields(cls, row):
        """the arguments of ``row()`` back from a row (float32 values as Python numbers)"""
        v = [float(x) for x in torch.as_tensor(row).reshape(cls.ROW)]
        return {"dim": tuple(v[0:3]), "src": tuple(v[3:6]), "mic": tuple(v[6:9]), "beta": tuple(v[9:15]), "rt60": v[15],
                "seed": int(v[16]) | (int(v[17]) << 16)}

    def draw(self):
        """one random room as a row: dimensions and rt60 uniform in their ranges, Sabine's coefficient on all six walls,
        source and microphone redrawn until both keep wall_margin from every wall and their distance lies in ``distance``"""
        f32 = lambda x: float(np.float32(x))                   # the row is float32: test what the kernel will see
        dim = [f32(random.uniform(lo, hi)) for lo, hi in self.room_dim]
        rt60 = random.uniform(*self.rt60)
        m = self.wall_margin
        while True:
            src = [f32(random.uniform(m, v - m)) for v in dim]
            mic = [f32(random.uniform(m, v - m)) for v in dim]
            inside = all(m <= p <= v - m for pt in (src, mic) for p, v in zip(pt, dim))
            if inside and self.distance[0] <= math.dist(src, mic) <= self.distance[1]:
                break
        return self.row(dim, src, mic, self.sabine(dim, rt60), rt60, random.randrange(2 ** 32))

    def __call__(self, rows):
        """rows: (B, ROW) on the GPU -> (rir (B, Kmax) fp32, lens (B,) int32), Kmax = round(max_rir_sec * sample_rate); a
        row of zeros (the collate's padding for "no room") gives length 0 and a zero RIR.  Asynchronous on the current
        stream; the workspace is kept per stream and reused."""
        _need_gpu(rows)
        dev = rows.device
        rows = rows.contiguous().float()
        if rows.dim() != 2 or rows.shape[1] != self.ROW:
            raise ValueError("RoomSim expects (B, %d) rows, got %s" % (self.ROW, tuple(rows.shape)))
        B, Kmax = rows.shape[0], self.max_taps
        rir = torch.empty((B, Kmax), device=dev, dtype=torch.float32)
        lens = torch.empty((B,), device=dev, dtype=torch.int32)
        if B == 0:
            return rir, lens
        ws_bytes = int(L.lib().trunet_rir_ism_workspace_bytes(B, Kmax))
        if ws_bytes == 0:
            raise L.TrunetHipError("trunet_rir_ism: %d rows of %d taps are out of range" % (B, Kmax))
        key = (str(dev), L.stream())
        ws = self._ws.get(key)
        if ws is None or ws.numel() < ws_bytes:
            ws = self._ws[key] = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        check(L.lib().trunet_rir_ism(ptr(rows), self.ROW, ptr(rir), lens.data_ptr(), B, Kmax, float(self.sample_rate),
                                     self.c, self.n_c, self.tw, self.max_rir_sec, ws.data_ptr(), ws_bytes, L.stream()),
              "rir_ism")
        return rir, lens


class Reverb:
    """Room simulation for the training pairs (an extension: the reference has gain and biquads only).
    ``draw()`` picks a room impulse response per item on the host (Python's ``random``, like ``DataAugment.draw``);
    ``__call__`` convolves a whole batch on the GPU (``trunet_reverb_mix``, reverb.hip), mixes the augmented noise in at a
    requested SNR and guards the pair against clipping:

        wet = h * clean (causal, truncated to L);  noisy = wet + g noise;  target = clean ("dry") or h[:early] * clean ("early")

    with ``h[0]`` the direct path, so the target stays time-aligned with ``noisy``.  RIRs come from the wav files of
    ``rir_root`` (mono or channel 0, at ``sample_rate`` exactly: there is no resampling) or, without a folder, from
    ``synthetic()``: exponentially decaying Gaussian noise with the drawn RT60 and direct-to-reverberant ratio.

    With ``room`` (a ``RoomSim``) the RIRs are simulated on the GPU instead: ``draw()`` returns the room's parameter row in
    place of taps, the collate pads and batches the rows like taps, and ``__call__`` reads a ``(B, RoomSim.ROW)`` tensor as
    rows: it runs the simulator on them, then the same convolution stage on the result."""

    PEAK = 0.99

    def __init__(self, rir_root=None, sample_rate=16000, p_reverb=0.5, rt60=(0.2, 1.0), drr_db=(0.0, 15.0),
                 max_rir_sec=1.0, target="dry", early_ms=50.0, room=None):
        if target not in ("dry", "early"):
            raise ValueError("Reverb target must be 'dry' or 'early', got %r" % (target,))
        if room is not None:
            if rir_root is not None:
                raise ValueError("Reverb takes its RIRs from rir_root or from room, not both")
            if room.sample_rate != int(sample_rate):
                raise ValueError("RoomSim is built for %d Hz, Reverb for %d Hz (no resampling)"
                                 % (room.sample_rate, int(sample_rate)))
            if target == "early" and float(early_ms) > room.ism_ms:
                raise ValueError("the early target (%g ms) must lie in the image-source part of the RIR (ism_ms = %g)"
                                 % (float(early_ms), room.ism_ms))
        self.room = room
        self.rir_root, self.sample_rate, self.p_reverb = rir_root, int(sample_rate), float(p_reverb)
        self.rt60, self.drr_db, self.max_rir_sec = tuple(rt60), tuple(drr_db), float(max_rir_sec)
        self.target, self.early_ms = target, float(early_ms)
        self.max_taps = max(int(self.max_rir_sec * self.sample_rate), 1)
        if self.max_taps > 65536:
            raise ValueError("RIRs of more than 65536 taps are not supported (max_rir_sec * sample_rate = %d)" % self.max_taps)
        self.files = None
        if rir_root is not None:
            self.files = sorted(f for f in os.listdir(rir_root) if f.lower().endswith(".wav"))
            if not self.files:
                raise ValueError("no wav files under %s" % rir_root)
        self._ws = {}

    def __getstate__(self):                      # DataLoader workers get the parameters, not the GPU workspace
        d = dict(self.__dict__)
        d["_ws"] = {}
        return d

    @property
    def early_taps(self):
        """taps of the RIR that make the target: 0 = the dry signal"""
        return 0 if self.target == "dry" else max(int(round(self.early_ms * 1e-3 * self.sample_rate)), 1)

    def synthetic(self, seed, rt60, drr_db):
        """float64 numpy RIR of min(rt60, max_rir_sec) * sample_rate taps: h[0] = 1, tail g[n] exp(-6.9078 n / (rt60 sr))
        (60 dB of decay after rt60) with g from default_rng(seed), scaled so that 10 log10(1 / sum_{n>=1} h[n]^2) = drr_db"""
        sr = self.sample_rate
        n = max(int(min(float(rt60), self.max_rir_sec) * sr), 1)
        h = np.zeros(n, dtype=np.float64)
        h[0] = 1.0
        if n > 1:
            t = np.arange(1, n, dtype=np.float64)
            tail = np.random.default_rng(seed).standard_normal(n - 1) * np.exp(-6.9078 * t / (float(rt60) * sr))
            h[1:] = tail * math.sqrt(10.0 ** (-float(drr_db) / 10.0) / float(np.sum(tail * tail)))
        return h

    def prepare(self, h):
        """a measured RIR -> 1-D float32 tensor: everything before the strongest tap dropped (the direct path moves to tap
        0), divided by that tap, truncated to max_rir_sec"""
        h = np.asarray(h, dtype=np.float64).reshape(-1)
        if h.size == 0 or not np.any(h):
            raise ValueError("empty or all-zero RIR")
        i = int(np.argmax(np.abs(h)))
        h = h[i:i + self.max_taps] / h[i]
        return torch.from_numpy(np.ascontiguousarray(h, dtype=np.float32))

    def draw(self):
        """a 1-D float32 RIR (with ``room``: its parameter row), or an empty tensor (no reverberation) with probability
        1 - p_reverb"""
        if random.random() >= self.p_reverb:
            return torch.empty(0, dtype=torch.float32)
        if self.room is not None:                           # the room's parameter row: the taps are made on the GPU
            return self.room.draw()
        if self.files is not None:
            path = os.path.join(self.rir_root, random.choice(self.files))
            h, sr = _read_wav(path)
            if sr != self.sample_rate:
                raise ValueError("RIR %s is sampled at %d Hz, the pipeline at %d Hz (no resampling)"
                                 % (path, sr, self.sample_rate))
            return self.prepare(h.numpy())
        seed = random.randrange(2 ** 31)
        rt60 = random.uniform(*self.rt60)
        drr = random.uniform(*self.drr_db)
        return torch.from_numpy(self.synthetic(seed, rt60, drr).astype(np.float32))

    def __call__(self, clean, rirs, lens, noise=None, snr_db=None):
        """clean, noise: (B, 1, L) on the GPU (noise already augmented, or None); rirs: (B, Kmax) zero-padded, lens: (B,)
        int32 tap counts (0 = the row does not reverberate); snr_db: (B,) or None (unit gain) -> (noisy, target).
        With ``room``, rirs of shape (B, RoomSim.ROW) are parameter rows (all zero: no room): their RIRs and tap counts come
        from the simulator, on the same stream, and ``lens`` is not read.
        Asynchronous on the current stream; the workspace is kept per stream and reused."""
        _need_gpu(clean)
        dev = clean.device
        clean = clean.contiguous().float()
        B, Ln = clean.shape[0], clean.shape[-1]
        if clean.numel() != B * Ln:
            raise ValueError("Reverb expects (B, 1, L) signals, got %s" % (tuple(clean.shape),))
        noise = None if noise is None else noise.to(dev).contiguous().float()
        if noise is not None and noise.numel() != clean.numel():
            raise ValueError("noise must have the shape of clean")
        if self.room is not None and rirs is not None and rirs.dim() == 2 and rirs.shape[-1] == RoomSim.ROW:
            if rirs.shape[0] != B:
                raise ValueError("one room row per signal")
            rirs, lens = self.room(rirs.to(dev))
        Kmax = 0 if rirs is None else int(rirs.shape[-1])
        rirs_d = lens_d = ws = None
        ws_bytes = 0
        if Kmax > 0:
            rirs_d = rirs.to(dev).contiguous().float()
            lens_d = lens.to(dev).to(torch.int32).contiguous()
            if rirs_d.shape[0] != B or lens_d.numel() != B:
                raise ValueError("one RIR row and one length per signal")
            ws_bytes = int(L.lib().trunet_reverb_workspace_bytes(B, Ln, Kmax))
            if ws_bytes == 0:
                raise L.TrunetHipError("trunet_reverb_mix: %d taps are out of range (at most 65536)" % Kmax)
            key = (str(dev), L.stream())
            ws = self._ws.get(key)
            if ws is None or ws.numel() < ws_bytes:
                ws = self._ws[key] = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        snr_d = None if snr_db is None else torch.as_tensor(snr_db, dtype=torch.float32).to(dev).contiguous()
        if snr_d is not None and snr_d.numel() != B:
            raise ValueError("one SNR per signal")
        noisy, target = torch.empty_like(clean), torch.empty_like(clean)
        check(L.lib().trunet_reverb_mix(ptr(clean), ptr(noise), ptr(rirs_d), None if lens_d is None else lens_d.data_ptr(),
                                        ptr(snr_d), self.early_taps, self.PEAK, ptr(noisy), ptr(target),
                                        None if ws is None else ws.data_ptr(), ws_bytes, B, Ln, Kmax, L.stream()),
              "reverb_mix")
        return noisy, target


class CleanNoisyPairDataset(Dataset):
    """dataset.py:301-390.  ``root/clean/fileid_{i}.wav`` and noise files in ``root/keyboard`` (training; each noise file
    must be exactly crop length, D19), or the DNS no-reverb test pairs (testing).  An element is
    ``(clean (1, L), noise (1, L), fileid, aug_params (11,))``: reading and the random crop happen here (host I/O in the
    DataLoader workers), the augmentation of the noise and ``noisy = clean + noise`` (:368, :380) are applied to the
    whole batch on the GPU by the loader of ``load_CleanNoisyPairDataset``.  ``root = "synthetic:<items>"`` generates
    DNS-shaped pairs instead of reading files (benchmarks, smoke runs; no dataset ships with the reference).

    ``reverb`` (a ``Reverb``) and ``snr_db`` (a ``(lo, hi)`` range in dB, uniform per item) are extensions; with either set a
    training element carries two more entries, ``(..., rir (K,), snr or None)``, drawn AFTER everything the 4-tuple draws, and
    the loader runs the reverberation stage.  With both ``None`` nothing changes, random-number consumption included.

    ``resample_to`` (an extension): ``sample_rate`` is the rate of the files, as in config/tiny.json, and the workers crop at
    it exactly as without; the loader then resamples clean and noise to ``resample_to`` on the GPU before it mixes
    (``resample.Resampler``, both signals in one launch).  A file at another rate than ``sample_rate`` is then an error,
    and a ``Reverb`` must be built for ``resample_to``.  With ``None`` elements and batches are exactly as before."""

    def __init__(self, root="./", subset="training", crop_length_sec=0, sample_rate=48000, *, reverb=None, snr_db=None,
                 resample_to=None):
        super().__init__()
        assert subset is None or subset in ["training", "testing"]
        self.root, self.subset = root, subset
        if resample_to is not None:
            from .resample import ratio
            ratio(sample_rate, resample_to)
            resample_to = int(resample_to)
            if reverb is not None and reverb.sample_rate != resample_to:
                raise ValueError("Reverb is built for %d Hz, the dataset resamples to %d Hz"
                                 % (reverb.sample_rate, resample_to))
        elif reverb is not None and reverb.sample_rate != sample_rate:
            raise ValueError("Reverb is built for %d Hz, the dataset for %d Hz (no resampling)"
                             % (reverb.sample_rate, sample_rate))
        self.resample_to = resample_to
        self.reverb = reverb
        self.snr_db = None if snr_db is None else (float(snr_db[0]), float(snr_db[1]))
        self.aug = DataAugment()
        self.crop_length_sec = crop_length_sec
        self.sample_rate = sample_rate
        self.synthetic = isinstance(root, str) and root.startswith("synthetic:")
        if self.synthetic:
            self.files = ["synthetic_%d" % i for i in range(int(root.split(":", 1)[1]))]
            self.noise_files = list(self.files)
        elif subset == "training":
            n_clean = len(os.listdir(os.path.join(root, "clean")))
            self.files = [os.path.join(root, "clean", "fileid_{}.wav".format(i)) for i in range(n_clean)]
            self.noise_files = sorted(os.listdir(os.path.join(root, "keyboard")))
        elif subset == "testing":
            sortkey = lambda name: "_".join(name.split("_")[-2:])          # DNS test-sample names
            base = os.path.join(root, "datasets/test_set/synthetic/no_reverb")
            clean_files = sorted(os.listdir(os.path.join(base, "clean")), key=sortkey)
            noisy_files = sorted(os.listdir(os.path.join(base, "noisy")), key=sortkey)
            self.files = []
            for c, n in zip(clean_files, noisy_files):
                assert sortkey(c) == sortkey(n)
                self.files.append((os.path.join(base, "clean", c), os.path.join(base, "noisy", n)))
            self.crop_length_sec = 0
        else:
            raise NotImplementedError

    def _synthetic(self, n, length):
        g = np.random.default_rng(n)
        c = 0.1 * g.standard_normal(length + 1)
        clean = (0.5 * (c[1:] + c[:-1])).astype(np.float32)
        return torch.from_numpy(clean), torch.from_numpy((0.05 * g.standard_normal(length)).astype(np.float32))

    def __getitem__(self, n):
        fileid = self.files[n]
        crop_length = int(self.crop_length_sec * self.sample_rate)
        if self.subset == "testing" and not self.synthetic:
            clean, sr = _read_wav(fileid[0])
            noisy, sr2 = _read_wav(fileid[1])
            assert len(clean) == len(noisy)
            self._check_rate(fileid[0], sr)
            self._check_rate(fileid[1], sr2)
            # no augmentation: unit gain and identity "filters" are not expressible as biquads, so the loader mixes
            # nothing for testing items (params = None): the second element already IS the noisy signal
            return clean.unsqueeze(0), noisy.unsqueeze(0), fileid, torch.zeros(11)
        if self.synthetic:
            clean, noise = self._synthetic(n, max(crop_length, 1) + self.sample_rate // 4)
            noise = noise[:crop_length] if crop_length > 0 else noise
            random.choice(self.noise_files)                 # same RNG consumption as the file-based path
        else:
            noise_file = random.choice(self.noise_files)
            clean, sr = _read_wav(fileid)
            noise, sr2 = _read_wav(os.path.join(self.root, "keyboard", noise_file))
            self._check_rate(fileid, sr)
            self._check_rate(noise_file, sr2)
            self.sample_rate = sr
            crop_length = int(self.crop_length_sec * sr)
        params = torch.from_numpy(self.aug.params(*self.aug.draw()))
        assert crop_length < len(clean)
        if crop_length > 0:                                   # random crop in the time domain (dataset.py:376-378)
            start = np.random.randint(low=0, high=len(clean) - crop_length + 1)
            clean = clean[start:start + crop_length]
        if len(noise) != len(clean):
            raise ValueError("noise file must be exactly the crop length (%d samples), got %d (dataset.py:380, D19)"
                             % (len(clean), len(noise)))
        if self.reverb is None and self.snr_db is None:
            return clean.unsqueeze(0), noise.unsqueeze(0), fileid, params
        rir = self.reverb.draw() if self.reverb is not None else torch.empty(0, dtype=torch.float32)
        snr = random.uniform(*self.snr_db) if self.snr_db is not None else None
        return clean.unsqueeze(0), noise.unsqueeze(0), fileid, params, rir, snr

    def _check_rate(self, name, sr):
        """with resample_to the loader converts from ``sample_rate``: the rate a worker reads cannot reach it otherwise"""
        if self.resample_to is not None and sr != self.sample_rate:
            raise ValueError("%s is sampled at %d Hz, the dataset resamples from %d Hz to %d Hz"
                             % (name, sr, self.sample_rate, self.resample_to))

    def __len__(self):
        return len(self.files)


def _collate_pairs(items):
    clean = torch.stack([it[0] for it in items])
    other = torch.stack([it[1] for it in items])
    params = torch.stack([it[3] for it in items])
    if len(items[0]) == 4:
        return clean, other, [it[2] for it in items], params
    # reverberant items: ragged RIRs zero-padded to the batch maximum, their tap counts, the SNRs (or None)
    lens = torch.tensor([int(it[4].numel()) for it in items], dtype=torch.int32)
    rirs = torch.zeros((len(items), int(lens.max())), dtype=torch.float32)
    for b, it in enumerate(items):
        rirs[b, :lens[b]] = it[4]
    snr = None if items[0][5] is None else torch.tensor([float(it[5]) for it in items], dtype=torch.float32)
    return clean, other, [it[2] for it in items], params, rirs, lens, snr


class GpuPairLoader:
    """Iterates a DataLoader of (clean, noise, fileid, params) batches and yields ``(clean, noisy, fileid)`` on the GPU:
    batch k+1 is copied host -> HBM (pinned, non-blocking) and augmented + mixed by trunet_augment_mix on a side stream
    while the consumer trains on batch k; an event orders the hand-over.  Batches of a dataset built with ``reverb`` /
    ``snr_db`` carry RIRs and SNRs and take one more GPU stage (``_stage_reverb``); the first element yielded is then the
    target of that stage."""

    def __init__(self, loader, mix=True):
        self.loader, self.mix = loader, mix
        self._plain = None                     # the stage without a room, for a dataset with snr_db only
        self._resampler = None
        self.dataset = loader.dataset
        self.sampler = loader.sampler

    def __len__(self):
        return len(self.loader)

    def _resample(self, clean_d, other_d, dev):
        """dataset.resample_to: clean and noise (B, 1, L) at the files' rate -> (B, 1, ceil(L p / q)), both in one launch
        on the current (side) stream"""
        to = getattr(self.dataset, "resample_to", None)
        if to is None or to == self.dataset.sample_rate:
            return clean_d, other_d
        if self._resampler is None or self._resampler.fs_in != self.dataset.sample_rate or self._resampler.device != dev:
            from .resample import Resampler
            self._resampler = Resampler(self.dataset.sample_rate, to, dev)
        B, _, Ln = clean_d.shape
        y = self._resampler.rows(torch.stack([clean_d.view(B, Ln), other_d.view(B, Ln)]))
        return y[0].unsqueeze(1), y[1].unsqueeze(1)

    def _stage(self, batch, side):
        if batch is None:
            return None
        if not torch.cuda.is_available():
            raise L.TrunetHipError("the input pipeline augments on the GPU: no MI355X visible")
        dev = torch.device("cuda", torch.cuda.current_device())
        if len(batch) == 7:
            return self._stage_reverb(batch, side, dev)
        clean, other, fileid, params = batch
        with torch.cuda.stream(side):
            clean_d = clean.to(dev, non_blocking=True).float().contiguous()
            other_d = other.to(dev, non_blocking=True).float().contiguous()
            clean_d, other_d = self._resample(clean_d, other_d, dev)
            if self.mix:
                par_d = params.to(dev, non_blocking=True).float().contiguous()
                B, _, Ln = other_d.shape
                noisy = torch.empty_like(other_d)
                check(L.lib().trunet_augment_mix(ptr(other_d), ptr(clean_d), ptr(par_d), ptr(noisy), None, B, Ln,
                                                 side.cuda_stream), "augment_mix")
            else:
                noisy = other_d
            ev = side.record_event()
        return clean_d, noisy, fileid, ev

    def _stage_reverb(self, batch, side, dev):
        """augment the noise (trunet_augment_mix without a clean signal: its output IS the augmented noise), then
        reverberate, mix at the drawn SNR and guard the peak (trunet_reverb_mix); the first element handed on is the
        target of the reverberation stage.  Nothing here waits for the device."""
        clean, other, fileid, params, rirs, lens, snr = batch
        if not self.mix:
            raise L.TrunetHipError("reverb / snr_db apply to training items, which carry a noise signal to mix")
        rv = self.dataset.reverb or self._plain
        if rv is None:
            rv = self._plain = Reverb(p_reverb=0.0, sample_rate=getattr(self.dataset, "resample_to", None) or
                                      self.dataset.sample_rate)
        with torch.cuda.stream(side):
            clean_d = clean.to(dev, non_blocking=True).float().contiguous()
            other_d = other.to(dev, non_blocking=True).float().contiguous()
            clean_d, other_d = self._resample(clean_d, other_d, dev)
            par_d = params.to(dev, non_blocking=True).float().contiguous()
            rirs_d = rirs.to(dev, non_blocking=True)
            lens_d = lens.to(dev, non_blocking=True)
            snr_d = None if snr is None else snr.to(dev, non_blocking=True)
            B, _, Ln = other_d.shape
            aug = torch.empty_like(other_d)
            check(L.lib().trunet_augment_mix(ptr(other_d), None, ptr(par_d), ptr(aug), None, B, Ln, side.cuda_stream),
                  "augment_mix")
            noisy, target = rv(clean_d, rirs_d if rirs_d.shape[1] > 0 else None, lens_d, noise=aug, snr_db=snr_d)
            ev = side.record_event()
        return target, noisy, fileid, ev

    def __iter__(self):
        it = iter(self.loader)
        side = torch.cuda.Stream() if torch.cuda.is_available() else None
        nxt = self._stage(next(it, None), side)
        while nxt is not None:
            clean, noisy, fileid, ev = nxt
            nxt = self._stage(next(it, None), side)
            cur = torch.cuda.current_stream()
            cur.wait_event(ev)
            clean.record_stream(cur)
            noisy.record_stream(cur)
            yield clean, noisy, fileid


def load_CleanNoisyPairDataset(root, subset, crop_length_sec, batch_size, sample_rate, num_gpus=1, num_workers=4, *,
                               reverb=None, snr_db=None, resample_to=None):
    """dataset.py:393-412: same arguments (``**trainset_config`` of config/tiny.json + subset, batch_size, num_gpus);
    DistributedSampler when num_gpus > 1, else shuffle.  Returns an iterable of (clean (B,1,L), noisy (B,1,L), fileid).
    ``reverb`` / ``snr_db`` (keyword-only extensions, see ``Reverb``): the training pairs are reverberated and mixed at a
    drawn SNR on the GPU; the first element is then the dereverberation target the ``Reverb`` was built for.
    ``resample_to`` (keyword-only extension): the files are at ``sample_rate``; clean and noise are resampled to
    ``resample_to`` on the GPU before the mix, so the batches have ceil(L resample_to / sample_rate) samples."""
    dataset = CleanNoisyPairDataset(root=root, subset=subset, crop_length_sec=crop_length_sec, sample_rate=sample_rate,
                                    reverb=reverb, snr_db=snr_db, resample_to=resample_to)
    kwargs = {"batch_size": batch_size, "num_workers": num_workers, "pin_memory": torch.cuda.is_available(),
              "drop_last": False, "collate_fn": _collate_pairs}
    if num_gpus > 1:
        loader = torch.utils.data.DataLoader(dataset, sampler=DistributedSampler(dataset), **kwargs)
    else:
        loader = torch.utils.data.DataLoader(dataset, sampler=None, shuffle=True, **kwargs)
    return GpuPairLoader(loader, mix=(subset != "testing" or dataset.synthetic))


class ProcessAudio(nn.Module):
    """dataset.py:130-298.  ``forward`` (1,1,L) -> (T,3,257); ``backward`` (T,3,257) -> (1,L)."""

    def __init__(self, n_fft=512, hop_length=128, sample_rate=48000, min_level_db=-100):
        super().__init__()
        if n_fft != N_FFT or hop_length != HOP:
            raise L.TrunetHipError("the HIP feature kernels are built for n_fft=512, hop=128 (config/tiny.json)")
        self.n_fft, self.hop_length = n_fft, hop_length
        self.n_mels = n_fft // 2 + 1
        self.sample_rate = self.sr = sample_rate
        self.min_level_db = -100.0      # dataset.py:145 overrides the argument
        self.ref_level_db = 25.0

    # elementwise helpers (dataset.py:156-243), kept for API parity; plain tensor expressions (the fused kernels
    # behind forward() / backward() do not call them)
    def get_mag_phase(self, spectrogram):
        """dataset.py:156-159: complex spectrogram -> (|S| without its leading dim, angle S)."""
        return torch.abs(spectrogram).squeeze(0), torch.angle(spectrogram)

    def demod_phase(self, phase):
        """dataset.py:162-179: (sin, cos) of the "demodulated" phase.  The reference's ``unwrap`` (:37-51) is the identity
        on the 3-D / 4-D tensors ProcessAudio passes (its ``diff`` slices only the first two dims) and ends
        in ``squeeze(0)``; the naming is the reference's: real = sin, imag = cos."""
        demodulated = unwrap(phase)
        return torch.sin(demodulated), torch.cos(demodulated)

    def mod_phase(self, magnitude, real_demod, imag_demod):
        """dataset.py:182-203: (norm-dB magnitude, sin, cos) -> complex spectrogram with a leading batch dim."""
        wrap = torch.arctan2(real_demod, imag_demod)
        mag = self.db_to_amp(self.de_norm(magnitude))
        return (mag * torch.exp(1j * wrap)).unsqueeze(0)

    def amp_to_db(self, magnitude):
        return 20 * torch.log10(torch.clamp(magnitude, min=1e-7)) - self.ref_level_db

    def db_to_amp(self, db_spec):
        return torch.pow(10, db_spec / 20.0)

    def perm(self, tensor):
        return tensor.permute(2, 0, 1)

    def de_perm(self, tensor):
        return tensor.permute(1, 2, 0)

    def norm(self, db_spec):
        return torch.clamp((((db_spec - self.min_level_db) / -self.min_level_db) * 2.) - 1., -1, 1)

    def de_norm(self, norm_spec):
        return (((torch.clamp(norm_spec, -1, 1) + 1.) / 2.) * -self.min_level_db) + self.min_level_db + self.ref_level_db

    def forward(self, audio):
        if audio.dim() != 3 or audio.shape[0] != 1 or audio.shape[1] != 1:
            raise ValueError("ProcessAudio.forward expects (1, 1, L) like the reference (dataset.py:246-272)")
        return stft_features(audio[0])

    def backward(self, denoised_features):
        """dataset.py:275-298: (T, 3, 257) (mag, sin, cos) -> (1, L) by rect-window iSTFT."""
        _need_gpu(denoised_features)
        f = denoised_features.contiguous().float()
        T = f.shape[0]
        # the mask/iSTFT kernel consumes the 8-channel net-output layout; present (mag, sin, cos) as a set whose
        # "noise" angle equals the "mixture" angle => sigmoid(0) = 1/2, compensated by doubling afterwards
        o = torch.zeros((T, 8, BINS), device=f.device, dtype=torch.float32)
        o[:, 0], o[:, 2], o[:, 3] = f[:, 0], f[:, 1], f[:, 2]
        o[:, 6], o[:, 7] = f[:, 1], f[:, 2]
        Ln = (T - 1) * HOP
        frames = torch.empty((1, T, N_FFT), device=f.device, dtype=torch.float32)
        audio = torch.empty((1, Ln), device=f.device, dtype=torch.float32)
        check(L.lib().trunet_mask_istft_fwd(ptr(o), ptr(frames), ptr(audio), None, None,
                                            ptr(L.twiddles(N_FFT, f.device)), 1, T, Ln, 0.5, L.stream()), "mask_istft")
        return audio * 2.0
