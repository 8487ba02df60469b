"""Fixtures of the intelligibility-loss tests (test_stoi_loss_cpu.py, test_stoi_loss_gpu.py) and their references, computed
once per process: modulated noise through a 4-tap mean as the clean signal, stretches scaled by 1e-4 so that frames are
dropped, and clean plus white noise as the estimate.  The lengths are the smallest that give the kept-frame counts K the
backward kernels branch on: 30 (no segment), 31 (one segment), 32 (K - 1 = 31 STFT frames, an odd number, so the last
FFT carries a single frame), 99 (69 segments: two segment workgroups, with a silent stretch in the middle, so the kept frames are not
contiguous), and 34 behind leading silence; at 10 kHz (no resampler), 16 kHz (5/8), 8 kHz (5/4) and 48 kHz (5/24).
"""
import functools
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import stoi_loss_ref as R                                   # noqa: E402

# name: (fs, samples, SNR dB, seed, silent stretches in seconds, kept frames K, segments)
CASES = {
    "k30_10k": (10000, 4096, 5, 3, (), 30, 0),
    "k30_16k": (16000, 6553, 5, 4, (), 30, 0),
    "k31_16k": (16000, 6758, 5, 1, (), 31, 1),
    "k32_8k": (8000, 3480, 0, 2, (), 32, 2),
    "k32_10k": (10000, 4352, 5, 7, (), 32, 2),
    "lead_48k": (48000, 23900, 5, 1, ((0.0, 0.05),), 34, 4),
    "mid_16k": (16000, 21120, 0, 1, ((0.6, 0.66),), 99, 69),
}
GRAD_CASES = ("k30_10k", "k31_16k", "k32_8k", "k32_10k", "lead_48k", "mid_16k")
MARGIN_DB = 1e-3                  # test_evaluate_gpu.py's rule: no frame energy this close to the silence threshold


@functools.lru_cache(maxsize=None)
def pair(name):
    """-> (estimate, clean) fp32 1-D cpu tensors"""
    fs, n, snr, seed, silent = CASES[name][:5]
    g = np.random.default_rng(seed)
    t = np.arange(n) / fs
    x = np.convolve(g.standard_normal(n + 3), np.ones(4) / 4, "valid")[:n]
    x = x * (1 + 0.8 * np.sin(2 * np.pi * 3 * t + g.uniform(0, 6))) * 0.1
    for a, b in silent:
        x[int(a * fs):int(b * fs)] *= 1e-4
    nz = g.standard_normal(n)
    nz *= np.linalg.norm(x) / np.linalg.norm(nz) * 10 ** (-snr / 20)
    return torch.tensor((x + nz).astype(np.float32)), torch.tensor(x.astype(np.float32))


@functools.lru_cache(maxsize=None)
def ref(name, extended):
    """-> dict(loss, g64, g32 (float64 / float32-restatement gradients of -score), r64, r32 (stoi_loss_ref.score dicts))"""
    y, x = pair(name)
    fs = CASES[name][0]
    l64, g64, r64 = R.loss_and_grads([y], [x], fs, extended, torch.float64)
    _, g32, r32 = R.loss_and_grads([y], [x], fs, extended, torch.float32)
    return dict(loss=l64, g64=g64[0], g32=g32[0], r64=r64[0], r32=r32[0])


TAIL_B, TAIL_T, TAIL_LAMBDA = 2, 65, 0.5          # the loss-tail fixture: 2 x 8192 samples (0.512 s at 16 kHz)


@functools.lru_cache(maxsize=None)
def tail_inputs():
    """-> (net_out (B T, 8, 257) fp32, clean (B, L) fp32): a random network output and fixture-like clean rows"""
    g = torch.Generator().manual_seed(11)
    net_out = torch.randn(TAIL_B * TAIL_T, 8, 257, generator=g)
    L = 128 * (TAIL_T - 1)
    rows = []
    for b in range(TAIL_B):
        r = np.random.default_rng(20 + b)
        t = np.arange(L) / 16000
        x = np.convolve(r.standard_normal(L + 3), np.ones(4) / 4, "valid")[:L]
        rows.append(x * (1 + 0.8 * np.sin(2 * np.pi * 3 * t + r.uniform(0, 6))) * 0.1)
    return net_out, torch.tensor(np.stack(rows).astype(np.float32))


@functools.lru_cache(maxsize=None)
def tail_ref(extended, dtype):
    """the tail mask + iSTFT -> L1 + TAIL_LAMBDA * STOI loss, restated: losstail_ref for the mask, the iSTFT and the L1
    gradient, stoi_loss_ref for the term -> dict(loss, audio, g_net, stoi (the unweighted term))"""
    import losstail_ref as LR
    net_out, clean = tail_inputs()
    order = "dft" if dtype == torch.float64 else "fft"
    audio = LR.mask_istft_fwd(net_out, TAIL_T, 0.5, dtype=dtype, order=order)["audio"]
    B, L = audio.shape
    term, gs, _ = R.loss_and_grads(list(audio), list(clean), 16000, extended, dtype)
    g_audio = LR.l1_grad(audio, clean.to(dtype), 1.0 / (B * L)) + TAIL_LAMBDA * torch.stack(gs).to(dtype)
    g_net = LR.mask_istft_bwd(g_audio, net_out, TAIL_T, 0.5, dtype=dtype, order=order)
    loss = (audio.double() - clean.double()).abs().mean() + TAIL_LAMBDA * term
    return dict(loss=loss, audio=audio, g_net=g_net, stoi=term)


def report(line):
    """printed, and appended to parity_stoi_loss.txt in the directory TRUNET_PARITY_DIR names"""
    from convt_cases import report as write
    write(line, "parity_stoi_loss.txt")
