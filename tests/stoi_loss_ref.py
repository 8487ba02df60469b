"""Torch restatement of the intelligibility loss (stoi_loss.py): the chain evaluate.py pins -- polyphase
resampler to 10 kHz, silent-frame removal, 512-point STFT, third-octave bands, 30-frame STOI / ESTOI segments -- written with
differentiable torch operations, so that autograd through the float64 instance is the reference gradient.

A test helper.  ``dtype`` sets the precision of everything up to the band magnitudes (float64: the reference; float32: the
yardstick that measures what fp32 storage and arithmetic cost on the same inputs); the segments are float64 in both, as in
the kernels.  The silence mask comes from ``metrics_ref`` on the float64 clean signal and is a constant, like everything
else computed from the clean signal.  Two conventions are fixed with ``torch.where``: sqrt has derivative 0 at 0, and the
STOI clip min(u, c x) passes the gradient on the branch the forward took, a tie going to the first.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import metrics_ref as M                                     # noqa: E402
from tinyrecurrentunet_amd.evaluate import kaiser_filter    # noqa: E402

f64 = torch.float64
CLIP = 1.0 + 10 ** (-M.BETA / 20)
NO_SEGMENT = 1e-5


def safe_sqrt(a):
    """sqrt(a) with derivative 0.5 / sqrt(a) for a > 0 and 0 at a == 0"""
    pos = a > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, a, torch.ones_like(a))), torch.zeros_like(a))


def resample(x, fs, dtype=f64):
    """y[m] = p sum_n h[m q - n p + L] x[n] with evaluate.kaiser_filter's taps rounded to ``dtype``; x in ``dtype``"""
    p, q = M.ratio(fs)
    if (p, q) == (1, 1):
        return x
    hn, L = kaiser_filter(p, q)
    h = torch.tensor(hn, dtype=f64).to(dtype)
    n_in = x.shape[0]
    n_out = -(-n_in * p // q)
    K = -(-(2 * L + 1) // p) + 1
    m = np.arange(n_out, dtype=np.int64)
    nmax = (m * q + L) // p
    t = (m * q + L - nmax * p)[:, None] + p * np.arange(K)[None, :]
    n = nmax[:, None] - np.arange(K)[None, :]
    ok = (t <= 2 * L) & (n >= 0) & (n < n_in)
    ti = torch.from_numpy(np.where(ok, t, 0))
    ni = torch.from_numpy(np.where(ok, n, 0))
    w = torch.where(torch.from_numpy(ok), h[ti], torch.zeros((), dtype=dtype))
    return p * (w * x[ni]).sum(dim=1)


def _silence_free(x10, keep, win):
    """overlap-add of the kept windowed frames -> ((K + 1) * 128,)"""
    idx = torch.tensor(keep, dtype=torch.int64)[:, None] * M.HOP + torch.arange(M.N_FRAME)[None, :]
    fr = win * x10[idx]                                       # (K, 256)
    K = len(keep)
    out = torch.zeros((K + 1, M.HOP), dtype=x10.dtype)
    out = out + torch.cat([fr[:, :M.HOP], torch.zeros((1, M.HOP), dtype=x10.dtype)])
    out = out + torch.cat([torch.zeros((1, M.HOP), dtype=x10.dtype), fr[:, M.HOP:]])
    return out.reshape(-1)


def _tob(sig, win, edges):
    """(K - 1, 15) band magnitudes of rfft(w * frame, 512) over range(0, len - 256, 128)"""
    nfr = len(range(0, sig.shape[0] - M.N_FRAME, M.HOP))
    fr = sig.unfold(0, M.N_FRAME, M.HOP)[:nfr] * win
    spec = torch.fft.rfft(fr, M.NFFT, dim=1)
    pw = spec.real ** 2 + spec.imag ** 2
    a = torch.stack([pw[:, edges[k]:edges[k + 1]].sum(dim=1) for k in range(M.NUMBAND)], dim=1)
    return safe_sqrt(a)


def _stoi_segments(X, Y):
    """X, Y: (nseg, 15, 30) float64 -> (per-segment sum over bands of d, the unclipped mask)"""
    nx = safe_sqrt((X * X).sum(dim=2, keepdim=True))
    ny = safe_sqrt((Y * Y).sum(dim=2, keepdim=True)) + M.EPS
    u = Y * nx / ny
    cx = X * CLIP
    first = u <= cx
    yp = torch.where(first, u, cx)
    dx = X - X.mean(dim=2, keepdim=True)
    dy = yp - yp.mean(dim=2, keepdim=True)
    d = (dx * dy).sum(dim=2) / ((safe_sqrt((dx * dx).sum(dim=2)) + M.EPS) * (safe_sqrt((dy * dy).sum(dim=2)) + M.EPS))
    return d.sum(dim=1), first


def _row_col(a):
    a = a - a.mean(dim=2, keepdim=True)
    a = a / (safe_sqrt((a * a).sum(dim=2, keepdim=True)) + M.EPS)
    a = a - a.mean(dim=1, keepdim=True)
    return a / (safe_sqrt((a * a).sum(dim=1, keepdim=True)) + M.EPS)


def score(est, clean, fs, extended=False, dtype=f64):
    """est: 1-D float64 tensor (may require grad), clean: 1-D float64 tensor -> dict(score (float64 scalar tensor),
    segments, kept, margin_db, first (the STOI branch mask, (nseg, 15, 30)) or None)"""
    x64 = M.resample(clean.detach().numpy(), fs)
    _, _, keep, margin = M.remove_silent_frames(x64, x64)
    K = len(keep)
    if K - 1 < M.N:
        return dict(score=torch.tensor(NO_SEGMENT, dtype=f64), segments=0, kept=K, margin_db=margin, first=None)
    win = torch.tensor(M.WINDOW, dtype=f64).to(dtype)
    edges = [int(e) for e in M.band_edges()]
    x10 = resample(clean.detach().to(dtype), fs, dtype)
    y10 = resample(est.to(dtype), fs, dtype)
    X = _tob(_silence_free(x10, keep, win), win, edges).to(f64)
    Y = _tob(_silence_free(y10, keep, win), win, edges).to(f64)
    Xs, Ys = X.unfold(0, M.N, 1), Y.unfold(0, M.N, 1)          # (nseg, 15, 30)
    nseg = Xs.shape[0]
    first = None
    if extended:
        s = (_row_col(Xs) * _row_col(Ys)).sum() / (M.N * nseg)
    else:
        d, first = _stoi_segments(Xs, Ys)
        s = d.sum() / (nseg * M.NUMBAND)
    return dict(score=s, segments=nseg, kept=K, margin_db=margin, first=first)


def loss_and_grads(ests, cleans, fs, extended=False, dtype=f64):
    """-(1 / B) sum_b score_b over lists of 1-D tensors -> (loss float64 tensor, [float64 gradient per estimate], [score
    dicts]); the gradient of an utterance without a segment is exactly zero"""
    ys = [e.detach().to(f64).clone().requires_grad_(True) for e in ests]
    rs = [score(y, c.detach().to(f64), fs, extended, dtype) for y, c in zip(ys, cleans)]
    loss = -sum(r["score"] for r in rs) / len(ys)
    if loss.requires_grad:
        loss.backward()
    return loss.detach(), [y.grad if y.grad is not None else torch.zeros_like(y) for y in ys], rs
