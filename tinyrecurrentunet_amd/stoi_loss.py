"""Intelligibility loss: the negative STOI or ESTOI of the estimate against the clean target, differentiable in the
estimate on the GPU.

``STOILoss(extended=False, fs=16000)(estimate, clean, lengths=None)`` takes the input forms of ``evaluate.evaluate`` (two
lists of 1-D cuda tensors, or two padded ``(B, Lmax)`` tensors with ``lengths``) and returns ``-(1 / B) sum_b s_b`` in fp32,
``s_b`` the STOI (ESTOI with ``extended``) of utterance ``b`` exactly as ``evaluate`` scores it: the forward IS evaluate's
(``evaluate._stoi_forward``), so the scores agree bit for bit.  Everything computed from the clean signal -- the silence
mask and kept-frame list, its band magnitudes, the clip level -- is a constant; there is no gradient for ``clean``.

    forward    pack + tables (one host -> device copy), trunet_resample_ragged, trunet_stoi_ragged, trunet_stoi_loss_value
    backward   trunet_stoi_loss_bwd: segment cotangents (fp64), frame gather + inverse kept-frame map, bands (FFT, dZ,
               inverse FFT), 10 kHz samples; then trunet_resample_ragged_bwd (skipped at 10 kHz)

No atomics anywhere: an utterance's gradient is bit for bit independent of its batch-mates and repeatable; an utterance
without a segment scores 1e-5 with an exactly zero gradient; a band magnitude sqrt(a) has derivative 0 at a = 0; the STOI
clip min(y nx / ny, c x) passes the gradient on the branch the forward took (a tie: the first).
"""
import torch

from . import _lib as L
from . import evaluate as ev
from ._lib import check, ptr


class _Run:
    """what one forward leaves for its backward(s)"""
    __slots__ = ("B", "p", "q", "tot", "offs", "op", "sig10", "ws", "extended", "scores", "segments")


def forward_packed(est, clean, lens, p, q, extended):
    """est, clean: packed (sum lens,) fp32 cuda tensors at fs -> _Run (scores (B,) float64, segments int64, state)"""
    dev = est.device
    r = _Run()
    r.B, r.p, r.q, r.extended = len(lens), p, q, bool(extended)
    offs, r.tot = ev._tables(lens, p, q)
    r.offs = torch.from_numpy(offs).to(dev)
    r.op = [r.offs[i].data_ptr() for i in range(6)]
    if r.tot[0]:
        sig = torch.stack([clean, est]).contiguous()
    else:
        sig = torch.zeros((2, 1), device=dev, dtype=torch.float32)
    stoi, estoi, r.segments, r.sig10, r.ws = ev._stoi_forward(sig, r.op, r.tot, p, q, r.B)
    r.scores = estoi if r.extended else stoi
    return r


def loss_value(r, lam=1.0, loss_accum=None):
    """-> (2,) fp32: [-mean_b score_b, lam * that]; loss_accum (a (), fp32 cuda tensor) += the weighted term on the device"""
    vals = torch.empty(2, device=r.scores.device, dtype=torch.float32)
    check(L.lib().trunet_stoi_loss_value(r.scores.data_ptr(), r.B, float(lam), ptr(vals), ptr(loss_accum), L.stream()),
          "stoi_loss_value")
    return vals


def backward_packed(r, gout, lam=1.0):
    """gout: (1,) fp32 cuda cotangent of lam * loss -> packed (sum lens,) fp32 gradient for the estimate at fs"""
    lib, st, dev = L.lib(), L.stream(), r.sig10.device
    nS, _, nR, nF, nG, nC = r.tot
    if nS == 0:
        return torch.zeros(0, device=dev, dtype=torch.float32)
    win, edges = ev._window_edges(dev)
    ws = torch.empty(int(lib.trunet_stoi_loss_workspace_bytes(r.B, nF, nG)), device=dev, dtype=torch.uint8)
    g10 = torch.empty(nR, device=dev, dtype=torch.float32)
    check(lib.trunet_stoi_loss_bwd(r.sig10.data_ptr(), r.op[2], r.op[3], r.op[4], r.op[5], ptr(win), edges.data_ptr(),
                                   ptr(L.twiddles(ev.NFFT, dev)), r.ws.data_ptr(), ws.data_ptr(), ptr(gout),
                                   -float(lam) / r.B, int(r.extended), ptr(g10), r.B, nR, nF, nG, nC, st), "stoi_loss_bwd")
    if (r.p, r.q) == (1, 1):
        return g10
    taps = ev._taps(r.p, r.q, dev)
    g = torch.empty(nS, device=dev, dtype=torch.float32)
    check(lib.trunet_resample_ragged_bwd(ptr(g10), ptr(g), r.op[0], r.op[2], ptr(taps), (taps.shape[0] - 1) // 2, r.p, r.q,
                                         r.B, nS, nR, st), "resample_ragged_bwd")
    return g


class _STOILossFn(torch.autograd.Function):
    """packed estimate, packed clean -> (loss, scores, segments); the run stays with the context, so a second backward on a
    retained graph reads the same state"""

    @staticmethod
    def forward(ctx, est, clean, lens, p, q, extended):
        r = forward_packed(est.detach(), clean, lens, p, q, extended)
        ctx.run = r
        ctx.mark_non_differentiable(r.scores, r.segments)
        return loss_value(r)[0], r.scores, r.segments

    @staticmethod
    def backward(ctx, g_loss, *_):
        g = backward_packed(ctx.run, g_loss.reshape(1).float().contiguous())
        return g, None, None, None, None, None


class STOILoss(torch.nn.Module):
    """-(mean STOI) (``extended``: ESTOI) of ``estimate`` against ``clean`` at ``fs`` Hz (a rate ``evaluate.ratio``
    accepts).  ``scores`` holds the last call's (B,) float64 scores and int64 segment counts, on the device."""

    def __init__(self, extended=False, fs=16000):
        super().__init__()
        self.extended, self.fs = bool(extended), fs
        self.ratio = ev.ratio(fs)
        self.scores = None

    def forward(self, estimate, clean, lengths=None):
        xs, ys, (p, q), _ = ev._check_args(clean, estimate, lengths, self.fs, ("estoi" if self.extended else "stoi",))
        if not xs:
            raise ValueError("no utterance to score")
        dev = xs[0].device
        lens = [int(x.shape[0]) for x in xs]
        whole = (torch.is_tensor(estimate) and estimate.dtype == torch.float32 and estimate.is_contiguous()
                 and all(n == estimate.shape[1] for n in lens))
        est = estimate.reshape(-1) if whole else torch.cat([y.to(device=dev, dtype=torch.float32) for y in ys])
        with torch.no_grad():
            cl = torch.cat([x.to(device=dev, dtype=torch.float32) for x in xs])
        loss, scores, segments = _STOILossFn.apply(est, cl, lens, p, q, self.extended)
        self.scores = (scores, segments)
        return loss
