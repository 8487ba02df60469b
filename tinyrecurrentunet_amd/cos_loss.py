"""MI355X-native ``cos_loss``: the segmental cosine-similarity loss of ``/root/reference/cos_loss.py:4-56`` in the repaired
form R8, and an SI-SDR loss, both on the kernels of csrc/wave_loss.hip.

R8.  The reference's ``CosSimLoss.forward`` raises for B > 1 (``torch.FloatTensor`` of a list of B-element tensors,
cos_loss.py:56) and for B = 1 returns a detached value that trains nothing.  The repaired definition: with the bounds
0, g[0], g[1], ... each clipped to L (as the reference's slices are), segment i is [bounds[i], bounds[i+1]) and

    L_cos = (1/m) sum_i mean_b (1 - cos_{b,i}),   cos = <x,y> / (max(|x|, eps) max(|y|, eps))     (nn.CosineSimilarity)

an empty segment has cos = 0.  For B = 1 this is the reference's value; for B > 1 it is defined; it is differentiable with
respect to x.  NOTE the reference's default g = [508, 1016, 2032, 4062] covers only the first 4062 samples -- 0.25 s at
16 kHz -- of however long a crop: samples beyond g[-1] get no gradient from this term.  ``CosSimLoss.uniform(segment,
length)`` builds a g that tiles ``length`` samples.

CUDA tensors run three HIP launches (partial sums, finalize, gradient) through one autograd node; CPU tensors take a plain
torch composition of the same definition, so the modules work (and are tested) without a GPU."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from ._lib import check, ptr

DEFAULT_G = (508, 1016, 2032, 4062)


def _check_g(g):
    try:
        g = [int(v) for v in g]
    except (TypeError, ValueError):
        g = []
    if not g:
        raise ValueError("g must be a non-empty list of integer segment ends")
    if len(g) > L.MAX_WAVE_SEG:
        raise ValueError("g has %d entries, at most %d are supported" % (len(g), L.MAX_WAVE_SEG))
    if g[0] <= 0 or any(b <= a for a, b in zip(g, g[1:])):
        raise ValueError("g must be positive and strictly increasing, got %r" % (g[:8],))
    return g


class WavePlan:
    """Device tables of one (length, g, SI-SDR on/off): bounds, first item of each segment, work items (segment, piece)."""

    def __init__(self, length, g, si_sdr, device):
        P = L.WAVE_PIECE
        b = [0] + [min(v, length) for v in g]
        items, first = [], []
        for i in range(len(g)):
            first.append(len(items))
            items += [(i, k) for k in range(-(-(b[i + 1] - b[i]) // P))]
        first.append(len(items))
        if si_sdr:
            items += [(len(g), k) for k in range(-(-length // P))]
        first.append(len(items))
        flat = b + first + [v for it in items for v in it]
        self.table = torch.tensor(flat, dtype=torch.int32, device=device)
        self.length, self.nseg, self.n_items, self.si_sdr = length, len(g), len(items), bool(si_sdr)
        self.o_first, self.o_items = len(b), len(b) + len(first)

    def args(self, audio, clean, cos_lambda=0.0, cos_eps=0.0, si_sdr_lambda=0.0, si_sdr_eps=0.0):
        a = L.WaveLossArgs()
        base = self.table.data_ptr()
        a.audio, a.clean = ptr(audio), ptr(clean)
        a.bounds, a.seg_first, a.items = base, base + 4 * self.o_first, base + 4 * self.o_items
        a.B, a.L, a.nseg, a.n_items = audio.shape[0], self.length, self.nseg, self.n_items
        a.cos_lambda, a.si_sdr_lambda, a.cos_eps, a.si_sdr_eps = cos_lambda, si_sdr_lambda, cos_eps, si_sdr_eps
        return a


_PLANS = {}


def wave_plan(length, g, si_sdr, device):
    """the cached WavePlan; g: validated segment ends (empty: no cosine term)"""
    key = (int(length), tuple(g), bool(si_sdr), str(device))
    plan = _PLANS.get(key)
    if plan is None:
        if len(_PLANS) >= 64:
            _PLANS.clear()
        plan = _PLANS[key] = WavePlan(int(length), list(g), si_sdr, device)
    return plan


def wave_forward(audio, clean, plan, cos_lambda, cos_eps, si_sdr_lambda, si_sdr_eps, loss_accum=None):
    """two launches -> (vals (5), terms (B, nseg + 1), coef (B, nseg + 1, 3)); loss_accum[0] += vals[0] when given"""
    B, dev = audio.shape[0], audio.device
    lib = L.lib()
    nbytes = lib.trunet_wave_loss_workspace_bytes(B, plan.length, plan.nseg)
    if nbytes == 0:
        raise ValueError("wave loss: B = %d, L = %d, %d segments out of range" % (B, plan.length, plan.nseg))
    ws = torch.empty(nbytes // 8, device=dev, dtype=torch.float64)
    vals = torch.empty(5, device=dev, dtype=torch.float32)
    terms = torch.empty((B, plan.nseg + 1), device=dev, dtype=torch.float32)
    coef = torch.empty((B, plan.nseg + 1, 3), device=dev, dtype=torch.float32)
    a = plan.args(audio, clean, float(cos_lambda), float(cos_eps), float(si_sdr_lambda), float(si_sdr_eps))
    check(lib.trunet_wave_loss_fwd(a, ws.data_ptr(), nbytes, ptr(vals), ptr(terms), ptr(coef), ptr(loss_accum), L.stream()),
          "wave_loss_fwd")
    return vals, terms, coef


def wave_backward(audio, clean, plan, coef, g_loss, g):
    """one launch: g += g_loss[0] * (A clean + B audio + C) per segment"""
    check(L.lib().trunet_wave_loss_grad(plan.args(audio, clean), ptr(coef), ptr(g_loss), ptr(g), L.stream()), "wave_loss_grad")


class _WaveLossFn(torch.autograd.Function):
    """audio, clean (B, L) -> (cos_lambda L_cos + si_sdr_lambda L_sisdr, vals, terms); gradient for audio only"""

    @staticmethod
    def forward(ctx, audio, clean, plan, cos_lambda, cos_eps, si_sdr_lambda, si_sdr_eps):
        loss = torch.zeros((), device=audio.device, dtype=torch.float32)
        vals, terms, coef = wave_forward(audio, clean, plan, cos_lambda, cos_eps, si_sdr_lambda, si_sdr_eps, loss_accum=loss)
        ctx.save_for_backward(audio, clean, coef)
        ctx.plan = plan
        ctx.mark_non_differentiable(vals, terms)
        return loss, vals, terms

    @staticmethod
    def backward(ctx, g_loss, _g_vals, _g_terms):
        audio, clean, coef = ctx.saved_tensors
        g = torch.zeros_like(audio)
        wave_backward(audio, clean, ctx.plan, coef, g_loss.reshape(1).float().contiguous(), g)
        return g, None, None, None, None, None, None


def _pair(x, y):
    if x.dim() != 2 or x.shape != y.shape:
        raise ValueError("expected two (B, L) tensors of one shape, got %s and %s" % (tuple(x.shape), tuple(y.shape)))
    return x.float().contiguous(), y.detach().float().contiguous()


def wave_loss(x, y, g=None, cos_lambda=0.0, cos_eps=1e-5, si_sdr_lambda=0.0, si_sdr_eps=1e-8):
    """Both terms of CUDA tensors x (estimate), y (target) through one node -> (cos_lambda L_cos + si_sdr_lambda L_sisdr,
    vals = [that sum, L_cos, mean SI-SDR in dB, cos_lambda L_cos, si_sdr_lambda L_sisdr], terms (B, m + 1) = 1 - cos per
    segment, then SI-SDR in dB per row).  A term whose lambda is not positive is not computed."""
    x, y = _pair(x, y)
    g = _check_g(DEFAULT_G if g is None else g) if cos_lambda > 0 else []
    plan = wave_plan(x.shape[1], g, si_sdr_lambda > 0, x.device)
    if plan.n_items == 0:
        raise ValueError("wave_loss: neither term is enabled")
    return _WaveLossFn.apply(x, y, plan, float(cos_lambda) if g else 0.0, float(cos_eps),
                             float(si_sdr_lambda) if plan.si_sdr else 0.0, float(si_sdr_eps))


def cos_sim_loss_torch(x, y, g, eps):
    """R8 composed from torch ops (any device, any float dtype)"""
    n = x.shape[1]
    b = [0] + [min(v, n) for v in g]
    total = x.new_zeros(())
    for i in range(len(g)):
        if b[i + 1] <= b[i]:
            total = total + 1.0
            continue
        cos = F.cosine_similarity(x[:, b[i]:b[i + 1]], y[:, b[i]:b[i + 1]], dim=1, eps=eps)
        total = total + (1.0 - cos).mean()
    return total / len(g)


def si_sdr_loss_torch(x, y, eps):
    """-mean_b SI-SDR (dB) composed from torch ops; rows with a constant target contribute 0"""
    xm, ym = x - x.mean(1, keepdim=True), y - y.mean(1, keepdim=True)
    sxy, sxx, syy = (xm * ym).sum(1), (xm * xm).sum(1), (ym * ym).sum(1)
    live = syy > 0
    p = sxy * sxy / torch.where(live, syy, torch.ones_like(syy))
    ratio = torch.where(live, (p + eps) / (sxx - p + eps), torch.ones_like(syy))
    return -(10.0 * torch.log10(ratio)).mean()


class CosSimLoss(nn.Module):
    """cos_loss.py:4-56 (R8): mean over the segments of g of the batch-mean of 1 - cosine similarity of x and y.

    eps: clamp of each norm (nn.CosineSimilarity); g: increasing segment ends in samples.  The default g covers only the
    first 4062 samples (0.25 s at 16 kHz); ``CosSimLoss.uniform(segment, length)`` tiles a whole crop.  Call: (x, y), each
    (B, L) -> scalar, differentiable with respect to x."""

    def __init__(self, eps=1e-5, g=DEFAULT_G):
        super().__init__()
        self.eps = float(eps)
        self.g = _check_g(g)
        self.m = len(self.g)

    @classmethod
    def uniform(cls, segment, length, eps=1e-5):
        """segments of ``segment`` samples tiling [0, length): the last one ends at ``length``"""
        segment, length = int(segment), int(length)
        if segment <= 0 or length <= 0:
            raise ValueError("segment and length must be positive")
        g = list(range(segment, length, segment)) + [length]
        return cls(eps=eps, g=g)

    def forward(self, x, y):
        if not x.is_cuda:
            if x.dim() != 2 or x.shape != y.shape:
                raise ValueError("expected two (B, L) tensors of one shape")
            return cos_sim_loss_torch(x, y.detach(), self.g, self.eps)
        x, y = _pair(x, y)
        plan = wave_plan(x.shape[1], self.g, False, x.device)
        return _WaveLossFn.apply(x, y, plan, 1.0, self.eps, 0.0, 0.0)[0]


class SISDRLoss(nn.Module):
    """-mean_b SI-SDR(x, y) in dB, per row over all samples with both signals zero-mean (evaluate.py's definition with
    ``eps`` added to numerator and denominator; eps = 0 is that definition).  Call: (x, y), each (B, L) -> scalar,
    differentiable with respect to x; a row whose target is constant contributes 0."""

    def __init__(self, eps=1e-8):
        super().__init__()
        if not eps >= 0:
            raise ValueError("eps must be non-negative")
        self.eps = float(eps)

    def forward(self, x, y):
        if not x.is_cuda:
            if x.dim() != 2 or x.shape != y.shape:
                raise ValueError("expected two (B, L) tensors of one shape")
            return si_sdr_loss_torch(x, y.detach(), self.eps)
        x, y = _pair(x, y)
        plan = wave_plan(x.shape[1], [], True, x.device)
        return _WaveLossFn.apply(x, y, plan, 0.0, 0.0, 1.0, self.eps)[0]
