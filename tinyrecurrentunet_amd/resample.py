"""Rational sample-rate conversion on the GPU: audio at any common rate to the network's 16 kHz and back.

``resample(x, fs_in, fs_out)`` takes the input forms of ``enhance.enhance`` (a list of 1-D fp32 cuda tensors, or a padded
``(B, Lmax)`` tensor with ``lengths``) and returns the same form at ``fs_out``: utterance b of L_b samples becomes
``ceil(L_b p / q)`` samples, ``p / q = fs_out / fs_in`` in lowest terms,

    y[m] = p sum_n h[m q - n p + half] x[n]            (taps and samples outside their ranges count as zero)

which is ``scipy.signal.resample_poly(x, p, q, window=h)`` with ``h`` the Kaiser-windowed sinc of ``design``.  One launch of
``trunet_resample_rational`` (resample.hip) for the whole batch, no device -> host synchronisation: the host builds the
int64 prefix tables (samples in, samples out, tiles) from the lengths and copies them once.  Each utterance's result is bit
for bit independent of its batch-mates, their order and the input form.  No gradients flow through it.

Not here: resampling inside ``AudioStream`` / ``StreamPool`` (it needs filter state across hops), and ``evaluate``'s own
10 kHz resampler, which keeps its limits.
"""
import math

import numpy as np
import torch

from . import _lib as L
from ._lib import check, ptr
from .enhance import _inputs

MAX_RATIO = 640              # 8, 11.025, 12, 22.05, 24, 32, 44.1, 48, 88.2, 96 kHz <-> 16 kHz; worst 11.025 -> 16: 640/441
ZEROS, BETA, ROLLOFF = 16, 8.6, 0.94
# resample.hip: RS_MAX_TILE, RS_SPAN_MAX (floats of input staged per window), RS_TAPS_LDS_MAX (floats of the tap table)
MAX_TILE = 4096
SPAN_FLOATS = 4608
TAPS_LDS_FLOATS = 16384
LDS_BUDGET = 4 * (SPAN_FLOATS + TAPS_LDS_FLOATS)        # 82 KiB of the CU's 160 KiB: the most a workgroup ever asks for
INT32_MAX = 2 ** 31 - 1


def ratio(fs_in, fs_out):
    """fs_out / fs_in in lowest terms -> (p, q); ValueError for rates that are not positive integers or when p or q
    exceeds MAX_RATIO"""
    for fs in (fs_in, fs_out):
        if isinstance(fs, bool) or not isinstance(fs, (int, float, np.integer, np.floating)) or fs != fs or \
                fs in (float("inf"), float("-inf")) or int(fs) != fs or fs <= 0:
            raise ValueError("sample rates must be positive integers, got %r" % (fs,))
    fs_in, fs_out = int(fs_in), int(fs_out)
    g = math.gcd(fs_in, fs_out)
    p, q = fs_out // g, fs_in // g
    if max(p, q) > MAX_RATIO:
        raise ValueError("%d -> %d Hz reduces to %d/%d, and resampling supports ratios up to %d"
                         % (fs_in, fs_out, p, q, MAX_RATIO))
    return p, q


def design(p, q, zeros=ZEROS, beta=BETA, rolloff=ROLLOFF):
    """Kaiser-windowed sinc for the ratio p / q -> (2 half + 1 float64 taps of unit sum, half): ``zeros`` zero crossings
    of the sinc on either side at the lower of the two rates, cut-off at ``rolloff`` of its Nyquist frequency"""
    big = max(int(p), int(q))
    half = int(zeros) * big
    fc = float(rolloff) / (2 * big)
    t = np.arange(-half, half + 1)
    h = np.kaiser(2 * half + 1, beta) * 2 * fc * np.sinc(2 * fc * t)
    return h / np.sum(h), half


def out_length(n, p, q):
    return -(-int(n) * p // q)


def taps_per_output(p, half):
    """K: the most taps one output reads, ceil((2 half + 1) / p)"""
    return -(-(2 * half + 1) // p)


def phase_table(h, p):
    """taps -> (p, Kp) phase-major table, table[r, k] = h[r + k p], zero past the last tap; Kp = K rounded up to 4"""
    h = np.asarray(h)
    K = -(-h.shape[0] // p)
    Kp = (K + 3) & ~3
    flat = np.zeros(p * Kp, dtype=h.dtype)
    flat[:h.shape[0]] = h
    return np.ascontiguousarray(flat.reshape(Kp, p).T)


def span_floats(p, q, tile, half=None):
    """input samples the outputs of one full tile read, as resample.hip lays them out (a multiple of 4)"""
    half = ZEROS * max(p, q) if half is None else half
    Kp = (taps_per_output(p, half) + 3) & ~3
    return (((tile - 1) * q + p - 1) // p + Kp + 1 + 3) & ~3


def tile_outputs(p, q, half=None):
    """outputs per workgroup: the largest multiple of 256, at most MAX_TILE, whose input span fits SPAN_FLOATS.  Ratios far
    below 1 (q / p above 16 or so) do not fit even at 256; the kernel then stages the span in windows of SPAN_FLOATS."""
    half = ZEROS * max(p, q) if half is None else half
    room = SPAN_FLOATS - ((taps_per_output(p, half) + 3) & ~3) - 1      # ceil((tile - 1) q / p) must fit it
    return min(max((room * p // q + 1) // 256 * 256, 256), MAX_TILE)


def windows(p, q, half=None):
    """staging windows per tile: 1 whenever the span of tile_outputs(p, q) fits SPAN_FLOATS"""
    return -(-span_floats(p, q, tile_outputs(p, q, half), half) // SPAN_FLOATS)


def taps_in_lds(p, half):
    """whether the kernel keeps the tap table in LDS (it must fit TAPS_LDS_FLOATS) or reads its rows from L2"""
    return p * ((taps_per_output(p, half) + 3) & ~3) <= TAPS_LDS_FLOATS


def lds_bytes(p, q, half=None):
    """LDS one workgroup asks for"""
    half = ZEROS * max(p, q) if half is None else half
    span = min(span_floats(p, q, tile_outputs(p, q, half), half), SPAN_FLOATS)
    return 4 * (span + (p * ((taps_per_output(p, half) + 3) & ~3) if taps_in_lds(p, half) else 0))


def plan(lens, p, q, tile):
    """host side of a call: lengths -> (output lengths, (3, B + 1) int64 prefix table of samples in, samples out and tiles).
    Raises for an empty utterance and for totals beyond int32 packing."""
    for b, n in enumerate(lens):
        if n < 1:
            raise ValueError("utterance %d is empty" % b)
    outs = [out_length(n, p, q) for n in lens]
    offs = np.zeros((3, len(lens) + 1), dtype=np.int64)
    offs[0, 1:] = np.cumsum(np.array(lens, dtype=np.int64))
    offs[1, 1:] = np.cumsum(np.array(outs, dtype=np.int64))
    offs[2, 1:] = np.cumsum(np.array([-(-m // tile) for m in outs], dtype=np.int64))
    if max(int(offs[0, -1]), int(offs[1, -1])) > INT32_MAX:
        raise ValueError("%d samples in, %d out: a call packs fewer than 2^31 of each"
                         % (int(offs[0, -1]), int(offs[1, -1])))
    return outs, offs


class Resampler:
    """fs_in -> fs_out with the device copy of the tap table and the layout constants kept for repeated calls.
    ``taps``: other taps than ``design``'s (float64, 2 half + 1 of them, half a multiple of max(p, q));
    ``lds_taps``: force the tap table into LDS (True) or leave it in L2 (False); default: LDS when it fits."""

    def __init__(self, fs_in, fs_out, device="cuda", taps=None, lds_taps=None):
        self.fs_in, self.fs_out = int(fs_in), int(fs_out)
        self.p, self.q = ratio(fs_in, fs_out)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.TrunetHipError("tinyrecurrentunet_amd runs on MI355X only: Resampler on %s" % self.device)
        self.identity = self.p == self.q
        self._rows = {}
        if self.identity:
            return
        if taps is None:
            h, self.half = design(self.p, self.q)
        else:
            h = np.asarray(taps, dtype=np.float64)
            self.half = (h.shape[0] - 1) // 2
            big = max(self.p, self.q)
            if h.ndim != 1 or h.shape[0] != 2 * self.half + 1 or self.half < big or self.half % big:
                raise ValueError("taps: 2 half + 1 values with half a positive multiple of max(p, q) = %d" % big)
        self.K = taps_per_output(self.p, self.half)
        self.tile = tile_outputs(self.p, self.q, self.half)
        self.lds_taps = taps_in_lds(self.p, self.half) if lds_taps is None else bool(lds_taps)
        if self.lds_taps and not taps_in_lds(self.p, self.half):
            raise ValueError("a table of %d x %d taps does not fit the LDS share of %d floats"
                             % (self.p, (self.K + 3) & ~3, TAPS_LDS_FLOATS))
        self.table = torch.from_numpy(phase_table(h, self.p).astype(np.float32)).to(self.device).contiguous()

    def out_lengths(self, lens):
        return [out_length(n, self.p, self.q) for n in lens]

    def plan(self, lens):
        return plan(lens, self.p, self.q, self.tile)

    def rows(self, x):
        """x: (nsig, B, L) fp32 on the device, nsig 1 or 2, every row one utterance of L samples -> (nsig, B, ceil(L p / q)).
        The prefix tables of a (B, L) are built and copied once and kept (the loader's every batch has the same)."""
        nsig, B, Ln = x.shape
        if self.identity:
            return x.clone()
        key = (B, Ln)
        if key not in self._rows:
            outs, offs = self.plan([Ln] * B)
            self._rows = {key: (outs[0] if outs else 0, offs, torch.from_numpy(offs).to(self.device))}
        M, offs, offs_d = self._rows[key]
        return self.packed(x.contiguous().view(nsig, B * Ln), offs, nsig, offs_d).view(nsig, B, M)

    def packed(self, sig, offs, nsig=1, offs_d=None):
        """sig: (nsig, total_in) fp32 on the device, the utterances of every plane back to back as ``offs`` (from ``plan``)
        says -> (nsig, total_out).  One launch on the current stream, nothing read back."""
        if nsig not in (1, 2):
            raise ValueError("nsig must be 1 or 2, got %r" % (nsig,))
        B = offs.shape[1] - 1
        nI, nO, nT = (int(v) for v in offs[:, -1])
        if tuple(sig.shape) != (nsig, nI):
            raise ValueError("expected %s packed samples, got %s" % ((nsig, nI), tuple(sig.shape)))
        if offs_d is None:
            offs_d = torch.from_numpy(offs).to(self.device)
        out = torch.empty((nsig, nO), device=self.device, dtype=torch.float32)
        check(L.lib().trunet_resample_rational(ptr(sig), ptr(out), offs_d[0].data_ptr(), offs_d[1].data_ptr(),
                                               offs_d[2].data_ptr(), ptr(self.table), self.half, self.K, self.p, self.q,
                                               self.tile, B, nI, nO, nT, nsig, int(self.lds_taps), L.stream()),
              "resample_rational")
        return out

    def __call__(self, x, lengths=None, x2=None):
        """x as for ``resample``; ``x2``: a second signal of the same form and lengths, resampled in the same launch
        (-> a pair of results)."""
        xs, width = _check(x, lengths)
        planes = [xs]
        if x2 is not None:
            ys, width2 = _check(x2, lengths)
            if [int(t.shape[0]) for t in ys] != [int(t.shape[0]) for t in xs] or width2 != width:
                raise ValueError("the second signal must have the lengths of the first")
            planes.append(ys)
        lens = [int(t.shape[0]) for t in xs]
        if self.identity:
            res = [_unpack([t.to(dtype=torch.float32).clone() for t in v], lens, width, self.device) for v in planes]
            return res[0] if x2 is None else tuple(res)
        outs, offs = self.plan(lens)
        if not xs:
            res = [[] if width is None else torch.zeros((0, out_length(width, self.p, self.q)), device=self.device)
                   for _ in planes]
            return res[0] if x2 is None else tuple(res)
        sig = torch.stack([torch.cat([t.to(dtype=torch.float32) for t in v]) for v in planes]).contiguous()
        y = self.packed(sig, offs, len(planes))
        wout = None if width is None else out_length(width, self.p, self.q)
        res = [_unpack(list(torch.split(y[k], outs)), outs, wout, self.device) for k in range(len(planes))]
        return res[0] if x2 is None else tuple(res)


def _check(x, lengths):
    """-> (list of 1-D cuda tensors, padded width or None); raises before anything reaches the device"""
    xs, width = _inputs(x, lengths)
    for b, t in enumerate(xs):
        if not t.is_cuda:
            raise L.TrunetHipError("tinyrecurrentunet_amd runs on MI355X only: utterance %d is a %s tensor" % (b, t.device))
        if t.shape[0] < 1:
            raise ValueError("utterance %d is empty" % b)
    return xs, width


def _unpack(ys, lens, width, dev):
    """list of results -> the caller's form: the list itself, or (B, width) with zeros past each length"""
    if width is None:
        return ys
    Y = torch.zeros((len(ys), width), device=dev, dtype=torch.float32)
    for b, (y, n) in enumerate(zip(ys, lens)):
        Y[b, :n] = y
    return Y


_CACHE = {}


def resampler(fs_in, fs_out, device):
    """the cached ``Resampler`` of a ratio and device"""
    key = (int(fs_in), int(fs_out), str(torch.device(device)))
    if key not in _CACHE:
        _CACHE[key] = Resampler(fs_in, fs_out, device)
    return _CACHE[key]


@torch.no_grad()
def resample(x, fs_in, fs_out, lengths=None):
    """x at fs_in -> the same form at fs_out (see the module docstring); ``fs_in == fs_out`` returns copies without a launch"""
    ratio(fs_in, fs_out)
    xs, _ = _check(x, lengths)
    dev = xs[0].device if xs else (x.device if torch.is_tensor(x) and x.is_cuda else torch.device("cuda"))
    return resampler(fs_in, fs_out, dev)(x, lengths)
