"""Rational sample-rate conversion on the GPU: audio at any common rate to the network's 16 kHz and back.

``resample(x, fs_in, fs_out)`` takes the input forms of ``enhance.enhance`` (a list of 1-D fp32 cuda tensors, or a padded
``(B, Lmax)`` tensor with ``lengths``) and returns the same form at ``fs_out``: utterance b of L_b samples becomes
``ceil(L_b p / q)`` samples, ``p / q = fs_out / fs_in`` in lowest terms,

    y[m] = p sum_n h[m q - n p + half] x[n]            (taps and samples outside their ranges count as zero)

which is ``scipy.signal.resample_poly(x, p, q, window=h)`` with ``h`` the Kaiser-windowed sinc of ``design``.  One launch of
``trunet_resample_rational`` (resample.hip) for the whole batch, no device -> host synchronisation: the host builds the
int64 prefix tables (samples in, samples out, tiles) from the lengths and copies them once.  Each utterance's result is bit
for bit independent of its batch-mates, their order and the input form.  No gradients flow through it.

``StreamResampler(fs_in, fs_out, slots)`` is the same filter for sessions that arrive in packets:
per slot it keeps the last K - 1 input samples, and whatever the packet sizes, ``feed`` ... ``feed``, ``close`` return
bit for bit what ``resample`` returns for the whole session.  ``StreamPool(net, slots, fs=...)`` runs one on either side
of the network.

Not here: resampling inside ``AudioStream`` (16 kHz, lockstep, graph-replayable), and ``evaluate``'s own 10 kHz
resampler, which keeps its limits.
"""
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L
from ._lib import check, ptr
from .enhance import _inputs

MAX_RATIO = 640              # 8, 11.025, 12, 22.05, 24, 32, 44.1, 48, 88.2, 96 kHz <-> 16 kHz; worst 11.025 -> 16: 640/441
ZEROS, BETA, ROLLOFF = 16, 8.6, 0.94
# trunet_hip.h: TRUNET_RS_MAX_TILE, TRUNET_RS_SPAN_MAX (floats of input staged per window), TRUNET_RS_TAPS_LDS_MAX (floats of
# the tap table); tests/test_resample_cpu.py compares them with the header
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


def padded_taps(p, half):
    """Kp: K rounded up to a multiple of 4, the floats of one row of the phase table"""
    return (taps_per_output(p, half) + 3) & ~3


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
    return (((tile - 1) * q + p - 1) // p + padded_taps(p, half) + 1 + 3) & ~3


def tile_outputs(p, q, half=None):
    """outputs per workgroup: the largest multiple of 256, at most MAX_TILE, whose input span fits SPAN_FLOATS.  Ratios far
    below 1 (q / p above 16 or so) do not fit even at 256; the kernel then stages the span in windows of SPAN_FLOATS."""
    half = ZEROS * max(p, q) if half is None else half
    room = SPAN_FLOATS - padded_taps(p, half) - 1       # ceil((tile - 1) q / p) must fit it
    return min(max((room * p // q + 1) // 256 * 256, 256), MAX_TILE)


def windows(p, q, half=None):
    """staging windows per tile: 1 whenever the span of tile_outputs(p, q) fits SPAN_FLOATS"""
    return -(-span_floats(p, q, tile_outputs(p, q, half), half) // SPAN_FLOATS)


def taps_in_lds(p, half):
    """whether the kernel keeps the tap table in LDS (it must fit TAPS_LDS_FLOATS) or reads its rows from L2"""
    return p * padded_taps(p, half) <= TAPS_LDS_FLOATS


def lds_bytes(p, q, half=None):
    """LDS one workgroup asks for"""
    half = ZEROS * max(p, q) if half is None else half
    span = min(span_floats(p, q, tile_outputs(p, q, half), half), SPAN_FLOATS)
    return 4 * (span + (p * padded_taps(p, half) if taps_in_lds(p, half) else 0))


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


def _filter(p, q, taps=None):
    """What both resamplers derive from a ratio, host only -> (float64 taps: ``design``'s, or ``taps``, 2 half + 1 of them
    with half a multiple of max(p, q); half; K; outputs per tile; whether the tap table fits LDS)"""
    if taps is None:
        h, half = design(p, q)
    else:
        h = np.asarray(taps, dtype=np.float64)
        half = (h.shape[0] - 1) // 2
        big = max(p, q)
        if h.ndim != 1 or h.shape[0] != 2 * half + 1 or half < big or half % big:
            raise ValueError("taps: 2 half + 1 values with half a positive multiple of max(p, q) = %d" % big)
    return h, half, taps_per_output(p, half), tile_outputs(p, q, half), taps_in_lds(p, half)


def _upload(h, p, device):
    """taps -> the fp32 phase table on the device"""
    return torch.from_numpy(phase_table(h, p).astype(np.float32)).to(device).contiguous()


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
        h, self.half, self.K, self.tile, fits = _filter(self.p, self.q, taps)
        self.lds_taps = fits if lds_taps is None else bool(lds_taps)
        if self.lds_taps and not fits:
            raise ValueError("a table of %d x %d taps does not fit the LDS share of %d floats"
                             % (self.p, padded_taps(self.p, self.half), TAPS_LDS_FLOATS))
        self.table = _upload(h, self.p, self.device)

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


# ---------------------------------------------------------------- streams: the same filter for sessions that arrive in packets
# Host side: plain numpy, no device, no library (tests/test_stream_resample_cpu.py drives it on its own).
STREAM_INTS = 10             # trunet_hip.h: TRUNET_RS_STREAM_INTS
MAX_HISTORY = 20480          # trunet_hip.h: TRUNET_RS_STREAM_MAX_HISTORY (floats per slot)
MAX_SESSION = 2 ** 40        # samples of one session: m q + half stays far inside int64
# table: (n, STREAM_INTS) int64, the records the kernels read; lengths, out_off: outputs each listed session gets and where
# they start in the call's output; received, emitted: per listed session AFTER the call (0 for a closing one); moves:
# whether any history changes (an open session brought samples)
StreamPlan = namedtuple("StreamPlan", "table lengths out_off received emitted n_in n_out n_tiles moves")


def ready(N, p, q, half):
    """Outputs a stream can emit once it has N samples of a session: max(0, ceil((N p - half) / q)).  Output m reads the
    samples nmax - k, k = 0 .. K - 1, nmax = (m q + half) // p, so it is computable once nmax <= N - 1, i.e.
    m q + half < N p.  N may be an array."""
    r = np.maximum(-((half - np.asarray(N, dtype=np.int64) * p) // q), 0)
    return int(r) if r.ndim == 0 else r


def history(p, half):
    """Samples a session keeps between calls: K - 1.  With N samples received the next output is m = ready(N) or later, so
    m q + half >= N p, nmax = (m q + half) // p >= N, and its lowest sample nmax - (K - 1) is at least N - (K - 1).  (While
    ready(N) is still 0 the next output is m = 0 with nmax = half // p >= N, because N p <= half.)"""
    return taps_per_output(p, half) - 1


def plan_stream(received, emitted, lengths, closing, p, q, half, tile, slots=None):
    """What one call owes.  Per listed session i: received[i] samples and emitted[i] outputs BEFORE the call, a packet of
    lengths[i] samples (0 allowed), closing[i]: the session ends with this packet; slots[i]: its state slot (default i).
    An open session gets the outputs below ready(N1), N1 = received + length; a closing one those below ceil(N1 p / q),
    computed with zeros to the right.  A workgroup owns ``tile`` consecutive outputs of one session, counted from the
    session's first output of the call.  ValueError, with nothing changed, for lengths that do not match, a negative
    count, outputs emitted that are not yet ready, and totals beyond int32 packing."""
    n = np.asarray(lengths)
    if n.ndim != 1 or (n.size and n.dtype.kind not in "iu"):
        raise ValueError("packet lengths: a 1-D sequence of integers, got %s %s" % (n.dtype, n.shape))
    n = n.astype(np.int64)
    N0 = np.asarray(received, dtype=np.int64).reshape(-1)
    E0 = np.asarray(emitted, dtype=np.int64).reshape(-1)
    slots = np.arange(n.shape[0], dtype=np.int64) if slots is None else np.asarray(slots, dtype=np.int64).reshape(-1)
    if not (N0.shape == E0.shape == n.shape == slots.shape):
        raise ValueError("%d packet lengths, %d received and %d emitted counts, %d slots"
                         % (n.shape[0], N0.shape[0], E0.shape[0], slots.shape[0]))
    cl = np.asarray(closing, dtype=bool)
    if cl.ndim > 1 or (cl.ndim == 1 and cl.shape != n.shape):
        raise ValueError("%d closing flags for %d sessions" % (cl.size, n.shape[0]))
    cl = np.broadcast_to(cl, n.shape)
    if (n < 0).any() or (N0 < 0).any() or (E0 < 0).any():
        raise ValueError("a count cannot be negative: lengths %s, received %s, emitted %s"
                         % (n.tolist(), N0.tolist(), E0.tolist()))
    if np.unique(slots).shape[0] != slots.shape[0]:
        raise ValueError("a slot is listed twice: %s" % (slots.tolist(),))
    if n.size and max(int(n.max()), int(N0.max())) > MAX_SESSION:       # below it no sum of a call's counts wraps around
        raise ValueError("a session of %d samples: at most 2^40" % max(int(n.max()), int(N0.max())))
    n_in = int(n.sum())
    if n_in > INT32_MAX:
        raise ValueError("%d samples in one call: a call packs fewer than 2^31" % n_in)
    N1 = N0 + n
    if n.size and int(N1.max()) > MAX_SESSION:
        raise ValueError("a session of %d samples: at most 2^40" % int(N1.max()))
    target = np.where(cl, -(-N1 * p // q), ready(N1, p, q, half))
    cnt = target - E0
    if (cnt < 0).any():
        i = int(np.argmax(cnt < 0))
        raise ValueError("session %d has emitted %d outputs and only %d are ready" % (i, E0[i], target[i]))
    n_out = int(cnt.sum())
    if n_out > INT32_MAX:
        raise ValueError("%d outputs in one call: a call packs fewer than 2^31" % n_out)
    tiles = -(-cnt // tile)
    t1 = np.cumsum(tiles)
    out_off = np.cumsum(cnt) - cnt
    table = np.zeros((n.shape[0], STREAM_INTS), dtype=np.int64)
    for c, v in enumerate((slots, N0, np.cumsum(n) - n, n, E0, cnt, out_off, cl, t1 - tiles, t1)):
        table[:, c] = v
    return StreamPlan(table, cnt.tolist(), out_off.tolist(), np.where(cl, 0, N1), np.where(cl, 0, target), n_in, n_out,
                      int(t1[-1]) if n.size else 0, bool(((n > 0) & ~cl).any()))


def _stream_packets(packets, n, dev, what="stream"):
    """packets as ``StreamResampler.feed`` and ``StreamPool.feed`` take them (the one set of refusals of both) -> (list of
    1-D device tensors to concatenate, int64 lengths); host checks only.  ``what`` names the owner of ``dev`` in the message."""
    if isinstance(packets, tuple) and len(packets) == 2 and torch.is_tensor(packets[0]) and not (
            torch.is_tensor(packets[1]) and packets[1].is_cuda):
        flat, lens = packets
        if torch.is_tensor(lens):
            lens = lens.numpy()
        lens = np.asarray(lens)
        if lens.ndim != 1 or (lens.size and lens.dtype.kind not in "iu"):
            raise ValueError("packet lengths: a 1-D sequence of host integers, got %s %s" % (lens.dtype, lens.shape))
        lens = lens.astype(np.int64)
        if (lens < 0).any():
            raise ValueError("a packet cannot have a negative length: %s" % lens[lens < 0].tolist())
        parts, total = [flat], int(lens.sum()) if lens.size else 0
        if flat.dim() != 1 or flat.shape[0] != total:
            raise ValueError("the packed samples: a 1-D tensor of sum(lengths) = %d samples, got %s"
                             % (total, tuple(flat.shape)))
    else:
        if torch.is_tensor(packets) or not isinstance(packets, (list, tuple)):
            raise ValueError("packets: a list of 1-D tensors, or (packed 1-D tensor, lengths), got %s"
                             % type(packets).__name__)
        parts = list(packets)
        for i, t in enumerate(parts):
            if not torch.is_tensor(t) or t.dim() != 1:
                raise ValueError("packet %d: expected a 1-D tensor, got %s"
                                 % (i, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
        lens = np.array([t.shape[0] for t in parts], dtype=np.int64)
    if lens.shape[0] != n:
        raise ValueError("%d packets for %d sessions" % (lens.shape[0], n))
    for i, t in enumerate(parts):
        if not t.is_cuda or t.device != dev:
            raise L.TrunetHipError("tinyrecurrentunet_amd runs on MI355X only: the %s sits on %s, packet %d is a %s tensor"
                                   % (what, dev, i, t.device))
        if not t.dtype.is_floating_point:
            raise ValueError("packet %d: samples are floating point, got %s" % (i, t.dtype))
    return parts, lens


class StreamResampler:
    """fs_in -> fs_out for ``slots`` independent sessions that arrive in packets of any size.

        sr = StreamResampler(fs_in, fs_out, slots, device="cuda")
        outs = sr.feed(packets, ids)    # packets: list of n 1-D fp32 cuda tensors, or (packed, lengths); -> n 1-D views of one buffer
        rest = sr.close(ids)            # the outputs that waited for the right-hand zeros; the slots start afresh
        sr.reset(ids); sr.received(id); sr.emitted(id)

    However a session x of N samples is cut -- empty packets, single samples, everything at once -- the concatenation of
    what ``feed`` returned for it and what ``close`` returns is bit for bit ``resample([x], fs_in, fs_out)[0]``,
    ceil(N p / q) samples: both kernels run resample.hip's one tile function, the streaming one on the line [the slot's
    last K - 1 samples | the packet].  After N samples ``ready(N)`` outputs are out; the rest wait
    for half / p more samples (16 at the lower of the two rates) or for ``close``, which supplies zeros.  ``history``
    derives why K - 1 samples per slot are all the state; the sample and output counts are host integers, and a slot
    whose count is zero reads nothing of its history, so ``reset`` / ``close`` are host work.  One call is one launch of
    trunet_resample_stream for all listed sessions and one of trunet_resample_stream_commit, with one copy of the int64
    plan (``plan_stream``); nothing is read back: no ``.item()``, ``.cpu()`` or ``synchronize``.  Every misuse raises
    before anything reaches the device and leaves all sessions as they were.  ``fs_in == fs_out``: copies, no launch.
    The tap table and the per-slot histories are allocated with the first call that reaches the device."""

    def __init__(self, fs_in, fs_out, slots, device="cuda"):
        self.fs_in, self.fs_out = int(fs_in), int(fs_out)
        self.p, self.q = ratio(fs_in, fs_out)
        if isinstance(slots, bool) or int(slots) != slots or slots < 1:
            raise ValueError("a stream resampler needs at least one slot, got %r" % (slots,))
        self.slots = int(slots)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.TrunetHipError("tinyrecurrentunet_amd runs on MI355X only: StreamResampler on %s" % self.device)
        if self.device.index is None and torch.cuda.is_available():
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.identity = self.p == self.q
        self._recv = np.zeros(self.slots, dtype=np.int64)       # samples received, per slot
        self._emit = np.zeros(self.slots, dtype=np.int64)       # outputs emitted, per slot
        self._table = self._hist = None
        if self.identity:
            self.half = self.K = self.H = 0
            return
        self._h, self.half, self.K, self.tile, self.lds_taps = _filter(self.p, self.q)
        self.H = history(self.p, self.half)
        if self.H > MAX_HISTORY:
            raise ValueError("%d -> %d Hz keeps %d samples per session, and a stream keeps at most %d"
                             % (self.fs_in, self.fs_out, self.H, MAX_HISTORY))

    # ---- device state, made with the first call that needs it
    @property
    def table(self):
        if self._table is None:
            self._table = _upload(self._h, self.p, self.device)
        return self._table

    @property
    def hist(self):
        """(slots, K - 1) fp32: per slot the last K - 1 samples of its session (what lies before sample 0 is not read)"""
        if self._hist is None:
            self._hist = torch.zeros((self.slots, max(self.H, 1)), device=self.device, dtype=torch.float32)
        return self._hist

    # ---- host-side bookkeeping
    def received(self, slot):
        """samples session ``slot`` has received"""
        return int(self._recv[self._ids([slot])[0]])

    def emitted(self, slot):
        """outputs session ``slot`` has been given"""
        return int(self._emit[self._ids([slot])[0]])

    def reset(self, ids):
        """the listed slots start afresh; host work only"""
        ids = self._ids(ids)
        self._recv[ids] = 0
        self._emit[ids] = 0

    def _ids(self, ids):
        """-> int64 array of distinct slots; raises otherwise"""
        if torch.is_tensor(ids):
            if ids.is_cuda:
                raise L.TrunetHipError("slot ids are host data (a list or a CPU integer tensor): a device tensor would have to "
                                       "be read back")
            ids = ids.numpy()
        ids = np.asarray(ids)
        if ids.size == 0:
            return np.zeros(0, dtype=np.int64)
        if ids.ndim != 1 or ids.dtype.kind not in "iu":
            raise ValueError("slot ids: a 1-D sequence of integers, got %s %s" % (ids.dtype, ids.shape))
        ids = ids.astype(np.int64)
        bad = (ids < 0) | (ids >= self.slots)
        if bad.any():
            raise ValueError("not a slot of this stream resampler (%d slots): %s" % (self.slots, ids[bad].tolist()))
        if np.unique(ids).shape[0] != ids.shape[0]:
            raise ValueError("a slot is listed twice: %s" % (ids.tolist(),))
        return ids

    def plan(self, lens, ids, closing=False):
        """the plan of a call for slots ``ids`` (checked, see ``_ids``) with packets of ``lens`` samples; host only, changes
        nothing"""
        if self.identity:
            return plan_stream(self._recv[ids], self._emit[ids], lens, closing, 1, 1, 0, MAX_TILE, ids)
        return plan_stream(self._recv[ids], self._emit[ids], lens, closing, self.p, self.q, self.half, self.tile, ids)

    def run(self, plan, samples, ids):
        """Carry out ``plan``: samples: the packets back to back (1-D fp32 on the device, or None when all are empty) ->
        the outputs back to back (plan.lengths each).  The host counters move only after every launch was accepted."""
        dev = self.device
        if self.identity:
            out = samples.clone() if plan.n_out else torch.empty(0, device=dev, dtype=torch.float32)
        else:
            out = torch.empty(plan.n_out, device=dev, dtype=torch.float32)
            if plan.n_out or plan.moves:
                lib, st = L.lib(), L.stream()
                tab = torch.from_numpy(plan.table).to(dev)                  # ONE copy
                if plan.n_out:
                    check(lib.trunet_resample_stream(ptr(self.hist), ptr(samples), ptr(out), tab.data_ptr(), ptr(self.table),
                                                     self.half, self.K, self.p, self.q, self.tile, len(plan.table),
                                                     self.slots, plan.n_in, plan.n_out, plan.n_tiles, int(self.lds_taps),
                                                     st), "resample_stream")
                if plan.moves:
                    check(lib.trunet_resample_stream_commit(ptr(self.hist), ptr(samples), tab.data_ptr(), self.half, self.K,
                                                            self.p, self.q, len(plan.table), self.slots, plan.n_in, st),
                          "resample_stream_commit")
        self._recv[ids] = plan.received
        self._emit[ids] = plan.emitted
        return out

    @staticmethod
    def _cat(parts, n_in):
        if not n_in:
            return None
        parts = [t for t in parts if t.shape[0]]
        return (parts[0] if len(parts) == 1 else torch.cat(parts)).contiguous().to(dtype=torch.float32)

    @torch.no_grad()
    def feed(self, packets, ids, closing=False):
        """A packet of any length (0 allowed) for each listed slot -> n 1-D tensors (views of one buffer): the outputs of
        each session that became computable with this call, possibly none.  ``closing``: the sessions end with these
        packets (``close`` is ``feed`` of empty packets with ``closing=True``)."""
        ids = self._ids(ids)
        parts, lens = _stream_packets(packets, len(ids), self.device)
        plan = self.plan(lens, ids, closing)
        if not len(ids):
            return []
        out = self.run(plan, self._cat(parts, plan.n_in), ids)
        return list(torch.split(out, plan.lengths))             # the outputs lie back to back in the order of ids

    @torch.no_grad()
    def close(self, ids):
        """End the listed sessions: per session the outputs ready(N) .. ceil(N p / q) - 1, computed with zeros to the right
        of its N samples.  The slots start afresh."""
        ids = self._ids(ids)
        plan = self.plan(np.zeros(len(ids), dtype=np.int64), ids, True)
        if not len(ids):
            return []
        out = self.run(plan, None, ids)
        return list(torch.split(out, plan.lengths))             # the outputs lie back to back in the order of ids
