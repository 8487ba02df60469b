"""Causal audio-in -> audio-out streaming on the HIP path (SURVEY.md 8f ranks 1-2 widened; the protocol the reference
sketches in ``/root/reference/stream.py:83-109``: per audio chunk ``ProcessAudio`` features -> model -> back to audio).

``AudioStream(net, streams)`` carries, per stream, the last 512 input samples, the PCEN smoother ``M`` of
``dataset.py:56-76``, the overlap-add tail of the inverse STFT (``dataset.py:293-296``) and -- with the time-recurrent
block -- the TGRU hidden state.  One hop of 128 new samples per stream costs THREE launches on the current stream:

    trunet_stream_features   ring shift + rect-window rFFT-512 + (norm-dB-mag, [PCEN with carried M], sin, cos)
    trunet_stream_fwd        the whole network in one launch (export.FoldedTRUNet; BatchNorm folded, eval semantics)
    trunet_stream_mask_istft phase-aware mask + irFFT-512 + overlap-add tail -> the 128 samples that are final now

All state tensors keep their addresses, so a captured hipGraph of one steady-state step replays hop after hop.
``AudioStream(..., atten_lim_db=L)`` (a scalar or one value per stream; atten.py) suppresses by at most L
dB: a fourth launch, trunet_atten_blend_rows, blends each emitted hop with its dry samples, which the ring still holds.

The stream reproduces the OFFLINE path of ``util.loss_fn`` (centred STFT with reflect padding, ``dataset.py:260-264``;
``torch.istft``'s envelope normalisation) sample for sample: frame t of the centred STFT covers samples
[128 t - 256, 128 t + 256), so it exists once 128 t + 256 samples have arrived (the first frame needs the reflection of
x[1..256]: nothing is emitted during the first three hops, then frames 0 and 1 at once), and output hop k is final once frame
k + 2 has been overlap-added: an algorithmic latency of four hops (32 ms at 16 kHz), the price of the reference's
512 / 128 analysis.  ``flush()`` feeds the right-hand reflection and returns the remaining hops, so that
``cat(push(...)..., flush())`` has exactly the input's length and equals the offline denoised audio.

``AudioStream`` runs its streams in lockstep: they start in the same call, receive a hop in every call and end in the same
``flush()``.  ``StreamPool(net, slots)`` is the same front end, network and back end for sessions that start, pause and end on
their own -- ``open`` / ``step`` / ``close`` / ``abort`` on a fixed number of state slots -- with utterances of any length
from 257 samples up (``close`` takes the 0..127 samples after the last whole hop) and each session bit for bit independent
of whatever shares its launches.  See the class.
"""
import heapq
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L
from ._lib import check, ptr

N_FFT, HOP, BINS = 512, 128, 257
SAMPLE_RATE = 16000                   # the network's rate (= enhance.SAMPLE_RATE)
PCEN = dict(eps=1e-6, s=0.025, alpha=0.98, delta=2.0, r=0.5)     # dataset.py:56 defaults


class AudioStream:
    def __init__(self, net, streams, tgru=False, beta=0.5, device=None, int8=False, atten_lim_db=None):
        # atten_lim_db: suppress by at most that many dB (atten.py), a scalar or one value per stream,
        # fixed for the life of the object.  None: no limit, nothing is added to a hop
        g = None
        if atten_lim_db is not None:
            from .atten import gains
            g = gains(atten_lim_db, int(streams), "streams")     # refuse before anything reaches the device
        if net.training:
            raise L.TrunetHipError("AudioStream is an inference path: call net.eval() first")
        dev = device if device is not None else next(net.parameters()).device
        if dev.type != "cuda":
            raise L.TrunetHipError("tinyrecurrentunet_amd runs on MI355X only: the network sits on %s" % dev)
        self.net, self.S, self.tgru, self.beta, self.dev = net, int(streams), bool(tgru), float(beta), dev
        self.C = net.encoder[0].StandardConv1d[0].in_channels
        if self.C not in (3, 4):
            raise L.TrunetHipError("features have 3 or 4 channels (R2), the network expects %d" % self.C)
        z = lambda *s: torch.zeros(s, device=dev, dtype=torch.float32)
        self.ring, self.ola = z(self.S, N_FFT), z(self.S, N_FFT)
        self.pcen_M = z(self.S, BINS) if self.C == 4 else None
        self.feat = z(self.S, self.C, BINS)
        # the exported artefact (BatchNorm folded, export.py) is taken HERE: weights are frozen for the life of a stream (no
        # per-hop cache check of the parameters; a new AudioStream picks up new weights)
        # int8=True: the int8 artefact of the same weights (quantize.py; stateless only)
        if int8:
            if self.tgru:
                raise L.TrunetHipError("the int8 artefact covers the stateless forward only: int8=True with tgru=True")
            from .quantize import QuantizedTRUNet
            self.run = QuantizedTRUNet.from_module(net)
        else:
            self.run = net.folded(tgru=self.tgru)
        self.h = self.run.new_state(self.S, dev) if self.tgru else None      # TGRU state (streams, 128, 16)
        self.tw = L.twiddles(N_FFT, dev)
        # the streams' gains at a fixed address, so that a captured hop replays with them
        self.gain = None if g is None else torch.from_numpy(g).to(dev)      # before the first launch: the stream is idle
        self.hops_in = 0                    # hops received
        self.frames = 0                     # STFT frames processed
        self._head = []                     # the first three hops (the reflect-padded first frame needs x[0..256])
        self._flushed = False

    # ---- one STFT frame through the three launches; returns the (S, 128) hop that became final (None: still padding)
    def _frame(self, chunk):
        lib, st = L.lib(), L.stream()
        p = PCEN
        check(lib.trunet_stream_features(ptr(self.ring), ptr(chunk), ptr(self.pcen_M), ptr(self.feat), ptr(self.tw), self.S,
                                         self.C, 1 if self.frames == 0 else 0, p["eps"], p["s"], p["alpha"], p["delta"],
                                         p["r"], st), "stream_features")
        y = self.run.stream_step(self.feat, self.h) if self.tgru else self.run(self.feat)
        t = self.frames
        self.frames += 1
        # frame t completes output hop k = t - 2; the hops of frames 0 and 1 are the centre padding torch.istft trims.
        # env = number of frames that cover the hop: 3 for the first hop of an utterance, 4 in steady state; flush() handles
        # the last hops
        out = torch.empty((self.S, HOP), device=self.dev, dtype=torch.float32)
        env = 4.0 if t >= 3 else float(t + 1)
        check(lib.trunet_stream_mask_istft(ptr(y), ptr(self.ola), ptr(out), ptr(self.tw), self.S, self.beta, env, st),
              "stream_mask_istft")
        if t < 2:
            return None
        # frame t covers samples [128 t - 256, 128 t + 256): the ring starts with the dry samples of hop t - 2
        self._blend(out, 0)
        return out

    def _blend(self, out, ring_off):
        """the attenuation limit on a (S, 128) hop whose dry samples are ring[:, ring_off:ring_off + 128]: one launch"""
        if self.gain is not None:
            check(L.lib().trunet_atten_blend_rows(ptr(out), self.ring.data_ptr() + 4 * ring_off, ptr(self.gain), self.S, HOP,
                                                  HOP, N_FFT, L.stream()), "atten_blend_rows")

    def push(self, chunk):
        """chunk: (streams, 128) new samples per stream (fp32, on the GPU).  Returns (streams, 128 k) denoised samples,
        k = 0 for the first three hops (the analysis window fills), then 1 per hop: the output lags the input by four hops."""
        if self._flushed:
            raise L.TrunetHipError("this stream has been flushed: create a new AudioStream for the next utterance")
        if not chunk.is_cuda:
            raise L.TrunetHipError("tinyrecurrentunet_amd runs on MI355X only: got a %s tensor" % chunk.device)
        chunk = chunk.contiguous().float()
        if tuple(chunk.shape) != (self.S, HOP):
            raise ValueError("expected (%d, %d) samples, got %s" % (self.S, HOP, tuple(chunk.shape)))
        self.hops_in += 1
        outs = []
        with torch.no_grad():
            if self.hops_in <= 3:
                self._head.append(chunk.clone())
                if self.hops_in < 3:
                    return chunk.new_empty((self.S, 0))
                x = torch.cat(self._head, 1)                     # x[0..383]
                self._head = None
                # frame 0 of the centred STFT: [x[256], ..., x[1] | x[0..255]] (reflect padding, dataset.py:260-264)
                self.ring.copy_(torch.cat([x[:, 1:257].flip(1), x[:, :256]], 1))
                outs.append(self._frame(None))
                outs.append(self._frame(x[:, 256:384].contiguous()))   # frame 1 = the ring shifted by one hop
            else:
                outs.append(self._frame(chunk))
        outs = [o for o in outs if o is not None]
        return torch.cat(outs, 1) if outs else chunk.new_empty((self.S, 0))

    def flush(self):
        """End of the utterance (dataset.py:260-264 reflect-pads the right end too): the last two frames and the hops they
        complete; afterwards every input sample has its output sample."""
        if self._flushed:
            return torch.empty((self.S, 0), device=self.dev)
        if self.hops_in < 3:
            raise L.TrunetHipError("an utterance needs at least 3 hops (257 samples) for the reflect padding of its first frame")
        self._flushed = True
        outs = []
        with torch.no_grad():
            # the ring holds x[L-512 .. L-1]; reflection: x[L-2-i], i = 0..255
            tail = self.ring[:, N_FFT - 2 - 255:N_FFT - 1].flip(1).contiguous()      # (S, 256)
            outs.append(self._frame(tail[:, :HOP].contiguous()))
            outs.append(self._frame(tail[:, HOP:].contiguous()))
            # the last hop is covered by three frames only, all of them done: it sits at the head of the overlap-add tail
            last = self.ola[:, :HOP] / 3.0
            self._blend(last, HOP)                              # the ring is x[L - 256, L) and its reflection by now
            outs.append(last)
        outs = [o for o in outs if o is not None]
        return torch.cat(outs, 1)


# ---------------------------------------------------------------- stream pool
# Host side of the pool: plain Python, no device, no library (tests/test_stream_pool_cpu.py drives it on its own).
MIN_SAMPLES = N_FFT // 2 + 1          # = enhance.MIN_SAMPLES: the reflect padding of the first frame needs x[1..256]
ROW_INTS = 8                          # trunet_hip.h: TRUNET_ROW_INTS and the TRUNET_ROW_* flags
ROW_SHIFT, ROW_FIRST, ROW_NOFRAME, ROW_FINISH, ROW_STASHED = 1, 2, 4, 8, 16
CLOSE_OUT_ROWS = 4                    # out rows (of 128 samples) a closing session can fill: 384 + 127 samples at most

# A pass is a table of rows, one STFT frame of one session each (or a hop that is only stored): (n, ROW_INTS) int32, the
# record the kernels read (trunet_hip.h).  Built with numpy, not row by row: a step of a thousand sessions is planned in about 0.1 ms of host time.
#   slot    state slot
#   flags   ROW_SHIFT: the row pushes the session's new hop into its ring; ROW_FIRST: frame 0 (PCEN smoother, overlap-add
#           tail and TGRU state start here; the kernel transforms frames 0 and 1 together, paired as the offline kernels
#           pair them, and keeps frame 1's features for the session's next row, ROW_STASHED); ROW_NOFRAME: store the hop, compute nothing; ROW_FINISH: last frame of the
#           session, the last whole hop (/ 3) and the tail samples (/ 2) follow in out + 1, out + 2
#   frame   frame index t of the session's centred STFT
#   hops    whole hops the session has received, the one of this step included
#   tail    samples after the last whole hop (closing sessions; 0 otherwise)
#   env     number of frames covering the hop this frame completes (hop t - 2; the divisor of torch.istft's envelope)
#   pos     index of the session in the call's id list (= its row of chunks / tails)
#   out     row (of 128 samples) of the call's output the completed hop goes to; -1: the hop is centre padding, dropped
Row = namedtuple("Row", "slot flags frame hops tail env pos out")
# tables: one per pass (a step has <= 2, a close <= 3); frames[k]: the first frames[k] rows of tables[k] compute a frame,
# the rest (ROW_NOFRAME) only store their hop
StepPlan = namedtuple("StepPlan", "tables frames valid hops")       # valid, hops: per listed session, after the step
ClosePlan = namedtuple("ClosePlan", "tables frames lengths")        # lengths: samples each session gets back


def rows_of(table):
    """a pass table as a list of Row"""
    return [Row(*(int(v) for v in r)) for r in table]


def hop_env(k, frames=None):
    """Frames of a centred 512 / 128 STFT that cover output hop k (frames k - 1 .. k + 2, cut to 0 .. frames - 1); k and
    frames may be arrays."""
    hi = k + 2 if frames is None else np.minimum(k + 2, frames - 1)
    return hi - np.maximum(k - 1, 0) + 1


def _table(n, **cols):
    tab = np.zeros((n, ROW_INTS), dtype=np.int32)
    for name, v in cols.items():
        tab[:, Row._fields.index(name)] = v
    return tab


def plan_step(hops, listed):
    """Which frames one ``step`` owes.  hops[slot]: whole hops received BEFORE the step; listed: the slots that get a hop.

    hop count after the step 1, 2: the hop is stored; 3: frames 0 (pass 1, with the shift) and 1 (pass 2), both centre
    padding; >= 4: frame a - 2 in pass 1, completing output hop a - 4.  Slots that are not listed do not appear."""
    listed = np.asarray(listed, dtype=np.int64).reshape(-1)
    a = np.asarray(hops, dtype=np.int64)[listed] + 1
    pos = np.arange(listed.shape[0])
    f, st, third = a >= 3, a < 3, a == 3
    af, t3 = a[f], third[f]
    p1 = _table(int(f.sum()), slot=listed[f], flags=np.where(t3, ROW_SHIFT | ROW_FIRST, ROW_SHIFT),
                frame=np.where(t3, 0, af - 2), hops=af, env=np.where(t3, 1, hop_env(af - 4)), pos=pos[f],
                out=np.where(t3, -1, pos[f]))
    stores = _table(int(st.sum()), slot=listed[st], flags=ROW_SHIFT | ROW_NOFRAME, hops=a[st], pos=pos[st], out=-1)
    p2 = _table(int(third.sum()), slot=listed[third], flags=ROW_STASHED, frame=1, hops=3, env=2, pos=pos[third], out=-1)
    tables, frames = [], []
    if len(p1) or len(stores):
        tables.append(np.concatenate([p1, stores]))
        frames.append(len(p1))
    if len(p2):
        tables.append(p2)
        frames.append(len(p2))
    return StepPlan(tables, frames, a >= 4, a)


def plan_close(hops, tails, slots=None):
    """The frames still missing when sessions end: hops[i] whole hops received, tails[i] = 0..127 samples after them, so
    the utterance has L = 128 a + r samples and T = 1 + L // 128 = a + 1 frames.  a >= 3: frames a - 1 and a (two passes);
    a = 2 with r >= 1: frames 0, 1, 2 (three passes).  Each session gets L - 128 max(a - 3, 0) samples, laid out from row
    CLOSE_OUT_ROWS * i of the output.  ValueError for L < 257, as enhance does."""
    a = np.asarray(hops, dtype=np.int64).reshape(-1)
    r = np.asarray(tails, dtype=np.int64).reshape(-1)
    slots = np.arange(a.shape[0]) if slots is None else np.asarray(slots, dtype=np.int64).reshape(-1)
    if not (a.shape == r.shape == slots.shape):
        raise ValueError("%d hop counts, %d tails, %d slots" % (a.shape[0], r.shape[0], slots.shape[0]))
    if ((r < 0) | (r >= HOP)).any():
        raise ValueError("a tail holds 0..%d samples, got %s" % (HOP - 1, r[(r < 0) | (r >= HOP)].tolist()))
    L = HOP * a + r
    if (L < MIN_SAMPLES).any():
        i = int(np.argmax(L < MIN_SAMPLES))
        raise ValueError("session %d has %d samples; at least %d are needed (reflect padding of the first frame)"
                         % (i, L[i], MIN_SAMPLES))
    pos = np.arange(a.shape[0])
    tables = []
    for k in range(3):
        m = (a == 2) if k == 2 else np.ones(a.shape, dtype=bool)
        am, short = a[m], a[m] == 2
        t = np.where(short, k, am - 1 + k)
        last, emit = t == am, t >= 2
        tab = _table(int(m.sum()), slot=slots[m], flags=np.where(last, ROW_FINISH, 0) | np.where(t == 0, ROW_FIRST, 0) |
                     np.where(short & (t == 1), ROW_STASHED, 0),
                     frame=t, hops=am, tail=r[m], env=np.where(emit, hop_env(t - 2, am + 1), t + 1), pos=pos[m],
                     out=np.where(emit, CLOSE_OUT_ROWS * pos[m] + np.where(short, 0, k), -1))
        if len(tab):
            tables.append(tab)
    return ClosePlan(tables, [len(t) for t in tables], (L - HOP * np.maximum(a - 3, 0)).tolist())


# ---- packets of any size (StreamPool.feed).  A call's plan is three int32 tables that go to the device in ONE copy (trunet_hip.h:
# TRUNET_FEED_INTS and the text above it):
#   rows   one record per STFT frame of the call; record i is feature row i, network row i and frames row i.  Laid out DEPTH-MAJOR:
#          first the first new frame of every session that has one, then the second, ...; sessions are ordered by their number of
#          new frames, most first, so depth d is the contiguous slice depths[d] = (lo, hi) and its sessions are the first hi - lo
#          of `sess` -- what the time-recurrent block needs, one network launch per depth.
#   sess   one record per listed session, in that order (``order[j]``: its position in the call)
#   seq    per session, its frame records in frame order
FEED_INTS = 10                        # trunet_hip.h: TRUNET_FEED_INTS
FEED_MAX_SAMPLES = 0x7fff0000         # trunet_hip.h: TRUNET_FEED_MAX_SAMPLES
INT32_MAX = 2 ** 31 - 1
FeedRow = namedtuple("FeedRow", "slot flags frame off r0 n poff env out pair")
FeedSess = namedtuple("FeedSess", "slot flags seq0 frames adv r0 n poff r1 pos")
# lengths: samples each listed session gets back; hops, pending: per listed session after the call; out_off: the hop of the
# call's output its samples start at; n_active: sessions that have frames (the first n_active records of sess)
FeedPlan = namedtuple("FeedPlan", "rows sess seq depths lengths hops pending out_off n_active n_out n_samples")


def feed_rows_of(table):
    """the frame records of a feed plan as a list of FeedRow"""
    return [FeedRow(*(int(v) for v in r)) for r in table]


def plan_feed(hops, pending, lengths, listed):
    """What one ``feed`` owes.  hops[slot], pending[slot]: whole hops received and samples waiting (0..127) BEFORE the call;
    listed: the slots that bring a packet; lengths[i]: samples in the packet of listed[i] (0 allowed).

    With a1 = (128 a0 + r0 + n) // 128 and r1 = (r0 + n) % 128 a session computes frames 0 and 1 when a1 >= 3 > a0, then
    every frame t with max(a0 - 1, 2) <= t <= a1 - 2, and gets back 128 (max(a1 - 3, 0) - max(a0 - 3, 0)) samples: exactly
    the frames, flags, envelope counts and output order of a1 - a0 calls of ``plan_step``.  ValueError, with nothing
    changed, for a slot listed twice, lengths that do not match the ids, a negative length and totals beyond int32."""
    listed = np.asarray(listed, dtype=np.int64).reshape(-1)
    n = np.asarray(lengths)
    if n.ndim != 1 or n.shape[0] != listed.shape[0]:
        raise ValueError("%d packet lengths for %d sessions" % (n.size if n.ndim == 1 else -1, listed.shape[0]))
    if n.size and n.dtype.kind not in "iu":
        raise ValueError("packet lengths are integers, got %s" % n.dtype)
    n = n.astype(np.int64)
    if (n < 0).any():
        raise ValueError("a packet cannot have a negative length: %s" % n[n < 0].tolist())
    if np.unique(listed).shape[0] != listed.shape[0]:
        raise ValueError("a slot is listed twice: %s" % (listed.tolist(),))
    ns = listed.shape[0]
    a0 = np.asarray(hops, dtype=np.int64)[listed]
    r0 = np.asarray(pending, dtype=np.int64)[listed]
    n_samples = int(n.sum())                                    # python int: no wrap-around
    if n_samples > FEED_MAX_SAMPLES or (ns and int(n.max()) > FEED_MAX_SAMPLES):
        raise ValueError("%d samples in one call: offsets into the packed buffers are int32 (at most %d)"
                         % (n_samples, FEED_MAX_SAMPLES))
    adv = (r0 + n) // HOP
    a1, r1 = a0 + adv, (r0 + n) % HOP
    start = (a0 < 3) & (a1 >= 3)
    lo = np.maximum(a0 - 1, 2)                                  # first steady frame
    emit = np.maximum(a1 - 2 - lo + 1, 0)                       # frames t >= 2: one output hop each
    nfr = emit + 2 * start
    n_rows, n_out = int(nfr.sum()), int(emit.sum())
    if n_rows * 8 * BINS > INT32_MAX:
        raise ValueError("%d frames in one call: offsets into the packed buffers are int32" % n_rows)
    poff, out_off = np.cumsum(n) - n, np.cumsum(emit) - emit
    order = np.argsort(-nfr, kind="stable")                     # most frames first
    fs = nfr[order]
    depth = int(fs[0]) if ns else 0
    cnt = ns - np.searchsorted(fs[::-1], np.arange(depth), side="right")       # sessions with more than d frames
    doff = np.cumsum(cnt) - cnt
    d = np.repeat(np.arange(depth), cnt)                        # per frame record: its depth ...
    j = np.arange(n_rows) - np.repeat(doff, cnt)                # ... and its session (index into order)
    sidx = order[j]
    st = start[sidx]
    t = np.where(st, d, lo[sidx] + d)
    first, second = st & (d == 0), st & (d == 1)
    rows = np.zeros((n_rows, FEED_INTS), dtype=np.int32)
    if n_rows:
        rows[:, 0] = listed[sidx]
        rows[:, 1] = np.where(first, ROW_FIRST, 0) | np.where(second, ROW_STASHED, 0)
        rows[:, 2] = np.minimum(t, INT32_MAX)
        rows[:, 3] = np.where(first, N_FFT - HOP * a0[sidx], HOP * (t - a0[sidx]) + N_FFT // 2)
        rows[:, 4], rows[:, 5], rows[:, 6] = r0[sidx], n[sidx], poff[sidx]
        rows[:, 7] = np.where(t < 2, t + 1, hop_env(t - 2))
        rows[:, 8] = np.where(t >= 2, out_off[sidx] + t - lo[sidx], -1)
        rows[:, 9] = np.where(first, (doff[1] if depth > 1 else 0) + j, -1)
    seq0 = np.cumsum(fs) - fs
    seq = np.zeros(n_rows, dtype=np.int32)
    seq[seq0[j] + d] = np.arange(n_rows)
    sess = np.zeros((ns, FEED_INTS), dtype=np.int32)
    for c, v in enumerate((listed[order], np.where(start[order], ROW_FIRST, 0), seq0, fs, adv[order], r0[order], n[order],
                           poff[order], r1[order], order)):
        sess[:, c] = v
    depths = [(int(o), int(o + c)) for o, c in zip(doff, cnt)]
    return FeedPlan(rows, sess, seq, depths, (HOP * emit).tolist(), a1, r1, out_off, int(cnt[0]) if depth else 0, n_out,
                    n_samples)


class SlotAllocator:
    """Free list of a fixed number of state slots: the lowest free id first, an id is never out twice."""

    def __init__(self, capacity):
        if int(capacity) != capacity or capacity < 1:
            raise ValueError("a pool needs at least one slot, got %r" % (capacity,))
        self.capacity = int(capacity)
        self._free = list(range(self.capacity))
        self.is_open = np.zeros(self.capacity, dtype=bool)          # per slot

    @property
    def free(self):
        return len(self._free)

    def open(self, n=1):
        if int(n) != n or n < 0:
            raise ValueError("open takes a number of sessions, got %r" % (n,))
        if n > len(self._free):
            raise L.TrunetHipError("the pool has %d free slots of %d, %d were asked for" % (len(self._free), self.capacity, n))
        ids = [heapq.heappop(self._free) for _ in range(int(n))]
        self.is_open[ids] = True
        return ids

    def release(self, ids):
        ids = [int(i) for i in ids]
        if len(set(ids)) != len(ids) or any(not 0 <= i < self.capacity or not self.is_open[i] for i in ids):
            raise ValueError("release of a slot that is not open, or twice: %s" % (ids,))
        for i in ids:
            self.is_open[i] = False
            heapq.heappush(self._free, i)


class StreamPool:
    """A fixed number of independent streaming sessions on the single-launch forward.

        pool = StreamPool(net, slots, tgru=None, beta=0.5, int8=False, fs=16000,   # net in eval mode on the GPU; tgru None: net.use_tgru
                          highband="drop", highband_floor_db=-30.0, atten_lim_db=None)
        ids = pool.open(n)                      # n free slot ids
        pool.set_atten_lim(ids, L)              # a pool built with atten_lim_db: move sessions' attenuation limit (dB)
        out, valid = pool.step(chunks, ids)     # chunks (n, 128) fp32 cuda; ids: n distinct open slots
        rest = pool.close(ids, tails)           # list of 1-D tensors; tails[i]: the 0..127 last samples of session i, or None
        pool.abort(ids)                         # drop sessions without output
        pool.free, pool.capacity, pool.hops(id)
        outs = pool.feed(packets, ids)          # packets of ANY size: list of n 1-D fp32 cuda tensors, or (packed, lengths)
        pool.pending(id)                        # samples of a fed session that wait for their hop to fill: 0..127
        rest = pool.close(ids)                  # a fed session's tail is what is pending: no tails needed

    A session that received ``a`` hops and a tail of ``r`` samples is the utterance x of L = 128 a + r samples, and the rows
    of ``out`` where ``valid`` is set followed by ``rest`` are ``net.enhance([x])[0]``: L samples.  Latency as in
    ``AudioStream``: a session's first three steps return a zero row (``valid`` False), step a >= 4 returns output hop a - 4.
    Sessions need not tick together: a slot that is not listed in a step does not advance.

    A step is at most two PASSES and a close at most three (``plan_step`` / ``plan_close``); a pass is one frame for each
    of its rows: upload of the row table (one copy for all passes of the call), trunet_stream_features_rows, the network
    (with ``tgru`` on the rows' states, gathered and scattered back), trunet_stream_mask_istft_rows.  Launches are sized
    by the rows, not by the capacity; idle slots cost nothing.  Per slot the pool keeps the last 512 samples, the PCEN
    smoother, the overlap-add tail and the TGRU state; the first frame of a session overwrites all of them, so nothing of
    a slot's last session reaches the next one.  The kernels transform one real frame per workgroup (frames 0 and 1 of a
    session, owed at the same moment, together: the offline kernels' pairing) and the network
    computes every row on its own: a session's samples do not depend, bit for bit, on the other sessions, the slot ids or
    the capacity.

    ``step`` does not synchronise with the device: no ``.item()``, ``.cpu()``, ``.tolist()`` on a device tensor and no
    ``synchronize``; ``valid`` comes from the host's hop counts.  Slot ids are host data (a list or a CPU integer tensor).
    Every misuse raises before anything reaches the device and leaves all sessions as they were.  The row count changes from
    step to step, so a pool step is not captured as a hipGraph; ``AudioStream`` remains the graph-replayable lockstep path.
    The weights are those of the folded (or int8) artefact taken at construction.

    ``feed`` is the ingress for transports that do not deliver 128-sample units (RTP's 160 or 320 samples, a jitter buffer
    that drains several packets, a second of audio after a stall).  Per slot the pool keeps a FIFO of the 0..127 samples
    that have not filled a hop; a session that had a0 hops and r0 pending samples and gets n more has a1 = (128 a0 + r0 + n)
    // 128 hops and r1 = (r0 + n) % 128 pending, computes frames 0 and 1 when a1 >= 3 > a0 and every frame t with
    max(a0 - 1, 2) <= t <= a1 - 2, and gets back 128 (max(a1 - 3, 0) - max(a0 - 3, 0)) samples.  However the utterance is
    cut -- empty packets, single samples, everything at once -- the samples are bit for bit those of ``step`` /
    ``close(tails)``: the kernels share the per-element expressions and keep their order.  All new frames
    of all listed sessions go through ONE pass (``plan_feed``): trunet_stream_feed_features (a workgroup per frame),
    trunet_stream_feed_commit (per session: PCEN in frame order, ring and FIFO move on), the network on all rows at once
    (with ``tgru``: once per burst depth, the rows laid out depth-major so that each launch reads a contiguous slice; at most
    ``net.fold_max_frames`` rows per launch either way), trunet_stream_feed_mask_istft (per frame), trunet_stream_feed_ola
    (per session: overlap-add in frame order).  No synchronisation with the device, one copy of the plan per call.  ``step``
    and ``feed`` may alternate on a session while nothing is pending; ``step``, or ``close`` with a tail, on a session with
    pending samples is a ValueError that changes nothing.

    ``fs`` (``pool.fs``): the sample rate of the packets ``feed`` takes and returns, 8 to 96 kHz (``resample.ratio``).  At
    another rate than 16 kHz the pool owns two ``resample.StreamResampler`` over its slots, ``fs`` -> 16 kHz and back
    (DESIGN section 3m): ``feed`` down-resamples the packets, runs the 16 kHz pass above on what became ready and
    up-resamples what it returned; ``close(ids)`` flushes the down-resampler into a last 16 kHz feed, runs the 16 kHz
    close, pushes both results through the up-resampler, closes it and cuts each session to the number of samples it was
    fed (``enhance``'s rule at another rate).  A session of L samples at ``fs`` is bit for bit
    ``resample(ys16, 16000, fs)[:L]``, ``ys16`` what a 16 kHz pool returns for ``resample(x, fs, 16000)``, however it is
    cut into packets, and needs ceil(L 16000 / fs) >= 257: ``close`` raises ValueError below that, and the session and its
    call-mates stay open and unchanged.  Each resampler adds a look-ahead of 16 samples at the lower of its two rates (1
    ms each way at 48 kHz) to the four hops of the 16 kHz path.  ``step`` and ``close`` with a non-empty tail take 16
    kHz hops and are a ValueError at another rate; ``pending`` and ``hops`` keep their 16 kHz meaning; ``open`` and
    ``abort`` reset both resamplers' counters of the slot.  With the default ``fs`` nothing changes.  ``AudioStream`` stays
    at 16 kHz.

    ``highband`` (keyword only; ``pool.highband``, ``pool.highband_floor_db``): what becomes of the band above 8 kHz when
    ``fs`` > 16 kHz.  ``"drop"``, the default: the pool above, bit for bit, with no further allocation or
    launch; the two low-passes leave nothing above 0.94 of 8 kHz.  ``"keep"``: out = up_y + (x - up_x), with up_x the
    session's own down-resampled samples resampled back; however the packets are cut, ``feed`` ... ``close`` is bit for bit
    ``highband.rejoin([x], [lo], [ys16], fs, "keep")[0]``.  ``"follow"``: out[n] = up_y[n] + G[n] (x[n] - up_x[n]) with a
    CAUSAL gain, the square root of the ratio of the energies of the enhanced and the incoming 16 kHz signal above 4 kHz
    (63-tap high-pass, 2 ms late) over the four hops that end where sample n is emitted, clamped to
    [10^(highband_floor_db / 20), 1] and interpolated from hop to hop.  That gain trails the suppression it follows by about
    two hops plus the filter's 2 ms; it is a definition of its own (``stream_highband``'s docstring, pinned in float64 by
    tests/stream_highband_ref.py), not the offline ``"follow"``, which looks two hops ahead and would cost 32 ms.  Neither
    mode adds latency: ``feed`` returns, call by call, the sample counts of ``"drop"``.  Per slot the pool then also keeps
    the samples at ``fs`` fed and not yet returned (at most 543 fs / 16000), the samples at 16 kHz that the network has not
    returned (at most 511), a third stream resampler plane and, for ``"follow"``, 62 samples of either 16 kHz signal, three
    block energies and two gains; ``open`` and ``abort`` reset their counters, host work only.  A mode outside
    ``highband.MODES`` and a floor outside (-inf, 0] are a ValueError before anything reaches the device; at ``fs`` <= 16 kHz
    the arguments are validated and the pool is that of ``"drop"``; a rate whose per-slot line cannot be bounded inside
    4096 samples (above 120 kHz) is refused at construction.  ``step`` and ``close`` with a tail stay a ValueError at these
    rates.

    ``atten_lim_db`` (keyword only; ``pool.atten_lim_db``): the attenuation limit a session opens with (atten.py, DESIGN
    section 3s): every 16 kHz sample the pool returns becomes y + g (x - y), g = 10^(-L / 20), y the enhanced and x the input
    sample.  None, the default: the pool above bit for bit, with no blend stage, no allocation and no launch of it.  A pool
    built with a limit (``inf`` for "none yet") takes ``pool.set_atten_lim(ids, L)`` for open sessions at any time: over the
    first hop a session emits after the call its gain goes linearly from the old value to the new one, so where the ramp
    lies follows from the samples fed so far, not from how they were cut into packets; a session whose frame 0 is still to
    come starts at the new value, and a slot's next session at the pool's limit again.  Per slot the pool then also keeps a
    dry line, the samples fed and not yet returned (at most 511), the gain the session last emitted with and its target;
    ``step``, ``feed`` and ``close`` add ONE launch each (trunet_stream_atten, after the overlap-add; two in a ``close`` at
    another rate), its records travel with the call's plan, and ``set_atten_lim`` is one copy of the slots' targets.  The
    blend sits in the 16 kHz pass: at another ``fs`` the up-resampler, ``"keep"`` and the ``"follow"`` gain read the blended
    signal.  Everything above holds with a limit: packets do not matter, pool-mates and their limits do not matter."""

    def __init__(self, net, slots, tgru=None, beta=0.5, int8=False, fs=SAMPLE_RATE, *, highband="drop",
                 highband_floor_db=-30.0, atten_lim_db=None):
        from . import atten as AT
        from . import highband as HB
        HB.check_args(highband, highband_floor_db)               # before anything touches the network or the device
        if atten_lim_db is not None:
            AT.gain(atten_lim_db)
        if net.training:
            raise L.TrunetHipError("StreamPool is an inference path: call net.eval() first")
        dev = next(net.parameters()).device
        if dev.type != "cuda":
            raise L.TrunetHipError("tinyrecurrentunet_amd runs on MI355X only: the network sits on %s" % dev)
        self._host_init(slots, fs, dev, highband, highband_floor_db, atten_lim_db)
        self.tgru = bool(net.use_tgru if tgru is None else tgru)
        self.net, self.beta, self.dev = net, float(beta), dev
        self.C = net.encoder[0].StandardConv1d[0].in_channels
        if self.C not in (3, 4):
            raise L.TrunetHipError("features have 3 or 4 channels (R2), the network expects %d" % self.C)
        if int8:
            if self.tgru:
                raise L.TrunetHipError("the int8 artefact covers the stateless forward only: int8=True with tgru=True")
            from .quantize import QuantizedTRUNet
            self.run = QuantizedTRUNet.from_module(net)
        else:
            self.run = net.folded(tgru=self.tgru)
        S = self._alloc.capacity
        z = lambda *s: torch.zeros(s, device=dev, dtype=torch.float32)
        self.ring, self.ola = z(S, N_FFT), z(S, N_FFT)
        self.pcen_M = z(S, BINS) if self.C == 4 else None
        self.stash = z(S, self.C, BINS)                          # frame 1's features between a session's first two passes
        self.h = self.run.new_state(S, dev) if self.tgru else None           # TGRU state (slots, 128, 16)
        self.fifo = z(S, HOP)                                    # feed(): the 0..127 samples that wait for their hop to fill
        self.tw = L.twiddles(N_FFT, dev)

    def _host_init(self, slots, fs, dev, highband="drop", highband_floor_db=-30.0, atten_lim_db=None):
        """the host side of a pool: the slot allocator, the per-slot counters and, at another rate than 16 kHz, the two
        stream resamplers (whose device buffers come with their first launch); above 16 kHz with ``highband`` "keep" or
        "follow", the state that carries the band above 8 kHz; with ``atten_lim_db`` the gain a session
        opens with and the host's copy of every slot's target gain (section 3s).  No device work."""
        from . import atten as AT
        from . import highband as HB
        from . import resample as R
        self.highband, self.highband_floor_db = HB.check_args(highband, highband_floor_db)
        self.atten_lim_db = atten_lim_db
        self._g_open = None if atten_lim_db is None else AT.gain(atten_lim_db)
        R.ratio(fs, SAMPLE_RATE)
        self._alloc = SlotAllocator(slots)
        S = self._alloc.capacity
        self.fs, self.dev = int(fs), dev
        self._hops = np.zeros(S, dtype=np.int64)
        self._pend = np.zeros(S, dtype=np.int64)                 # samples in the FIFO, per slot
        self._down = self._up = self._hb = None
        # the attenuation limit: target gain per slot (host copy; the device's is brought up to date before it is read),
        # and the device state (dry line, current and target gain per slot), which comes with the first launch
        self._g_tgt = None if self._g_open is None else np.full(S, self._g_open, dtype=np.float32)
        self._g_stale, self._att_state = self._g_open is not None, None
        if self.fs != SAMPLE_RATE:
            self._down = R.StreamResampler(self.fs, SAMPLE_RATE, S, dev)
            self._up = R.StreamResampler(SAMPLE_RATE, self.fs, S, dev)
        if self.fs > SAMPLE_RATE and self.highband != "drop":    # at or below 16 kHz nothing lies above the network's band
            from .stream_highband import StreamHighband
            self._hb = StreamHighband(self.fs, S, self.highband, self.highband_floor_db, dev)

    # ---- host-side bookkeeping
    @property
    def capacity(self):
        return self._alloc.capacity

    @property
    def free(self):
        return self._alloc.free

    def hops(self, slot):
        """whole hops session ``slot`` has received"""
        return int(self._hops[self._ids([slot])[0]])

    def pending(self, slot):
        """samples of session ``slot`` that wait for their hop to fill (``feed``): 0..127, a host value"""
        return int(self._pend[self._ids([slot])[0]])

    def open(self, n=1):
        """n new sessions -> their slot ids; raises when fewer than n slots are free.  Host work only: the first frame of a
        session overwrites the slot's state."""
        ids = self._alloc.open(n)
        for i in ids:
            self._hops[i] = 0
            self._pend[i] = 0
        if self._g_open is not None and len(ids):               # a session opens with the pool's limit, whatever the
            self._g_tgt[ids] = self._g_open                      # slot's last session was given
            self._g_stale = True
        self._reset_rate(ids)
        return ids

    # ---- the attenuation limit
    def set_atten_lim(self, ids, atten_lim_db):
        """Move the limit of open sessions while they run: ids n distinct open slots, atten_lim_db a scalar or one value per
        id (dB >= 0 or inf).  Over the first hop a session emits after the call its gain goes linearly from the old value to
        the new one, then stays there; a session whose frame 0 is still to come starts at the new value.  One small host
        -> device copy (the slots' target gains), no synchronisation.  ValueError, with nothing changed, for a pool built
        without ``atten_lim_db`` (it has no blend stage), ids that are not open and values ``atten.gain`` refuses."""
        from . import atten as AT
        if self._g_open is None:
            raise ValueError("this pool was built without atten_lim_db and has no blend stage: give StreamPool a limit "
                             "(inf for none) to move it per session")
        ids = self._ids(ids)
        g = AT.gains(atten_lim_db, len(ids), "sessions")
        if not len(ids):
            return
        self._g_tgt[ids] = g
        self._g_stale = True
        self._push_targets()

    def _att(self):
        """the per-slot device state of the blend stage: dry line, current gain, target gain"""
        from . import atten as AT
        if self._att_state is None:
            S, z = self.capacity, lambda *s: torch.zeros(s, device=self.dev, dtype=torch.float32)
            self._att_state = (z(S, AT.DRY_LINE), z(S), z(S))
        return self._att_state

    def _push_targets(self):
        """the slots' target gains, host -> device, when the host's copy has moved: staged in pinned memory of its own and
        copied asynchronously, so the host does not wait for the stream and a later change cannot reach an earlier copy"""
        if self._g_stale:
            self._att()[2].copy_(torch.from_numpy(self._g_tgt).pin_memory(), non_blocking=True)
            self._g_stale = False

    def _dry_count(self, ids):
        """samples of each listed session fed and not yet returned: a hop comes back four hops after it arrived"""
        return HOP * np.minimum(self._hops[ids], 3) + self._pend[ids]

    # the blend stage's records of a call (``atten.plan_atten``), host only, from the counters BEFORE the call; None for a
    # pool without a limit
    def _att_step(self, ids, plan):
        """``step``: the hop that came is the packet, row pos of (n, 128) the output where valid; frame 0 at hop three"""
        if self._g_open is None:
            return None
        from .atten import plan_atten
        at = HOP * np.arange(len(ids))
        return plan_atten(ids, self._dry_count(ids), at, np.full(len(ids), HOP), at, HOP * plan.valid, plan.hops == 3, False)[0]

    def _att_feed(self, plan):
        """``feed``: one record per session in the order of ``plan.sess``; None also for a call that moves nothing"""
        if self._g_open is None or not (plan.n_samples or plan.n_out):
            return None
        from .atten import plan_atten
        sl, order = plan.sess[:, 0].astype(np.int64), plan.sess[:, 9].astype(np.int64)
        return plan_atten(sl, self._dry_count(sl), plan.sess[:, 7], plan.sess[:, 6], HOP * np.asarray(plan.out_off)[order],
                          np.asarray(plan.lengths, dtype=np.int64)[order], (plan.sess[:, 1] & ROW_FIRST) != 0, False)[0]

    def _att_close(self, ids, plan, tails, rs):
        """``close``: the packet is row i of the (n, 128) tails, read only for a tail that was given (a fed session's
        already waits in its dry line); the output row i of (n, 512); frame 0 for a session of two hops"""
        if self._g_open is None:
            return None
        from .atten import plan_atten
        n = len(ids)
        return plan_atten(ids, self._dry_count(ids), HOP * np.arange(n), [0 if t is None else r for t, r in zip(tails, rs)],
                          CLOSE_OUT_ROWS * HOP * np.arange(n), plan.lengths, self._hops[ids] < 3, True)[0]

    def _atten(self, table, packet, n_packet, out, n_out):
        """trunet_stream_atten over the records ``table`` (device, ``atten.plan_atten``): the call's output, blended in
        place, and the slots' dry lines and current gains moved on.  One launch."""
        dry, g_cur, g_tgt = self._att()
        self._push_targets()
        check(L.lib().trunet_stream_atten(ptr(out) if n_out else None, ptr(dry), ptr(g_cur), ptr(g_tgt),
                                          ptr(packet) if n_packet else None, table.data_ptr(), table.shape[0], self.capacity,
                                          n_packet, n_out, L.stream()), "stream_atten")

    def abort(self, ids):
        """Drop sessions without output; the slots are free again."""
        ids = self._ids(ids)
        self._alloc.release(ids)
        self._reset_rate(ids)

    def _reset_rate(self, ids):
        """another rate than 16 kHz: both resamplers' counters of the slots start at zero, and a slot whose count is zero
        reads nothing of its history -- a session never sees the samples of the one before it"""
        if self._down is not None and len(ids):
            self._down.reset(ids)
            self._up.reset(ids)
            if self._hb is not None:
                self._hb.reset(ids)

    def _ids(self, ids):
        """-> int64 array of distinct open slots; raises otherwise"""
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
        bad = (ids < 0) | (ids >= self.capacity)
        bad |= ~self._alloc.is_open[np.where(bad, 0, ids)]
        if bad.any():
            raise ValueError("not an open session of this pool: slot %s" % ids[bad].tolist())
        if np.unique(ids).shape[0] != ids.shape[0]:
            raise ValueError("a slot is listed twice: %s" % (ids.tolist(),))
        return ids

    # ---- one pass: one frame for each row
    def _pass(self, rows, table, nf, chunks, n_chunks, out, n_out):
        """rows: the pass table on the device, table: the same on the host; its first nf rows compute a frame"""
        lib, st, p = L.lib(), L.stream(), PCEN
        feat = torch.empty((nf, self.C, BINS), device=self.dev, dtype=torch.float32) if nf else None
        check(lib.trunet_stream_features_rows(ptr(self.ring), ptr(chunks), ptr(self.pcen_M), ptr(self.stash), ptr(feat),
                                              rows.data_ptr(),
                                              len(table), nf, n_chunks, self.capacity, ptr(self.tw), self.C, p["eps"], p["s"],
                                              p["alpha"], p["delta"], p["r"], st), "stream_features_rows")
        if not nf:
            return
        if self.tgru:
            idx = rows[:nf, 0].long()
            h = self.h.index_select(0, idx)
            if (table[:nf, 1] & ROW_FIRST).any():               # h0 = 0 like nn.GRU, whatever the slot's last session left
                h.masked_fill_(((rows[:nf, 1] & ROW_FIRST) != 0)[:, None, None], 0.0)
            y = self.run.stream_step(feat, h)
            self.h.index_copy_(0, idx, h)
        else:
            y = self.run(feat)
        check(lib.trunet_stream_mask_istft_rows(ptr(y), ptr(self.ola), ptr(out), rows.data_ptr(), nf, n_out, self.capacity,
                                                ptr(self.tw), self.beta, st), "stream_mask_istft_rows")

    def _run_passes(self, plan, chunks, n_chunks, out, n_out, att=None):
        """att: the records of the blend stage (``atten.plan_atten``; they travel with the row tables), or None"""
        tabs = plan.tables if att is None else plan.tables + [att]
        dev_tab = torch.from_numpy(np.concatenate(tabs)).to(self.dev)           # the row tables of every pass: ONE copy
        r0 = 0
        for table, nf in zip(plan.tables, plan.frames):
            self._pass(dev_tab[r0:r0 + len(table)], table, nf, chunks, n_chunks, out, n_out)
            r0 += len(table)
        if att is not None:
            self._atten(dev_tab[r0:], chunks, n_chunks * HOP, out, n_out * HOP)

    @torch.no_grad()
    def step(self, chunks, ids):
        """One hop of 128 new samples for each listed session: chunks (n, 128) fp32 on the pool's device, ids n distinct open
        slots.  Returns (out (n, 128), valid (n,) CPU bool): row i is session ids[i]'s next 128 denoised samples where
        valid[i], zeros otherwise (its first three hops).  Never synchronises with the device."""
        ids = self._ids(ids)
        if self._down is not None:
            raise ValueError("step() takes hops of 128 samples at %d Hz; this pool runs at %d Hz, where feed() is the ingress"
                             % (SAMPLE_RATE, self.fs))
        if not torch.is_tensor(chunks):
            raise ValueError("chunks: a (%d, %d) tensor, got %s" % (len(ids), HOP, type(chunks).__name__))
        if not chunks.is_cuda or chunks.device != self.dev:
            raise L.TrunetHipError("tinyrecurrentunet_amd runs on MI355X only: the pool sits on %s, got a %s tensor"
                                   % (self.dev, chunks.device))
        if tuple(chunks.shape) != (len(ids), HOP):
            raise ValueError("expected (%d, %d) samples, got %s" % (len(ids), HOP, tuple(chunks.shape)))
        self._no_pending(ids, "step() takes whole hops")
        out = torch.zeros((len(ids), HOP), device=self.dev, dtype=torch.float32)
        if not len(ids):
            return out, torch.zeros(0, dtype=torch.bool)
        chunks = chunks.contiguous().float()
        plan = plan_step(self._hops, ids)
        self._run_passes(plan, chunks, len(ids), out, len(ids), self._att_step(ids, plan))
        self._hops[ids] = plan.hops
        return out, torch.from_numpy(plan.valid)

    # ---- packets of any size
    def _no_pending(self, ids, what):
        bad = self._pend[ids] != 0
        if bad.any():
            raise ValueError("%s: session %s has pending samples from feed() (%s); go on with feed(), or close()"
                             % (what, ids[bad].tolist(), self._pend[ids][bad].tolist()))

    def _packets(self, packets, n):
        """-> (list of 1-D device tensors to concatenate, int64 lengths); host checks only, the stream resampler's own"""
        from . import resample as R
        return R._stream_packets(packets, n, self.dev, "pool")

    def _net_rows(self, feat, rows, lo, hi, first):
        """the network on feature rows [lo, hi), at most net.fold_max_frames per launch; with the time-recurrent block the
        rows are one frame each of distinct sessions and their slots' states step with them"""
        step = max(int(self.net.fold_max_frames), 1)
        ys = []
        for b in range(lo, hi, step):
            e = min(b + step, hi)
            if self.tgru:
                idx = rows[b:e, 0].long()
                h = self.h.index_select(0, idx)
                if first:                                       # h0 = 0 like nn.GRU, whatever the slot's last session left
                    h.masked_fill_(((rows[b:e, 1] & ROW_FIRST) != 0)[:, None, None], 0.0)
                ys.append(self.run.stream_step(feat[b:e], h))
                self.h.index_copy_(0, idx, h)
            else:
                ys.append(self.run(feat[b:e]))
        return ys

    @torch.no_grad()
    def feed(self, packets, ids):
        """A packet of ANY length (0 allowed) for each listed session: packets is a list of n 1-D fp32 tensors on the pool's
        device, or a pair (packed 1-D tensor, lengths as host integers); ids n distinct open slots.  Returns n 1-D tensors
        (views of one buffer): the denoised samples of each session that became final with this call, possibly none.

        However an utterance is cut into packets, what ``feed`` returned for it, concatenated and followed by ``close(ids)``,
        is bit for bit the ``step`` / ``close(tails)`` result.  Samples that do not fill a hop wait in the slot's FIFO
        (``pending``); ``step`` and ``feed`` may alternate while nothing is pending.  Never synchronises with the device;
        the plan of the call goes up in one copy."""
        ids = self._ids(ids)
        parts, lens = self._packets(packets, len(ids))
        if self._down is not None:
            return self._feed_at(parts, lens, ids)
        plan = plan_feed(self._hops, self._pend, lens, ids)
        if not len(ids):
            return []
        out = self._feed16(plan, parts, ids)
        return [out[HOP * int(o):HOP * int(o) + m] for o, m in zip(plan.out_off, plan.lengths)]

    def _feed16(self, plan, parts, ids):
        """the device side of ``feed``: the 16 kHz pass of ``plan`` over the packets ``parts`` -> the call's output, the
        sessions' new samples back to back in the order of ``ids``"""
        lib, st, p, dev = L.lib(), L.stream(), PCEN, self.dev
        n_rows, n_sess, S = len(plan.rows), len(plan.sess), self.capacity
        samples = None
        if plan.n_samples:
            parts = [t for t in parts if t.shape[0]]
            samples = (parts[0] if len(parts) == 1 else torch.cat(parts)).contiguous().float()
        host_tabs, att = [plan.rows.reshape(-1), plan.sess.reshape(-1), plan.seq], self._att_feed(plan)
        if att is not None:                                     # the blend stage's records travel with the plan
            host_tabs.append(att.reshape(-1))
        tab = torch.from_numpy(np.concatenate(host_tabs)).to(dev)              # ONE copy
        rows = tab[:n_rows * FEED_INTS].view(n_rows, FEED_INTS)
        sess = tab[n_rows * FEED_INTS:(n_rows + n_sess) * FEED_INTS]
        seq = tab[(n_rows + n_sess) * FEED_INTS:(n_rows + n_sess) * FEED_INTS + n_rows]
        prow, pseq = (rows.data_ptr(), seq.data_ptr()) if n_rows else (None, None)
        feat = None
        if n_rows:
            feat = torch.empty((n_rows, self.C, BINS), device=dev, dtype=torch.float32)
            check(lib.trunet_stream_feed_features(ptr(self.ring), ptr(self.fifo), ptr(samples), ptr(feat), prow, n_rows,
                                                  plan.n_samples, S, ptr(self.tw), self.C, st), "stream_feed_features")
        check(lib.trunet_stream_feed_commit(ptr(self.ring), ptr(self.fifo), ptr(samples), ptr(self.pcen_M), ptr(feat), prow,
                                            sess.data_ptr(), pseq, n_sess, n_rows, plan.n_samples, S, self.C, p["eps"], p["s"],
                                            p["alpha"], p["delta"], p["r"], st), "stream_feed_commit")
        out = torch.empty(plan.n_out * HOP, device=dev, dtype=torch.float32)
        if n_rows:
            if self.tgru:                                       # one launch per burst depth: the d-th new frame of every session
                ys = [y for d, (lo, hi) in enumerate(plan.depths) for y in self._net_rows(feat, rows, lo, hi, d == 0)]
            else:                                               # frames are independent: all of them at once
                ys = self._net_rows(feat, rows, 0, n_rows, False)
            y = ys[0] if len(ys) == 1 else torch.cat(ys)
            frames = torch.empty((n_rows, N_FFT), device=dev, dtype=torch.float32)
            check(lib.trunet_stream_feed_mask_istft(ptr(y), ptr(frames), n_rows, ptr(self.tw), self.beta, st),
                  "stream_feed_mask_istft")
            check(lib.trunet_stream_feed_ola(ptr(frames), ptr(self.ola), ptr(out) if plan.n_out else None, prow,
                                             sess.data_ptr(), pseq, plan.n_active, n_rows, plan.n_out, S, st),
                  "stream_feed_ola")
        if att is not None:
            self._atten(tab[(n_rows + n_sess) * FEED_INTS + n_rows:].view(n_sess, -1), samples, plan.n_samples, out,
                        plan.n_out * HOP)
        self._hops[ids] = plan.hops
        self._pend[ids] = plan.pending
        return out

    # ---- another rate than 16 kHz: a stream resampler on either side of the 16 kHz pass
    def _plan_feed_at(self, lens, ids):
        """the plans of a ``feed`` at ``fs``, host only: down, 16 kHz, up and (or None) the band above 8 kHz"""
        down, up, hb = self._down, self._up, self._hb
        pd = down.plan(lens, ids)
        p16 = plan_feed(self._hops, self._pend, np.asarray(pd.lengths, dtype=np.int64), ids)
        pu = up.plan(np.asarray(p16.lengths, dtype=np.int64), ids)
        ph = None if hb is None else hb.plan(ids, lens, pd.lengths, p16.lengths, pu, up._emit[ids])
        return pd, p16, pu, ph

    def _plan_close_at(self, ids):
        """the plans of a ``close`` at ``fs``, host only -> (down, 16 kHz feed, 16 kHz close, up, band above 8 kHz or None,
        samples each session still gets); ValueError for a session below 257 samples at 16 kHz"""
        down, up, hb = self._down, self._up, self._hb
        fed = down._recv[ids].copy()
        pd = down.plan(np.zeros(len(ids), dtype=np.int64), ids, True)
        L16 = HOP * self._hops[ids] + self._pend[ids] + np.asarray(pd.lengths, dtype=np.int64)     # = ceil(fed p / q)
        if (L16 < MIN_SAMPLES).any():
            i = int(np.argmax(L16 < MIN_SAMPLES))
            raise ValueError("session %d has %d samples at %d Hz, %d at %d Hz; at least %d are needed there (reflect padding "
                             "of the first frame)" % (ids[i], fed[i], self.fs, L16[i], SAMPLE_RATE, MIN_SAMPLES))
        p16 = plan_feed(self._hops, self._pend, np.asarray(pd.lengths, dtype=np.int64), ids)
        pc = plan_close(p16.hops, p16.pending, ids)
        both = np.asarray(p16.lengths, dtype=np.int64) + np.asarray(pc.lengths, dtype=np.int64)
        pu = up.plan(both, ids, True)
        owed = np.minimum(np.asarray(pu.lengths, dtype=np.int64), fed - up._emit[ids])
        ph = None if hb is None else hb.plan(ids, np.zeros(len(ids), dtype=np.int64), pd.lengths, both, pu, up._emit[ids],
                                             owed, True)
        return pd, p16, pc, pu, ph, owed

    def _feed_at(self, parts, lens, ids):
        """``feed`` at ``fs``: down-resample, the 16 kHz pass on what became ready, up-resample what it returned, and with
        ``highband`` rejoin the band above 8 kHz.  All plans are made before the first launch, so a refusal leaves every
        session as it was."""
        down, up, hb = self._down, self._up, self._hb
        pd, p16, pu, ph = self._plan_feed_at(lens, ids)
        if not len(ids):
            return []
        packet = down._cat(parts, pd.n_in)
        x16 = down.run(pd, packet, ids)
        y16 = self._feed16(p16, [x16], ids)
        y = up.run(pu, y16 if pu.n_in else None, ids)
        if hb is not None:                                      # the band above 8 kHz rejoins what came back (section 3r)
            y = hb.run(ph, pu, packet, x16 if pd.n_out else None, y16 if pu.n_in else None, y, ids)
        return list(torch.split(y, pu.lengths))                 # back to back in the order of ids

    def _close_at(self, ids, tails):
        """``close`` at ``fs``: the down-resampler's last outputs go through a last 16 kHz feed, the 16 kHz close follows, and
        the up-resampler closes on both; each session is cut to the number of samples it was fed (``enhance``'s rule at
        another rate: ceil(ceil(L p / q) q / p) >= L, so there is always enough to cut)."""
        tails = None if tails is None else list(tails)
        if tails is not None and len(tails) != len(ids):
            raise ValueError("%d tails for %d sessions" % (len(tails), len(ids)))
        if tails is not None and any(t is not None and (not torch.is_tensor(t) or t.numel()) for t in tails):
            raise ValueError("close() takes tails at %d Hz; this pool runs at %d Hz, where feed() is the ingress and the "
                             "samples that wait are the tail" % (SAMPLE_RATE, self.fs))
        down, up, hb = self._down, self._up, self._hb
        pd, p16, _, pu, ph, owed = self._plan_close_at(ids)
        if not len(ids):
            return []
        x16 = down.run(pd, None, ids)
        a = self._feed16(p16, [x16], ids)
        b = self._close16(ids, [None] * len(ids))
        pieces = []
        for i, (o, m) in enumerate(zip(p16.out_off, p16.lengths)):
            pieces += [a[HOP * int(o):HOP * int(o) + m], b[i]]
        y16 = torch.cat(pieces)
        y = up.run(pu, y16, ids)
        if hb is not None:
            y = hb.run(ph, pu, None, x16 if pd.n_out else None, y16, y, ids)
        return [y[o:o + int(m)] for o, m in zip(pu.out_off, owed)]

    @torch.no_grad()
    def close(self, ids, tails=None):
        """End sessions: tails[i] (None, or a 1-D fp32 tensor of 0..127 samples on the pool's device) are the samples after
        session i's last whole hop.  A session with pending samples from ``feed`` has them as its tail already: ``close(ids)``;
        giving it a tail as well is a ValueError.  Returns, per session, the L - 128 max(a - 3, 0) samples not yet delivered,
        and frees the slots.  ValueError for a session of fewer than 257 samples; it stays open, like every other session of
        the call."""
        ids = self._ids(ids)
        if self._down is not None:
            return self._close_at(ids, tails)
        return self._close16(ids, tails)

    def _close16(self, ids, tails):
        tails = [None] * len(ids) if tails is None else list(tails)
        if len(tails) != len(ids):
            raise ValueError("%d tails for %d sessions" % (len(tails), len(ids)))
        rs = []
        pend = self._pend[ids]
        for i, t in enumerate(tails):
            if t is None:
                rs.append(int(pend[i]))                          # a fed session: its tail is what waits in the FIFO
                continue
            if pend[i]:
                raise ValueError("tail %d: session %d has %d pending samples from feed(), they are its tail"
                                 % (i, ids[i], pend[i]))
            if not torch.is_tensor(t) or t.dim() != 1:
                raise ValueError("tail %d: expected a 1-D tensor or None" % i)
            if t.shape[0] >= HOP:
                raise ValueError("tail %d has %d samples: whole hops go through step(), a tail holds at most %d"
                                 % (i, t.shape[0], HOP - 1))
            if t.shape[0] and (not t.is_cuda or t.device != self.dev):
                raise L.TrunetHipError("tinyrecurrentunet_amd runs on MI355X only: the pool sits on %s, tail %d is a %s tensor"
                                       % (self.dev, i, t.device))
            rs.append(int(t.shape[0]))
        plan = plan_close(self._hops[ids], rs, ids)
        if not len(ids):
            return []
        n = len(ids)
        tl, n_tl = None, 0
        if pend.any():                                          # rows of the FIFO; what lies past a row's r samples is not read
            tl, n_tl = self.fifo.index_select(0, torch.from_numpy(ids).to(self.dev)), n
        elif any(rs):
            tl, n_tl = torch.zeros((n, HOP), device=self.dev, dtype=torch.float32), n
        given = [i for i, (t, r) in enumerate(zip(tails, rs)) if t is not None and r]
        if given:
            where = np.concatenate([HOP * i + np.arange(rs[i]) for i in given])
            tl.view(-1).index_copy_(0, torch.from_numpy(where).to(self.dev), torch.cat([tails[i].float() for i in given]))
        out = torch.zeros((n, CLOSE_OUT_ROWS * HOP), device=self.dev, dtype=torch.float32)
        self._run_passes(plan, tl, n_tl, out, n * CLOSE_OUT_ROWS, self._att_close(ids, plan, tails, rs))
        self._alloc.release(ids)
        return [out[i, :m] for i, m in enumerate(plan.lengths)]
