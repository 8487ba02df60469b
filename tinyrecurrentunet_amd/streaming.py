"""Causal audio-in -> audio-out streaming on the HIP path (SURVEY.md 8f ranks 1-2 widened; the protocol the reference
sketches in ``/root/reference/stream.py:83-109``: per audio chunk ``ProcessAudio`` features -> model -> back to audio).

``AudioStream(net, streams)`` carries, per stream, the last 512 input samples, the PCEN smoother ``M`` of
``dataset.py:56-76``, the overlap-add tail of the inverse STFT (``dataset.py:293-296``) and -- with the time-recurrent
block -- the TGRU hidden state.  One hop of 128 new samples per stream costs THREE launches on the current stream:

    trunet_stream_features   ring shift + rect-window rFFT-512 + (norm-dB-mag, [PCEN with carried M], sin, cos)
    trunet_stream_fwd        the whole network in one launch (export.FoldedTRUNet; BatchNorm folded, eval semantics)
    trunet_stream_mask_istft phase-aware mask + irFFT-512 + overlap-add tail -> the 128 samples that are final now

All state tensors keep their addresses, so a captured hipGraph of one steady-state step replays hop after hop.

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
PCEN = dict(eps=1e-6, s=0.025, alpha=0.98, delta=2.0, r=0.5)     # dataset.py:56 defaults


class AudioStream:
    def __init__(self, net, streams, tgru=False, beta=0.5, device=None, int8=False):
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
        return out if t >= 2 else None

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
            outs.append(self.ola[:, :HOP] / 3.0)
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

        pool = StreamPool(net, slots, tgru=None, beta=0.5, int8=False)     # net in eval mode on the GPU; tgru None: net.use_tgru
        ids = pool.open(n)                      # n free slot ids
        out, valid = pool.step(chunks, ids)     # chunks (n, 128) fp32 cuda; ids: n distinct open slots
        rest = pool.close(ids, tails)           # list of 1-D tensors; tails[i]: the 0..127 last samples of session i, or None
        pool.abort(ids)                         # drop sessions without output
        pool.free, pool.capacity, pool.hops(id)

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
    The weights are those of the folded (or int8) artefact taken at construction."""

    def __init__(self, net, slots, tgru=None, beta=0.5, int8=False):
        if net.training:
            raise L.TrunetHipError("StreamPool is an inference path: call net.eval() first")
        dev = next(net.parameters()).device
        if dev.type != "cuda":
            raise L.TrunetHipError("tinyrecurrentunet_amd runs on MI355X only: the network sits on %s" % dev)
        self._alloc = SlotAllocator(slots)
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
        self.tw = L.twiddles(N_FFT, dev)
        self._hops = np.zeros(S, dtype=np.int64)

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

    def open(self, n=1):
        """n new sessions -> their slot ids; raises when fewer than n slots are free.  Host work only: the first frame of a
        session overwrites the slot's state."""
        ids = self._alloc.open(n)
        for i in ids:
            self._hops[i] = 0
        return ids

    def abort(self, ids):
        """Drop sessions without output; the slots are free again."""
        self._alloc.release(self._ids(ids))

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

    def _run_passes(self, plan, chunks, n_chunks, out, n_out):
        dev_tab = torch.from_numpy(np.concatenate(plan.tables)).to(self.dev)     # the row tables of every pass: ONE copy
        r0 = 0
        for table, nf in zip(plan.tables, plan.frames):
            self._pass(dev_tab[r0:r0 + len(table)], table, nf, chunks, n_chunks, out, n_out)
            r0 += len(table)

    @torch.no_grad()
    def step(self, chunks, ids):
        """One hop of 128 new samples for each listed session: chunks (n, 128) fp32 on the pool's device, ids n distinct open
        slots.  Returns (out (n, 128), valid (n,) CPU bool): row i is session ids[i]'s next 128 denoised samples where
        valid[i], zeros otherwise (its first three hops).  Never synchronises with the device."""
        ids = self._ids(ids)
        if not torch.is_tensor(chunks):
            raise ValueError("chunks: a (%d, %d) tensor, got %s" % (len(ids), HOP, type(chunks).__name__))
        if not chunks.is_cuda or chunks.device != self.dev:
            raise L.TrunetHipError("tinyrecurrentunet_amd runs on MI355X only: the pool sits on %s, got a %s tensor"
                                   % (self.dev, chunks.device))
        if tuple(chunks.shape) != (len(ids), HOP):
            raise ValueError("expected (%d, %d) samples, got %s" % (len(ids), HOP, tuple(chunks.shape)))
        out = torch.zeros((len(ids), HOP), device=self.dev, dtype=torch.float32)
        if not len(ids):
            return out, torch.zeros(0, dtype=torch.bool)
        chunks = chunks.contiguous().float()
        plan = plan_step(self._hops, ids)
        self._run_passes(plan, chunks, len(ids), out, len(ids))
        self._hops[ids] = plan.hops
        return out, torch.from_numpy(plan.valid)

    @torch.no_grad()
    def close(self, ids, tails=None):
        """End sessions: tails[i] (None, or a 1-D fp32 tensor of 0..127 samples on the pool's device) are the samples after
        session i's last whole hop.  Returns, per session, the L - 128 max(a - 3, 0) samples not yet delivered, and frees the
        slots.  ValueError for a session of fewer than 257 samples; it stays open, like every other session of the call."""
        ids = self._ids(ids)
        tails = [None] * len(ids) if tails is None else list(tails)
        if len(tails) != len(ids):
            raise ValueError("%d tails for %d sessions" % (len(tails), len(ids)))
        rs = []
        for i, t in enumerate(tails):
            if t is None:
                rs.append(0)
                continue
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
        if any(rs):
            tl, n_tl = torch.zeros((n, HOP), device=self.dev, dtype=torch.float32), n
            where = np.concatenate([HOP * i + np.arange(r) for i, r in enumerate(rs) if r])
            tl.view(-1).index_copy_(0, torch.from_numpy(where).to(self.dev),
                                    torch.cat([t.float() for t, r in zip(tails, rs) if r]))
        out = torch.zeros((n, CLOSE_OUT_ROWS * HOP), device=self.dev, dtype=torch.float32)
        self._run_passes(plan, tl, n_tl, out, n * CLOSE_OUT_ROWS)
        self._alloc.release(ids)
        return [out[i, :m] for i, m in enumerate(plan.lengths)]
