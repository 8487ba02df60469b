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
"""
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
