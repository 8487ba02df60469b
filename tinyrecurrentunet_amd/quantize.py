"""The int8 inference artefact (the quantized model of the reference's README) and its runner, ``trunet_stream_fwd_i8``
(csrc/stream_fwd_i8.hip): the stateless eval forward (N, C_in, 257) -> (N, 8, 257) of
``export.FoldedTRUNet`` with every matrix layer on the int8 MFMA.

Numerics (the tests restate them in float64, tests/quant_ref.py):

* Starting point: the BatchNorm-folded fp32 weights of ``export.fold()``.
* int8 layers: encoder pointwise convs, the FGRU input projection (both directions, 384 rows), FGRU.conv, every decoder
  pointwise conv and the transposed convs (as ``fold()``'s per-tap GEMMs, tap-major K).  Weights are symmetric with one
  scale per output row, ``s_w = fp32(max_k |W| / 127)``, ``q = clamp(rint(W / s_w), -127, 127)`` in float64 (an all-zero
  row has s_w = 0 and q = 0); biases stay fp32.
* Activations are quantized by the kernel, per frame and per layer, with one scale for the layer's whole operand:
  ``amax = max |x|``, ``inv = 127 / amax`` (fp32), ``q = clamp(rne(x inv), -127, 127)``; int32 accumulation;
  ``z = float(acc) (s_w s_x) + b`` with ``s_x = amax / 127``.  Every frame stays independent of its batch-mates.
* W_hh of the FGRU recurrence: int8 with per-row scales, dequantized once in the kernel; the recurrence is fp32.
* The first conv, the depthwise convs and the last 8 -> 8 transposed conv are ``fold()``'s fp32 values bit for bit.

The image is one byte blob (a multiple of 4 bytes) + 26 section offsets in 32-bit words, in ``fold()``'s section order.
``python -m tinyrecurrentunet_amd.quantize --checkpoint CKPT --input-size {3,4} --out PATH`` writes it."""
import argparse
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import export as E
from ._lib import check, ptr

FORMAT = "trunet-int8-v1"
N_SECTIONS = 26
PAD_WORDS = 512                # behind the last section: the kernel requests the 3-tap ConvT tiles as 5 quads
PAPER_BYTES = 362_000          # the quantized model size the reference's README quotes
SECTION_NAMES = (["first"] + ["pw%d" % i for i in range(5)] + ["dw%d" % i for i in range(5)] + ["gi", "whh", "fg"]
                 + ["dpw%d" % i for i in range(6)] + ["ct%d" % i for i in range(5)] + ["last"])
# matrix sections: index -> (rows, K, row tiles of 32 in fold()'s image (else 16))
_MATS = {i: (M, K, tile == 32) for i, (M, K, tile, _) in E._X3_SECTIONS.items() if i < N_SECTIONS}
_FP32 = (0, 6, 7, 8, 9, 10, 25)


def _fp32_size(i, cin):
    return 64 * cin * 5 + 64 if i == 0 else (8 * 8 * 5 + 8 if i == 25 else 128 * (5 if (i - 6) & 1 else 3) + 128)


def quantize_rows(W):
    """W (M, K) -> (q int8 (M, K), s_w float32 (M,)): symmetric per-row codes, q = clamp(rint(W / s_w), -127, 127) in
    float64 with the stored fp32 scale s_w = fp32(max_k |W| / 127); an all-zero row has s_w = 0 and q = 0."""
    W = np.asarray(W, dtype=np.float64)
    s = (np.abs(W).max(1) / 127.0).astype(np.float32)
    sd = s.astype(np.float64)[:, None]
    q = np.where(sd > 0, np.rint(W / np.where(sd > 0, sd, 1.0)), 0.0)
    return np.clip(q, -127, 127).astype(np.int8), s


def _tiles_i8(q, s, b):
    """q (M, K) int8, K a multiple of 64; s, b (M,) -> uint32 words: per 16-row tile [K/64 quads][16 scales][16 biases], quad
    = [64 lanes][16 bytes], lane l holding q[row l & 15][k = 64 ks + 16 (l >> 4) + 0..15] (v_mfma_i32_16x16x64_i8 A)."""
    M, K = q.shape
    assert K % 64 == 0, K
    nrt = (M + 15) // 16
    qp = np.zeros((nrt * 16, K), dtype=np.int8)
    qp[:M] = q
    sp = np.zeros(nrt * 16, dtype=np.float32)
    sp[:M] = s
    bp = np.zeros(nrt * 16, dtype=np.float32)
    bp[:M] = b
    lane = np.arange(64)
    out = []
    for rt in range(nrt):
        rows = rt * 16 + (lane & 15)
        for ks in range(K // 64):
            k0 = 64 * ks + 16 * (lane >> 4)
            out.append(np.ascontiguousarray(qp[rows[:, None], k0[:, None] + np.arange(16)[None, :]]).view(np.uint32).reshape(-1))
        out.append(sp[rt * 16:rt * 16 + 16].view(np.uint32))
        out.append(bp[rt * 16:rt * 16 + 16].view(np.uint32))
    return np.concatenate(out)


def _untiles_i8(words, M, K):
    """Inverse of _tiles_i8 -> (q (M, K) int8, s (M,) float32, b (M,) float32)."""
    nrt, KS = (M + 15) // 16, K // 64
    per = 256 * KS + 32
    w = np.asarray(words, dtype=np.uint32)[:nrt * per].reshape(nrt, per)
    q = np.zeros((nrt * 16, K), dtype=np.int8)
    s = np.zeros(nrt * 16, dtype=np.float32)
    b = np.zeros(nrt * 16, dtype=np.float32)
    lane = np.arange(64)
    for rt in range(nrt):
        rows = rt * 16 + (lane & 15)
        for ks in range(KS):
            blk = np.ascontiguousarray(w[rt, 256 * ks:256 * ks + 256]).view(np.int8).reshape(64, 16)
            q[rows[:, None], 64 * ks + 16 * (lane >> 4)[:, None] + np.arange(16)[None, :]] = blk
        s[rt * 16:rt * 16 + 16] = w[rt, 256 * KS:256 * KS + 16].view(np.float32)
        b[rt * 16:rt * 16 + 16] = w[rt, 256 * KS + 16:256 * KS + 32].view(np.float32)
    return q[:M], s[:M], b[:M]


def _whh_of_folded(sec):
    """fold()'s W_hh section -> ([W_hh (192, 64) per direction] float32, b_hh (384,) float32)."""
    blk = np.asarray(sec[:2 * 24 * 128 * 4], dtype=np.float32).reshape(2, 24, 128, 4)
    Ws = []
    for d in range(2):
        W = np.zeros((192, 64), dtype=np.float32)
        for g in range(3):
            for i in range(8):
                # quad 8 g + i, thread 2 j + kh: W[64 g + j][32 kh + 4 i + e]
                v = blk[d, 8 * g + i].reshape(64, 2, 4)                   # (j, kh, e)
                for kh in range(2):
                    W[64 * g:64 * g + 64, 32 * kh + 4 * i:32 * kh + 4 * i + 4] = v[:, kh, :]
        Ws.append(W)
    return Ws, np.asarray(sec[2 * 24 * 128 * 4:2 * 24 * 128 * 4 + 384], dtype=np.float32)


def _whh_words(qs, ss, bhh):
    """[q (192, 64) int8] and [s (192,)] per direction, b_hh (384,) -> words: [direction][6 quads: gate g, half h][128 threads
    t = 2 j + kh][16 bytes q[64 g + j][32 kh + 16 h + 0..15]], then scales [2][192], then b_hh [2][192]."""
    out = []
    for q in qs:
        blk = np.zeros((6, 128, 16), dtype=np.int8)
        for g in range(3):
            for h in range(2):
                for t in range(128):
                    j, kh = t >> 1, t & 1
                    blk[2 * g + h, t] = q[64 * g + j, 32 * kh + 16 * h:32 * kh + 16 * h + 16]
        out.append(blk.reshape(-1).view(np.uint32))
    out.append(np.concatenate(ss).astype(np.float32).view(np.uint32))
    out.append(np.asarray(bhh, dtype=np.float32).view(np.uint32))
    return np.concatenate(out)


def _folded_sections(blob, offsets):
    blob = np.ascontiguousarray(np.asarray(blob, dtype=np.float32))
    offsets = np.asarray(offsets, dtype=np.int64)
    starts = sorted(set(int(offsets[i]) for i in range(E.N_OFFSETS) if i < 26 or offsets[i] > 0))
    bounds = {a: b for a, b in zip(starts, starts[1:] + [len(blob)])}
    return [blob[int(offsets[i]):bounds[int(offsets[i])]] for i in range(N_SECTIONS)]


def quantize_folded(blob, offsets, cin):
    """fold()'s image (blob, offsets, cin) -> (int8 image: uint8 ndarray, a multiple of 4 bytes; offsets int32[26] in
    32-bit words; cin).  Refuses an image with the time-recurrent block (out of scope)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    if offsets.shape != (E.N_OFFSETS,) or int(cin) not in (3, 4):
        raise L.TrunetHipError("not a folded TRU-Net image: %s offsets, cin %r" % (offsets.shape, cin))
    if offsets[26] > 0:
        raise L.TrunetHipError("the int8 artefact covers the stateless forward only: the time-recurrent block is not "
                               "quantized (export without tgru)")
    secs = _folded_sections(blob, offsets)
    words, offs = [], []
    for i in range(N_SECTIONS):
        if i in _MATS:
            M, K, t32 = _MATS[i]
            W, b = (E._unfrag_tiles if t32 else E._unfrag_tiles16)(secs[i], M, K)
            q, s = quantize_rows(W)
            w = _tiles_i8(q, s, b)
        elif i == 12:
            Ws, bhh = _whh_of_folded(secs[i])
            qs = [quantize_rows(W) for W in Ws]
            w = _whh_words([a for a, _ in qs], [b for _, b in qs], bhh)
        else:
            n = _fp32_size(i, int(cin))
            w = np.ascontiguousarray(secs[i][:n + (-n) % 4]).view(np.uint32)
        offs.append(sum(len(x) for x in words))
        words.append(np.concatenate([w, np.zeros((-len(w)) % 4, dtype=np.uint32)]))
    words.append(np.zeros(PAD_WORDS, dtype=np.uint32))
    return np.concatenate(words).view(np.uint8), np.array(offs, dtype=np.int32), int(cin)


def quantize(net):
    """TRUNet -> (int8 image bytes as a uint8 ndarray, offsets int32[26], cin): fold() (BatchNorm folded), then quantized."""
    if getattr(net, "use_tgru", False):
        raise L.TrunetHipError("the int8 artefact covers the stateless forward only: this net runs the time-recurrent block")
    return quantize_folded(*E.fold(net))


class QuantizedTRUNet:
    """The int8 artefact and its runner (one kernel launch per forward)."""

    def __init__(self, blob, offsets, cin, device=None):
        blob = blob.detach().cpu().numpy() if torch.is_tensor(blob) else np.asarray(blob)
        blob = np.ascontiguousarray(blob).view(np.uint8) if blob.dtype != np.uint8 else np.ascontiguousarray(blob)
        offsets = np.ascontiguousarray(np.asarray(offsets, dtype=np.int32))
        if blob.ndim != 1 or len(blob) % 4 or offsets.shape != (N_SECTIONS,) or int(cin) not in (3, 4):
            raise L.TrunetHipError("not an int8 TRU-Net image: blob %s, %s offsets, cin %r" % (blob.shape, offsets.shape, cin))
        # host-side twin of the entry point's bounds check: a truncated or foreign artefact must not reach the kernel
        rc = L.lib().trunet_stream_fwd_i8_check(offsets.ctypes.data_as(C.POINTER(C.c_int32)), len(offsets), len(blob),
                                                int(cin))
        if rc != L.TRUNET_OK:
            raise L.TrunetHipError("int8 TRU-Net image fails the section bounds check (truncated or foreign artefact)")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.blob = torch.from_numpy(blob.copy()).to(dev)
        self.offsets = offsets
        self._offs = (C.c_int32 * N_SECTIONS)(*[int(v) for v in offsets])
        self.cin = int(cin)
        self._scratch = None

    @classmethod
    def from_module(cls, net, device=None, tgru=False):
        if tgru:
            raise L.TrunetHipError("the int8 artefact covers the stateless forward only (tgru=True)")
        dev = device if device is not None else next(net.parameters()).device
        return cls(*quantize(net), device=dev)

    @classmethod
    def from_folded(cls, folded, device=None):
        """An export.FoldedTRUNet -> its int8 artefact (the same folded weights, quantized)."""
        if folded.has_tgru:
            raise L.TrunetHipError("the int8 artefact covers the stateless forward only: the folded image has the "
                                   "time-recurrent block")
        dev = device if device is not None else folded.blob.device
        return cls(*quantize_folded(folded.blob.cpu().numpy(), folded.offsets, folded.cin), device=dev)

    @property
    def nbytes(self):
        """Size of the artefact: the image and its section table."""
        return int(self.blob.numel()) + 4 * N_SECTIONS

    def save(self, path):
        torch.save({"format": FORMAT, "blob": self.blob.cpu(), "offsets": torch.tensor(self.offsets), "cin": self.cin}, path)

    @classmethod
    def load(cls, path, device=None):
        d = torch.load(path, map_location="cpu", weights_only=True)
        fmt = d.get("format") if isinstance(d, dict) else None
        if fmt != FORMAT:
            raise L.TrunetHipError("%s is not an int8 TRU-Net artefact (format %r)" % (path, fmt))
        if not torch.is_tensor(d["blob"]) or d["blob"].dtype != torch.uint8:
            raise L.TrunetHipError("%s: the int8 image is a uint8 tensor" % path)
        return cls(d["blob"], d["offsets"].numpy(), int(d["cin"]), device)

    def dequantized_sections(self):
        """The image decoded on the host: name (SECTION_NAMES) -> for int8 layers (q int8 (M, K), s_w float32 (M,), bias
        float32 (M,)) in fold()'s matrix layout (ConvT: tap-major K); "whh" -> [(q (192, 64), s_w (192,))] per direction;
        "bhh" -> (384,); fp32 sections -> their float32 values: "first" (64 C_in 5 weights, 64 biases), "dw<i>" (128 k,
        128), "last" (320, 8)."""
        w = self.blob.cpu().numpy().view(np.uint32)
        o = [int(v) for v in self.offsets]
        out = {}
        for i, name in enumerate(SECTION_NAMES):
            if i in _MATS:
                M, K, _ = _MATS[i]
                out[name] = _untiles_i8(w[o[i]:], M, K)
            elif i == 12:
                blk = w[o[i]:o[i] + 2 * 6 * 128 * 4].view(np.int8).reshape(2, 6, 128, 16)
                sc = w[o[i] + 6144:o[i] + 6144 + 384].view(np.float32)
                out["bhh"] = w[o[i] + 6144 + 384:o[i] + 6144 + 768].view(np.float32).copy()
                out["whh"] = []
                for d in range(2):
                    q = np.zeros((192, 64), dtype=np.int8)
                    for g in range(3):
                        for h in range(2):
                            v = blk[d, 2 * g + h].reshape(64, 2, 16)      # (j, kh, 16)
                            for kh in range(2):
                                q[64 * g:64 * g + 64, 32 * kh + 16 * h:32 * kh + 16 * h + 16] = v[:, kh]
                    out["whh"].append((q, sc[192 * d:192 * d + 192].copy()))
            else:
                n = _fp32_size(i, self.cin)
                v = w[o[i]:o[i] + n].view(np.float32).copy()
                nb = 8 if i == 25 else (64 if i == 0 else 128)
                out[name] = (v[:n - nb], v[n - nb:])
        return out

    def forward(self, x):
        if not x.is_cuda or not self.blob.is_cuda:
            raise L.TrunetHipError("tinyrecurrentunet_amd runs on MI355X only: got a %s tensor and an artefact on %s"
                                   % (x.device, self.blob.device))
        x = x.contiguous().float()
        if x.dim() != 3 or x.shape[1] != self.cin or x.shape[2] != 257:
            raise ValueError("expected (N, %d, 257) features, got %s" % (self.cin, tuple(x.shape)))
        N = x.shape[0]
        lib = L.lib()
        need = lib.trunet_stream_fwd_scratch_floats(lib.trunet_stream_fwd_grid(N))
        if self._scratch is None or self._scratch.numel() < need or self._scratch.device != x.device:
            self._scratch = torch.empty(need, device=x.device, dtype=torch.float32)
        y = torch.empty((N, 8, 257), device=x.device, dtype=torch.float32)
        check(lib.trunet_stream_fwd_i8(ptr(x), ptr(y), self.blob.data_ptr(), self._offs, N_SECTIONS, self.blob.numel(),
                                       ptr(self._scratch), N, self.cin, L.stream()), "stream_fwd_i8")
        return y

    __call__ = forward


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m tinyrecurrentunet_amd.quantize",
                                 description="Write the int8 inference artefact of a trained TRU-Net (stateless forward).")
    ap.add_argument("--checkpoint", required=True, help="train.py checkpoint ({'model_state_dict': ...}) or a state_dict")
    ap.add_argument("--input-size", type=int, choices=(3, 4), required=True, help="feature channels the net was trained on")
    ap.add_argument("--out", required=True, help="artefact path (QuantizedTRUNet.load)")
    args = ap.parse_args(argv)
    from .enhance import load_net
    net = load_net(args.checkpoint, args.input_size, device="cpu")
    q = QuantizedTRUNet(*quantize(net), device="cpu")
    q.save(args.out)
    print("%s: %d bytes (the paper's quantized model: %d bytes)" % (args.out, q.nbytes, PAPER_BYTES))


if __name__ == "__main__":
    main()
