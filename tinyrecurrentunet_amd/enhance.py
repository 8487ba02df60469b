"""Offline enhancement of many recordings of any lengths: the role of the reference's ``denoise.py:27-97`` (broken there,
SURVEY D12).

``enhance(net, xs)`` takes a list of 1-D fp32 cuda tensors (16 kHz, at least 257 samples each) or a padded ``(B, Lmax)``
tensor with ``lengths`` and returns the denoised audio with exactly each input's length.  Per utterance the result is the
offline path of ``util.loss_fn`` -- centred rect STFT with reflect padding and PCEN from the utterance's first frame
(``dataset.py:56-76,246-272``), the network in eval mode, phase-aware mask and ``torch.istft(..., length=L)``
(``phm.py:31-45``, ``dataset.py:293-296``) -- and does not depend on which other utterances share the call, their order,
or the chunking of the frames.  Audio at another rate (``fs=``, 8 to 96 kHz) is resampled to 16 kHz and back on the GPU
around the same call (resample.py); ``highband="keep"`` or ``"follow"`` carries the band above 8 kHz,
which the resampler's low-pass removes, around the network (highband.py).  A call is

    pack          the utterances back to back + their offset tables (one host -> device copy)
    features      trunet_stft_features_ragged (+ trunet_pcen_ragged for C_in = 4): one launch each for the whole batch
    network       eval mode, no autograd, in chunks of at most ``max_frames`` frames
    back end      trunet_mask_istft_ragged: one launch pair for the whole batch
    unpack

The network runs the folded single-launch artefact (``path="folded"``, BatchNorm folded, fp32 whatever the net's
precision) or the layer kernels (``path="layers"``: the net's own precision, eval schedule); the choice is made once per
call.  Without the time-recurrent block every frame is independent, so a chunk may split an utterance.  With it
(``use_tgru``) utterances are grouped by length, each group laid out as B_g blocks of T_max frames with zero features
after each utterance's end and run with ``frames_per_seq = T_max``: exact, since the block is unidirectional and every
other layer acts per frame with eval BatchNorm.

Command line (the ``denoise.py`` role)::

    python -m tinyrecurrentunet_amd.enhance --checkpoint CKPT --input-size {3,4} [--use-tgru] --in DIR --out DIR [--resample]
    ... --resample [--highband {drop,keep,follow}] [--highband-floor-db DB]
    ... --atten-lim-db L        suppress the noise by at most L dB (atten.py)
"""
import argparse
import math
import os

import numpy as np
import torch

from . import _lib as L
from ._lib import check, ptr

N_FFT, HOP, BINS = 512, 128, 257
MIN_SAMPLES = N_FFT // 2 + 1          # the reflect padding of the first frame needs x[1..256]
SAMPLE_RATE = 16000
PCEN = dict(eps=1e-6, s=0.025, alpha=0.98, delta=2.0, r=0.5)     # dataset.py:56 defaults
# frames per network launch: 8192 = TRUNet.fold_max_frames.  The folded kernel is persistent (one frame per workgroup
# iteration), so beyond a few thousand frames its rate no longer moves with the chunk size; the layer kernels' activations
# grow with it (DESIGN section 3d has the measured rates)
MAX_FRAMES = 8192
# TGRU groups: an utterance joins the group of the longest one while it has at least this share of its frames
TGRU_MIN_FILL = 0.75
PATHS = ("auto", "folded", "layers", "int8")


def n_frames(length):
    return 1 + int(length) // HOP


def tgru_groups(frames, max_frames=MAX_FRAMES, min_fill=TGRU_MIN_FILL):
    """Group utterances (frame counts ``frames``) for the time-recurrent block: longest first, a group of B_g utterances
    padded to its longest T_max holds at most max(max_frames, T_max) frames, and every member has at least
    ``min_fill * T_max`` frames.  Returns (groups as lists of indices, padding fraction = padded / computed frames)."""
    order = sorted(range(len(frames)), key=lambda i: (-frames[i], i))
    groups, cur, tmax = [], [], 0
    for i in order:
        t = frames[i]
        if cur and ((len(cur) + 1) * tmax > max_frames or t < min_fill * tmax):
            groups.append(cur)
            cur = []
        if not cur:
            tmax = t
        cur.append(i)
    if cur:
        groups.append(cur)
    computed = sum(len(g) * frames[g[0]] for g in groups)
    return groups, (1.0 - sum(frames) / computed) if computed else 0.0


def _inputs(x, lengths):
    """-> (list of 1-D tensors, padded width or None).  Raises before anything reaches the device."""
    if isinstance(x, (list, tuple)):
        if lengths is not None:
            raise ValueError("lengths goes with a padded (B, Lmax) tensor, not with a list")
        xs = list(x)
        for b, t in enumerate(xs):
            if not torch.is_tensor(t) or t.dim() != 1:
                raise ValueError("utterance %d: expected a 1-D tensor, got %s" % (
                    b, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
        return xs, None
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError("expected a list of 1-D tensors or a (B, Lmax) tensor with lengths")
    B, width = x.shape
    if lengths is None:
        lens = [width] * B
    else:
        lens = [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        if len(lens) != B:
            raise ValueError("%d lengths for %d rows" % (len(lens), B))
        for b, n in enumerate(lens):
            if n > width or n < 0:
                raise ValueError("lengths[%d] = %d does not fit a row of %d samples" % (b, n, width))
    return [x[b, :n] for b, n in enumerate(lens)], width


@torch.no_grad()
def enhance(net, x, lengths=None, beta=0.5, max_frames=None, path="auto", fs=SAMPLE_RATE, highband="drop",
            highband_floor_db=-30.0, atten_lim_db=None):
    """Denoise recordings of any lengths with ``net`` (a ``network.TRUNet`` in eval mode, on the GPU).

    x: a list of 1-D fp32 cuda tensors -> list of 1-D tensors of the same lengths; or a (B, Lmax) tensor with ``lengths``
    (default: all Lmax) -> (B, Lmax), zeros past each length.  Every utterance needs at least 257 samples.
    max_frames: frames per network launch (default 8192; with ``use_tgru`` the frames of one group of equal-ish lengths,
    a single longer utterance being a group of its own).  path: "folded" (the single-launch eval artefact, fp32), "layers"
    (the layer kernels in the net's precision) or "auto" (folded unless ``net.fold_eval`` is off; a ``use_tgru`` net
    always runs the layer kernels, the only ones that carry the block over whole sequences); "int8" quantizes the net's
    current weights once per call (quantize.QuantizedTRUNet, stateless nets only).
    fs: the sample rate of ``x``.  At another rate than 16 kHz the audio is resampled to 16 kHz on the GPU
    (resample.resample), enhanced, resampled back and cut to exactly each input's length.  Every utterance then needs at
    least 257 samples at 16 kHz.
    highband: what becomes of the band above 8 kHz when ``fs`` is above 16 kHz.  "drop" (default): the band above 8 kHz is
    not restored.  "keep": the input's band is added back as it was.  "follow": it is added back attenuated, frame by
    frame, by the suppression the network applied between 4 and 8 kHz, never below ``highband_floor_db`` (at most 0 dB)
    and never amplified (highband.rejoin).  At ``fs`` <= 16 kHz there is no such band: the result is
    that of "drop".
    atten_lim_db: the most the noise is suppressed, in dB: a number >= 0 or inf, or one per utterance (a sequence or a 1-D
    tensor).  None (default): no limit, and nothing is added to the call.  With L dB every 16 kHz sample becomes
    y + g (x - y), g = 10^(-L / 20), y the enhanced and x the input sample (atten.py): one more launch,
    trunet_atten_blend_ragged, in place on the iSTFT output.  At another ``fs`` the blend acts at 16 kHz, so resampling and
    ``highband`` read the blended signal, and "follow" holds the band above 8 kHz by the same limit."""
    if path not in PATHS:
        raise ValueError("path must be one of %s, got %r" % (PATHS, path))
    from .highband import check_args
    highband, highband_floor_db = check_args(highband, highband_floor_db)
    if max_frames is None:
        max_frames = MAX_FRAMES
    if int(max_frames) != max_frames or max_frames < 1:
        raise ValueError("max_frames must be a positive integer, got %r" % (max_frames,))
    max_frames = int(max_frames)
    if net.training:
        raise L.TrunetHipError("enhance is an inference path: call net.eval() first")
    if net.use_tgru and path in ("folded", "int8"):
        raise ValueError("use_tgru runs the layer kernels (frames_per_seq): path=%r carries no sequence" % path)
    if fs != SAMPLE_RATE:
        return _enhance_at(net, x, lengths, beta, max_frames, path, fs, highband, highband_floor_db, atten_lim_db)
    xs, width = _inputs(x, lengths)
    g = None
    if atten_lim_db is not None:
        from .atten import gains
        g = gains(atten_lim_db, len(xs))
    for b, t in enumerate(xs):
        if t.shape[0] < MIN_SAMPLES:
            raise ValueError("utterance %d has %d samples; at least %d are needed (reflect padding of the first frame)"
                             % (b, t.shape[0], MIN_SAMPLES))
    if not xs:
        return [] if width is None else x.new_zeros((0, width))
    for b, t in enumerate(xs):
        if not t.is_cuda:
            raise L.TrunetHipError("tinyrecurrentunet_amd runs on MI355X only: utterance %d is a %s tensor" % (b, t.device))
    dev = next(net.parameters()).device
    if dev.type != "cuda":
        raise L.TrunetHipError("tinyrecurrentunet_amd runs on MI355X only: the network sits on %s" % dev)
    C = net.encoder[0].StandardConv1d[0].in_channels
    if C not in (3, 4):
        raise L.TrunetHipError("features have 3 or 4 channels (R2), the network expects %d" % C)
    if path == "auto":
        path = "layers" if (net.use_tgru or not net.fold_eval) else "folded"

    # 1. pack
    pk = Packed(xs, dev)
    if g is not None:                             # the gains go up with the offset tables, before the first launch
        g = torch.from_numpy(g).pin_memory().to(dev, non_blocking=True)
    # 2. features (+ PCEN)
    feat = features(pk, C)
    # 3. network
    if net.use_tgru:
        out = _tgru_forward(net, feat, pk.frames, pk.offs[1], max_frames)
    else:
        if path == "folded":
            run = net.folded()                    # ONE weight check per call (fold_verify), not one per chunk
        elif path == "int8":
            from .quantize import QuantizedTRUNet
            run = QuantizedTRUNet.from_module(net)
        else:
            if net._engine is None:
                object.__setattr__(net, "_engine", net._make_engine())
            eng = net._engine
            run = lambda v: eng.forward(v, False)[0]
        if pk.nT <= max_frames:
            out = run(feat)
        else:
            out = torch.cat([run(feat[i:i + max_frames]) for i in range(0, pk.nT, max_frames)])
    del feat
    # 4. mask + iSTFT
    den = mask_istft(pk, out, beta)
    if g is not None:
        atten_blend(pk, den, g)
    # 5. unpack
    if width is None:
        return list(torch.split(den, pk.lens))
    Y = torch.zeros((pk.B, width), device=dev, dtype=torch.float32)
    for b, (s0, n) in enumerate(zip(pk.offs[0, :-1].tolist(), pk.lens)):
        Y[b, :n] = den[s0:s0 + n]
    return Y


def _enhance_at(net, x, lengths, beta, max_frames, path, fs, highband="drop", floor_db=-30.0, atten_lim_db=None):
    """enhance() for audio at ``fs``: resample -> enhance at 16 kHz -> resample back -> cut to the input lengths.
    ceil(ceil(L p / q) q / p) >= L, so there is always enough to cut.  With ``highband`` "keep" or "follow" and ``fs``
    above 16 kHz the way back is highband.rejoin, which adds the input's band above 8 kHz to the resampled result.  An
    attenuation limit goes to the 16 kHz call."""
    from . import resample as R
    p, q = R.ratio(fs, SAMPLE_RATE)
    xs, width = _inputs(x, lengths)
    if atten_lim_db is not None:
        from .atten import gains
        gains(atten_lim_db, len(xs))                      # refuse before anything reaches the device
    for b, t in enumerate(xs):
        if R.out_length(t.shape[0], p, q) < MIN_SAMPLES:
            raise ValueError("utterance %d has %d samples at %d Hz, %d at %d Hz; at least %d are needed there (reflect "
                             "padding of the first frame)" % (b, t.shape[0], fs, R.out_length(t.shape[0], p, q),
                                                              SAMPLE_RATE, MIN_SAMPLES))
    lens = [int(t.shape[0]) for t in xs]
    down = R.resample(xs, fs, SAMPLE_RATE)
    if atten_lim_db is None:
        den = enhance(net, down, beta=beta, max_frames=max_frames, path=path)
    else:
        den = enhance(net, down, beta=beta, max_frames=max_frames, path=path, atten_lim_db=atten_lim_db)
    if highband != "drop" and p < q and xs:
        from .highband import rejoin
        up = rejoin(xs, down, den, fs, highband, floor_db)
    else:
        up = R.resample(den, SAMPLE_RATE, fs)
    if width is None:
        return [y[:n] for y, n in zip(up, lens)]
    Y = torch.zeros((len(xs), width), device=up[0].device if up else x.device, dtype=torch.float32)
    for b, (y, n) in enumerate(zip(up, lens)):
        Y[b, :n] = y[:n]
    return Y


class Packed:
    """B utterances back to back on ``dev`` (``audio``, sum L_b samples) and their int64 offset tables: rows of ``offs``
    (host) / ``offs_d`` (device, one copy) = prefix sums of L_b, of T_b = 1 + L_b // 128 and of ceil(T_b / 2)."""

    def __init__(self, xs, dev):
        self.lens = [int(t.shape[0]) for t in xs]
        self.frames = [n_frames(n) for n in self.lens]
        self.B = len(xs)
        offs = np.zeros((3, self.B + 1), dtype=np.int64)
        offs[0, 1:] = np.cumsum(self.lens)
        offs[1, 1:] = np.cumsum(self.frames)
        offs[2, 1:] = np.cumsum([(t + 1) // 2 for t in self.frames])
        self.offs = offs
        self.nS, self.nT, self.nP = (int(v) for v in offs[:, -1])
        self.offs_d = torch.from_numpy(offs).to(dev)
        self.audio = torch.cat([t.to(device=dev, dtype=torch.float32) for t in xs]).contiguous()
        self.dev = dev

    def ptrs(self):
        return tuple(self.offs_d[i].data_ptr() for i in range(3))


def features(pk, C):
    """trunet_stft_features_ragged (+ trunet_pcen_ragged, C = 4): features (sum T_b, C, 257) of every utterance"""
    lib, st = L.lib(), L.stream()
    so, fo, po = pk.ptrs()
    feat = torch.empty((pk.nT, C, BINS), device=pk.dev, dtype=torch.float32)
    mag = torch.empty((pk.nT, BINS), device=pk.dev, dtype=torch.float32) if C == 4 else None
    check(lib.trunet_stft_features_ragged(ptr(pk.audio), so, fo, po, ptr(feat), ptr(mag), ptr(L.twiddles(N_FFT, pk.dev)),
                                          pk.B, pk.nS, pk.nT, pk.nP, C, st), "stft_features_ragged")
    if C == 4:
        p = PCEN
        check(lib.trunet_pcen_ragged(ptr(mag), feat.view(-1)[BINS:].data_ptr(), fo, pk.B, pk.nT, C * BINS, p["eps"],
                                     p["s"], p["alpha"], p["delta"], p["r"], st), "pcen_ragged")
    return feat


def mask_istft(pk, out, beta=0.5):
    """trunet_mask_istft_ragged: net output (sum T_b, 8, 257) -> packed denoised audio (sum L_b)"""
    out = out.contiguous().float()
    if tuple(out.shape) != (pk.nT, 8, BINS):
        raise ValueError("expected (%d, 8, %d) net output, got %s" % (pk.nT, BINS, tuple(out.shape)))
    so, fo, po = pk.ptrs()
    fr = torch.empty((pk.nT, N_FFT), device=pk.dev, dtype=torch.float32)
    den = torch.empty(pk.nS, device=pk.dev, dtype=torch.float32)
    check(L.lib().trunet_mask_istft_ragged(ptr(out), ptr(fr), ptr(den), so, fo, po, ptr(L.twiddles(N_FFT, pk.dev)), pk.B,
                                           pk.nS, pk.nT, pk.nP, float(beta), L.stream()), "mask_istft_ragged")
    return den


def atten_blend(pk, den, g):
    """trunet_atten_blend_ragged: den[n] <- den[n] + g_b (x[n] - den[n]) in place, x the packed input ``pk.audio`` and g
    the (B,) fp32 gains on the device, one per utterance (atten.gains)"""
    if tuple(g.shape) != (pk.B,):
        raise ValueError("expected %d gains, got %s" % (pk.B, tuple(g.shape)))
    check(L.lib().trunet_atten_blend_ragged(ptr(den), ptr(pk.audio), ptr(g), pk.ptrs()[0], pk.B, pk.nS, L.stream()),
          "atten_blend_ragged")
    return den


def _tgru_forward(net, feat, frames, frame_off, max_frames):
    """use_tgru: per group of similar lengths, B_g blocks of T_max frames (zero features after each utterance's end) through
    net(..., frames_per_seq=T_max); the padding frames are dropped."""
    nT, C = feat.shape[0], feat.shape[1]
    out = torch.empty((nT, 8, BINS), device=feat.device, dtype=torch.float32)
    groups, _ = tgru_groups(frames, max_frames)
    for g in groups:
        tmax = frames[g[0]]
        xg = torch.zeros((len(g), tmax, C, BINS), device=feat.device, dtype=torch.float32)
        for k, b in enumerate(g):
            f0 = int(frame_off[b])
            xg[k, :frames[b]] = feat[f0:f0 + frames[b]]
        yg = net(xg.view(-1, C, BINS), frames_per_seq=tmax).view(len(g), tmax, 8, BINS)
        for k, b in enumerate(g):
            f0 = int(frame_off[b])
            out[f0:f0 + frames[b]] = yg[k, :frames[b]]
    return out


# ---------------------------------------------------------------- command line
def load_net(checkpoint, input_size, use_tgru=False, device="cuda"):
    """train.py's {"model_state_dict": ...} pickle or a bare state_dict -> TRUNet in eval mode on ``device``."""
    from .network import TRUNet
    ck = torch.load(checkpoint, map_location="cpu", weights_only=True)
    sd = ck["model_state_dict"] if isinstance(ck, dict) and "model_state_dict" in ck else ck
    net = TRUNet(input_size=input_size, use_tgru=use_tgru)
    net.load_state_dict(sd)
    return net.to(device).eval()


def _batches(lens, max_samples):
    """consecutive files up to max_samples samples per call (a longer file is a call of its own)"""
    cur, tot = [], 0
    for i, n in enumerate(lens):
        if cur and tot + n > max_samples:
            yield cur
            cur, tot = [], 0
        cur.append(i)
        tot += n
    if cur:
        yield cur


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m tinyrecurrentunet_amd.enhance",
                                 description="Denoise every 16 kHz *.wav of a folder with a trained TRU-Net (HIP, MI355X).  "
                                             "With --resample, files at other rates are resampled to 16 kHz on the GPU, "
                                             "denoised and written back at their own rate; the band above 8 kHz is not "
                                             "restored unless --highband says so.")
    ap.add_argument("--checkpoint", required=True, help="train.py checkpoint ({'model_state_dict': ...}) or a state_dict")
    ap.add_argument("--input-size", type=int, choices=(3, 4), required=True, help="feature channels the net was trained on")
    ap.add_argument("--use-tgru", action="store_true", help="the net was trained with the time-recurrent block")
    ap.add_argument("--in", dest="indir", required=True, help="folder of noisy *.wav (mono, 16 kHz)")
    ap.add_argument("--out", dest="outdir", required=True, help="folder for the denoised int16 *.wav (same names)")
    ap.add_argument("--max-seconds", type=float, default=600.0, help="audio per enhance() call (default 600 s)")
    ap.add_argument("--path", choices=PATHS, default="auto", help="network path (default auto)")
    ap.add_argument("--resample", action="store_true",
                    help="accept files at other rates than 16 kHz (8 to 96 kHz): resample to 16 kHz, denoise, resample "
                         "back; every file keeps its rate and sample count")
    ap.add_argument("--highband", choices=("drop", "keep", "follow"), default="drop",
                    help="with --resample, for files above 16 kHz: drop (default): the band above 8 kHz is not restored; "
                         "keep: the input's band is added back as it was; follow: added back with the suppression the "
                         "network applied between 4 and 8 kHz.  Files at 16 kHz and below are unaffected")
    ap.add_argument("--highband-floor-db", type=float, default=-30.0,
                    help="--highband follow: the most the band above 8 kHz is attenuated, in dB (default -30)")
    ap.add_argument("--atten-lim-db", type=float, default=None,
                    help="suppress the noise by at most this many dB (>= 0; default: no limit): every sample becomes "
                         "y + 10^(-L/20) (x - y), y the enhanced and x the input sample at 16 kHz")
    args = ap.parse_args(argv)
    if args.atten_lim_db is not None:
        from .atten import gain
        try:
            gain(args.atten_lim_db)
        except ValueError as e:
            ap.error(str(e))
    if not args.resample and (args.highband != "drop" or args.highband_floor_db != -30.0):
        ap.error("--highband and --highband-floor-db go with --resample")
    from .highband import check_args
    try:
        check_args(args.highband, args.highband_floor_db)
    except ValueError as e:
        ap.error(str(e))

    from scipy.io.wavfile import write as wavwrite
    from .dataset import _read_wav
    names = sorted(f for f in os.listdir(args.indir) if f.lower().endswith(".wav"))
    xs, rates = [], []
    for nm in names:
        x, sr = _read_wav(os.path.join(args.indir, nm))
        if sr != SAMPLE_RATE:
            if not args.resample:
                raise SystemExit("%s: %d Hz; the network runs at %d Hz (no resampling)" % (nm, sr, SAMPLE_RATE))
            from .resample import ratio, out_length
            try:
                p, q = ratio(sr, SAMPLE_RATE)
            except ValueError as e:
                raise SystemExit("%s: %s" % (nm, e))
            if out_length(x.shape[0], p, q) < MIN_SAMPLES:
                raise SystemExit("%s: %d samples at %d Hz, at least %d are needed at %d Hz"
                                 % (nm, x.shape[0], sr, MIN_SAMPLES, SAMPLE_RATE))
        elif x.shape[0] < MIN_SAMPLES:
            raise SystemExit("%s: %d samples, at least %d are needed" % (nm, x.shape[0], MIN_SAMPLES))
        xs.append(x)
        rates.append(sr)
    net = load_net(args.checkpoint, args.input_size, args.use_tgru)
    os.makedirs(args.outdir, exist_ok=True)
    for rate in sorted(set(rates)):                       # --max-seconds counts seconds: samples at each group's rate
        group = [i for i, r in enumerate(rates) if r == rate]
        max_samples = max(1, int(math.floor(args.max_seconds * rate)))
        for chunk in _batches([xs[i].shape[0] for i in group], max_samples):
            idx = [group[k] for k in chunk]
            ys = enhance(net, [xs[i].cuda() for i in idx], path=args.path, fs=rate, highband=args.highband,
                         highband_floor_db=args.highband_floor_db, atten_lim_db=args.atten_lim_db)
            for i, y in zip(idx, ys):
                q16 = torch.clamp(torch.round(y * 32768.0), -32768, 32767).to(torch.int16).cpu().numpy()
                wavwrite(os.path.join(args.outdir, names[i]), rate, q16)
    print("%d files -> %s" % (len(names), args.outdir))


if __name__ == "__main__":
    main()
