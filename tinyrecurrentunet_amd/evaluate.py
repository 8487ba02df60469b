"""Scoring of enhanced speech on the GPU: STOI, ESTOI and SI-SDR of many clean / estimate pairs of any lengths, the role of
the reference's ``eval.py`` (PESQ is not computed).

``evaluate(clean, estimate)`` takes the input forms of ``enhance.enhance`` (two lists of 1-D cuda tensors, or two padded
``(B, Lmax)`` tensors with ``lengths``) and returns ``(B,)`` float64 cuda tensors: ``stoi``, ``estoi``, ``si_sdr`` (those
asked for) and, with STOI or ESTOI, ``segments`` (int64, the 30-frame segments scored; 0 = too short, scores 1e-5).
Nothing is read back to the host.  The definition follows the ``pystoi`` 0.3 formulation as far as it
is pinned there; agreement with any ``pystoi`` release has not been checked, and ESTOI adds no random dither.

    pack       clean and estimate back to back + six int64 prefix tables (one host -> device copy)
    resample   trunet_resample_ragged: fs -> 10 kHz, both signals in one launch (skipped at 10 kHz)
    STOI       trunet_stoi_ragged: frame energies, silence mask + kept-frame lists, fused overlap-add + STFT + bands,
               segments, per-utterance means (five launches)
    SI-SDR     trunet_si_sdr_ragged: fp64 block partials at fs, then the per-utterance finalise (two launches)

Each utterance's results are bit for bit independent of its batch-mates and their order.

Command line (the ``eval.py`` role)::

    python -m tinyrecurrentunet_amd.evaluate --clean DIR --enhanced DIR [--noisy DIR] [--json PATH] [--max-seconds S]
"""
import argparse
import json
import math
import os
import re

import numpy as np
import torch

from . import _lib as L
from ._lib import check, ptr
from .enhance import _inputs

FS = 10000
N_FRAME, HOP, NFFT = 256, 128, 512
NUMBAND, MINFREQ, SEG = 15, 150, 30
SEG_WG = 64                  # metrics.hip: segments per workgroup
SDR_CHUNK = 16384            # metrics.hip: samples per SI-SDR partial
MAX_RATIO = 64
METRICS = ("stoi", "estoi", "si_sdr")


def ratio(fs):
    """10000 / fs in lowest terms -> (p, q); ValueError when p or q exceeds 64"""
    if isinstance(fs, bool) or int(fs) != fs or fs <= 0:
        raise ValueError("fs must be a positive integer sample rate, got %r" % (fs,))
    fs = int(fs)
    g = math.gcd(FS, fs)
    p, q = FS // g, fs // g
    if p > MAX_RATIO or q > MAX_RATIO:
        raise ValueError("fs = %d Hz: 10000/%d reduces to %d/%d, and resampling supports ratios up to %d/%d "
                         "(44.1 kHz and 22.05 kHz are not supported)" % (fs, fs, p, q, MAX_RATIO, MAX_RATIO))
    return p, q


def kaiser_filter(p, q):
    """the Octave-compatible Kaiser-windowed sinc of resample_poly, normalised to unit sum -> (float64 taps, half length)"""
    fc = 1.0 / (2 * max(p, q))
    half = math.ceil((60 - 8) / (28.714 * fc / 10))
    t = np.arange(-half, half + 1)
    h = np.kaiser(2 * half + 1, 0.1102 * (60 - 8.7)) * 2 * p * fc * np.sinc(2 * fc * t)
    return h / np.sum(h), half


def band_edges():
    """16 bins: third-octave band k covers rfft-512 bins [edges[k], edges[k+1]) at 10 kHz"""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    edges = [MINFREQ * 2.0 ** ((2 * k - 1) / 6) for k in range(NUMBAND)] + [MINFREQ * 2.0 ** ((2 * NUMBAND - 1) / 6)]
    return np.array([int(np.argmin((f - e) ** 2)) for e in edges], dtype=np.int64)


def window():
    return np.hanning(N_FRAME + 2)[1:-1]


def n_frames(n):
    """analysis frames range(0, n - 256, 128) of n samples at 10 kHz"""
    return max(0, -(-(n - N_FRAME) // HOP))


_CONST = {}


def _const(name, dev, make):
    key = (name, str(dev))
    if key not in _CONST:
        _CONST[key] = make()
    return _CONST[key]


def _check_args(clean, estimate, lengths, fs, metrics):
    """-> (clean list, estimate list, (p, q), metrics); raises before anything reaches the device"""
    if isinstance(metrics, str):
        metrics = (metrics,)
    metrics = tuple(metrics)
    for m in metrics:
        if m not in METRICS:
            raise ValueError("unknown metric %r: choose from %s (PESQ is not computed)" % (m, METRICS))
    if not metrics:
        raise ValueError("no metric asked for")
    pq = ratio(fs)
    xs, _ = _inputs(clean, lengths)
    ys, _ = _inputs(estimate, lengths)
    if len(xs) != len(ys):
        raise ValueError("%d clean and %d estimated utterances" % (len(xs), len(ys)))
    for b, (x, y) in enumerate(zip(xs, ys)):
        if x.shape[0] != y.shape[0]:
            raise ValueError("utterance %d: clean has %d samples, the estimate %d" % (b, x.shape[0], y.shape[0]))
    for b, (x, y) in enumerate(zip(xs, ys)):
        if not (x.is_cuda and y.is_cuda):
            raise L.TrunetHipError("tinyrecurrentunet_amd runs on MI355X only: utterance %d is on %s / %s"
                                   % (b, x.device, y.device))
    return xs, ys, pq, metrics


def _stoi_forward(sig, op, tot, p, q, B):
    """Steps 3 and 4 of ``evaluate`` on the packed (2, nS) signals -> (stoi, estoi, segments, sig10, workspace).  The
    workspace holds what trunet_stoi_ragged left (kept frames, counts, band magnitudes): stoi_loss.py's backward reads it,
    and shares this forward so that the loss scores are evaluate's bit for bit."""
    lib, st, dev = L.lib(), L.stream(), sig.device
    nS = tot[0]
    # 3. resample to 10 kHz (each plane of sig / sig10 is nS / nR wide whenever it holds a sample)
    nR = tot[2]
    if (p, q) == (1, 1) or nS == 0:
        sig10 = sig
    else:
        taps = _taps(p, q, dev)
        sig10 = torch.empty((2, nR), device=dev, dtype=torch.float32)
        check(lib.trunet_resample_ragged(ptr(sig), ptr(sig10), op[0], op[2], ptr(taps), (taps.shape[0] - 1) // 2, p, q, B,
                                         nS, nR, 2, st), "resample_ragged")

    # 4. STOI / ESTOI
    win, edges = _window_edges(dev)
    nF, nG, nC = tot[3], tot[4], tot[5]
    ws = torch.empty(int(lib.trunet_stoi_workspace_bytes(B, nF, nG)), device=dev, dtype=torch.uint8)
    stoi = torch.empty(B, device=dev, dtype=torch.float64)
    estoi = torch.empty(B, device=dev, dtype=torch.float64)
    segments = torch.empty(B, device=dev, dtype=torch.int64)
    check(lib.trunet_stoi_ragged(sig10.data_ptr(), op[2], op[3], op[4], op[5], ptr(win), edges.data_ptr(),
                                 ptr(L.twiddles(NFFT, dev)), ws.data_ptr(), stoi.data_ptr(), estoi.data_ptr(),
                                 segments.data_ptr(), B, nR, nF, nG, nC, st), "stoi_ragged")
    return stoi, estoi, segments, sig10, ws


def _window_edges(dev):
    return (_const("window", dev, lambda: torch.tensor(window(), dtype=torch.float32, device=dev)),
            _const("edges", dev, lambda: torch.tensor(band_edges(), dtype=torch.int32, device=dev)))


def _taps(p, q, dev):
    return _const(("taps", p, q), dev, lambda: torch.tensor(kaiser_filter(p, q)[0], dtype=torch.float32, device=dev))


def _tables(lens, p, q):
    """the six int64 prefix tables of a batch (samples, SI-SDR chunks, resampled samples, frames, segments, segment
    workgroups) -> (offs (6, B + 1) numpy, their totals)"""
    res = [-(-n * p // q) for n in lens]
    frames = [n_frames(r) for r in res]
    segs = [max(f - SEG, 0) for f in frames]
    rows = [lens, [-(-n // SDR_CHUNK) for n in lens], res, frames, segs, [-(-s // SEG_WG) for s in segs]]
    offs = np.zeros((6, len(lens) + 1), dtype=np.int64)
    offs[:, 1:] = np.cumsum(np.array(rows, dtype=np.int64), axis=1)
    return offs, [int(v) for v in offs[:, -1]]


@torch.no_grad()
def evaluate(clean, estimate, lengths=None, fs=16000, metrics=METRICS):
    """STOI / ESTOI / SI-SDR of every (clean, estimate) pair -> dict of (B,) cuda tensors (float64; ``segments`` int64)."""
    xs, ys, (p, q), metrics = _check_args(clean, estimate, lengths, fs, metrics)
    want_stoi = "stoi" in metrics or "estoi" in metrics
    dev = xs[0].device if xs else torch.device("cuda")
    B = len(xs)
    if B == 0:
        out = {m: torch.zeros(0, device=dev, dtype=torch.float64) for m in metrics}
        if want_stoi:
            out["segments"] = torch.zeros(0, device=dev, dtype=torch.int64)
        return out
    lib, st = L.lib(), L.stream()

    # 1. pack: sample, SI-SDR chunk, resampled sample, frame, segment and segment-workgroup prefix tables
    offs, tot = _tables([int(x.shape[0]) for x in xs], p, q)
    offs_d = torch.from_numpy(offs).to(dev)
    op = [offs_d[i].data_ptr() for i in range(6)]
    nS = tot[0]
    if nS:
        sig = torch.stack([torch.cat([x.to(device=dev, dtype=torch.float32) for x in v]) for v in (xs, ys)]).contiguous()
    else:
        sig = torch.zeros((2, 1), device=dev, dtype=torch.float32)
    out = {}

    # 2. SI-SDR at fs
    if "si_sdr" in metrics:
        partials = torch.empty(max(tot[1], 1) * 5, device=dev, dtype=torch.float64)
        out["si_sdr"] = torch.empty(B, device=dev, dtype=torch.float64)
        check(lib.trunet_si_sdr_ragged(sig[0].data_ptr(), sig[1].data_ptr(), op[0], op[1], partials.data_ptr(),
                                       out["si_sdr"].data_ptr(), B, nS, tot[1], st), "si_sdr_ragged")
    if not want_stoi:
        return out

    # 3., 4. resample to 10 kHz, then STOI / ESTOI
    stoi, estoi, segments = _stoi_forward(sig, op, tot, p, q, B)[:3]
    if "stoi" in metrics:
        out["stoi"] = stoi
    if "estoi" in metrics:
        out["estoi"] = estoi
    out["segments"] = segments
    return {k: out[k] for k in list(metrics) + ["segments"] if k in out}


def validate(net, noisy, clean, lengths=None, **enhance_kwargs):
    """Enhance ``noisy`` with ``net`` (enhance.enhance) and score both the noisy input and the result against ``clean``
    (16 kHz) -> {"noisy": metrics, "enhanced": metrics}."""
    from .enhance import enhance, SAMPLE_RATE
    _check_args(clean, noisy, lengths, SAMPLE_RATE, METRICS)
    est = enhance(net, noisy, lengths=lengths, **enhance_kwargs)
    return {"noisy": evaluate(clean, noisy, lengths, fs=SAMPLE_RATE),
            "enhanced": evaluate(clean, est, lengths, fs=SAMPLE_RATE)}


# ---------------------------------------------------------------- command line
_FILEID = re.compile(r"fileid_(\d+)")


def _fileid(name):
    ids = _FILEID.findall(os.path.splitext(name)[0])
    return ids[-1] if ids else None


def pair_files(clean_names, other_names):
    """Pair by identical name, failing that by the trailing ``fileid_<n>`` token (``clean_fileid_3.wav`` <->
    ``enhanced_fileid_3.wav``; a token shared by several files pairs nothing).  -> (sorted [(clean, other)], unmatched
    count over both folders)."""
    other = set(other_names)
    by_id = {}
    for nm in other_names:
        by_id.setdefault(_fileid(nm), []).append(nm)
    clean_ids = {}
    for nm in clean_names:
        clean_ids.setdefault(_fileid(nm), []).append(nm)
    pairs, used = [], set()
    for nm in sorted(clean_names):
        if nm in other:
            pairs.append((nm, nm))
            used.add(nm)
    done = {c for c, _ in pairs}
    for nm in sorted(clean_names):
        if nm in done:
            continue
        fid = _fileid(nm)
        cand = [o for o in by_id.get(fid, []) if o not in used] if fid is not None else []
        if len(cand) == 1 and len(clean_ids[fid]) == 1:
            pairs.append((nm, cand[0]))
            used.add(cand[0])
    pairs.sort()
    unmatched = (len(set(clean_names)) - len(pairs)) + (len(other) - len(used))
    return pairs, unmatched


def _wavs(d):
    return sorted(f for f in os.listdir(d) if f.lower().endswith(".wav"))


def score_folder(clean_dir, other_dir, max_seconds=600.0):
    """-> (per-file [(clean name, other name, {metric: value})], {metric: length-weighted mean}, unmatched count)"""
    from .dataset import _read_wav
    from .enhance import _batches
    pairs, unmatched = pair_files(_wavs(clean_dir), _wavs(other_dir))
    items = []
    for c, o in pairs:
        x, sx = _read_wav(os.path.join(clean_dir, c))
        y, sy = _read_wav(os.path.join(other_dir, o))
        if sx != sy:
            raise SystemExit("%s: %d Hz, but %s is %d Hz" % (os.path.join(other_dir, o), sy, c, sx))
        if x.shape[0] != y.shape[0]:
            raise SystemExit("%s: %d samples, but %s has %d" % (os.path.join(other_dir, o), y.shape[0], c, x.shape[0]))
        try:
            ratio(sx)
        except ValueError as e:
            raise SystemExit("%s: %s" % (c, e))
        items.append((c, o, x, y, sx))
    per = [None] * len(items)
    for rate in sorted({it[4] for it in items}):
        idx = [i for i, it in enumerate(items) if it[4] == rate]
        for chunk in _batches([items[i][2].shape[0] for i in idx], max(1, int(math.floor(max_seconds * rate)))):
            sel = [idx[k] for k in chunk]
            r = evaluate([items[i][2].cuda() for i in sel], [items[i][3].cuda() for i in sel], fs=rate)
            vals = {m: r[m].cpu().tolist() for m in METRICS}
            for k, i in enumerate(sel):
                per[i] = {m: vals[m][k] for m in METRICS}
    weights = np.array([it[2].shape[0] for it in items], dtype=np.float64)
    means = {}
    for m in METRICS:
        v = np.array([p[m] for p in per], dtype=np.float64)
        means[m] = float(np.sum(v * weights) / np.sum(weights)) if len(items) else float("nan")
    return [(it[0], it[1], p) for it, p in zip(items, per)], means, unmatched


def format_means(means):
    """eval.py's line: ``stoi = 0.xxx, estoi = 0.xxx, si_sdr = xx.xxx, ``"""
    return "".join("{} = {:.3f}, ".format(m, means[m]) for m in METRICS)


def main(argv=None):
    ap = argparse.ArgumentParser(
        prog="python -m tinyrecurrentunet_amd.evaluate",
        description="Score enhanced speech against clean references on the GPU: STOI, ESTOI and SI-SDR, length-weighted "
                    "means over the files (the role of eval.py).  PESQ is not computed.  Files pair by identical name, "
                    "failing that by their trailing fileid_<n> token; unmatched files are skipped and counted.")
    ap.add_argument("--clean", required=True, help="folder of clean reference *.wav")
    ap.add_argument("--enhanced", required=True, help="folder of enhanced *.wav")
    ap.add_argument("--noisy", help="folder of noisy *.wav, scored the same way for comparison")
    ap.add_argument("--json", help="write the per-file values and the means of every scored folder here")
    ap.add_argument("--max-seconds", type=float, default=600.0, help="audio per evaluate() call (default 600 s)")
    args = ap.parse_args(argv)
    if not args.max_seconds > 0:
        ap.error("--max-seconds must be positive")
    for d in [args.clean, args.enhanced] + ([args.noisy] if args.noisy else []):
        if not os.path.isdir(d):
            ap.error("%s is not a folder" % d)
    report = {}
    for label, d in [("noisy", args.noisy), ("enhanced", args.enhanced)]:
        if d is None:
            continue
        files, means, unmatched = score_folder(args.clean, d, args.max_seconds)
        report[label] = {"folder": d, "means": means, "files": len(files), "unmatched": unmatched,
                         "per_file": [dict(clean=c, file=o, **v) for c, o, v in files]}
        print("%s (%d files, %d unmatched skipped): %s" % (label, len(files), unmatched, format_means(means)))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
