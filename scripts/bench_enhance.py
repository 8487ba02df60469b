"""Throughput of offline enhancement (tinyrecurrentunet_amd/enhance.py) on one MI355X; one JSON line per measurement.

Cases (16 kHz):
  a       150 x 10 s, the DNS synthetic test-set shape
  b       a ragged mix of 1-30 s files totalling about 1,500 s
  c       case a with a use_tgru net
For each: frames/s and x real time of the whole enhance() call, the same for the bare network calls it wraps (the same
chunks on precomputed features), the share of the ragged front + back end, and (c) the TGRU padding fraction.  Device
events around each timed repetition, after a warm-up call.

    python scripts/bench_enhance.py [--cases a,b,c] [--reps 5] [--paths folded,layers] [--max-frames 8192]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tinyrecurrentunet_amd import enhance as en                      # noqa: E402
from tinyrecurrentunet_amd.network import TRUNet                      # noqa: E402

SR = 16000


def lengths(case):
    if case in ("a", "c"):
        return [10 * SR] * 150
    g = np.random.default_rng(0)
    out, tot = [], 0
    while tot < 1500 * SR:
        n = int(g.uniform(1, 30) * SR) + int(g.integers(0, 128))
        out.append(n)
        tot += n
    return out


def timed(fn, reps):
    fn()                                                             # warm-up (artefact, scratch, engine buffers)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--paths", default="folded,layers")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-frames", default="8192", help="comma-separated list")
    ap.add_argument("--input-size", type=int, default=4)
    args = ap.parse_args()
    torch.manual_seed(0)
    for case in args.cases.split(","):
        tgru = case == "c"
        net = TRUNet(input_size=args.input_size, use_tgru=tgru).cuda().eval()
        lens = lengths(case)
        g = np.random.default_rng(1)
        xs = [torch.tensor(g.standard_normal(n) * 0.1, dtype=torch.float32).cuda() for n in lens]
        frames = sum(en.n_frames(n) for n in lens)
        seconds = sum(lens) / SR
        pk = en.Packed(xs, xs[0].device)
        with torch.no_grad():
            feat = en.features(pk, args.input_size)
        paths = ["layers"] if tgru else args.paths.split(",")
        for path in paths:
            for mf in (int(v) for v in args.max_frames.split(",")):
                with torch.no_grad():
                    if tgru:
                        _, pad = en.tgru_groups([en.n_frames(n) for n in lens], mf)
                        net_fn = lambda: en._tgru_forward(net, feat, pk.frames, pk.offs[1], mf)
                    else:
                        pad = 0.0
                        run = net.folded()
                        if path == "layers":
                            if net._engine is None:
                                object.__setattr__(net, "_engine", net._make_engine())
                            eng = net._engine
                            run = lambda v: eng.forward(v, False)[0]
                        net_fn = lambda: [run(feat[i:i + mf]) for i in range(0, pk.nT, mf)]
                    out = torch.cat(net_fn()) if not tgru else net_fn()
                    front_ms, _ = timed(lambda: en.features(en.Packed(xs, xs[0].device), args.input_size), args.reps)
                    back_ms, _ = timed(lambda: en.mask_istft(pk, out), args.reps)
                    bare_ms, _ = timed(net_fn, args.reps)
                    full_ms, _ = timed(lambda: en.enhance(net, xs, max_frames=mf, path=path), args.reps)
                rec = dict(case=case, path=path, max_frames=mf, utterances=len(lens), seconds=round(seconds, 1),
                           frames=frames, enhance_ms=round(full_ms, 3), enhance_frames_per_s=round(frames / full_ms * 1e3),
                           enhance_x_realtime=round(seconds / full_ms * 1e3), net_ms=round(bare_ms, 3),
                           net_frames_per_s=round(frames / bare_ms * 1e3), ratio_vs_net=round(bare_ms / full_ms, 4),
                           front_ms=round(front_ms, 3), back_ms=round(back_ms, 3),
                           front_back_share=round((front_ms + back_ms) / full_ms, 4), tgru_padding=round(pad, 4))
                print(json.dumps(rec), flush=True)
                del out


if __name__ == "__main__":
    main()
