"""The int8 artefact (quantize.QuantizedTRUNet, stream_fwd_i8.hip) against the default fp32 artefact (export.FoldedTRUNet, the
x3 kernel) on one MI355X, in the same process; one JSON line per measurement.

  forward   ms per call at 1024 and 8192 frames (C_in = 4), device events around each repetition after a warm-up, median
  enhance   150 x 10 s through enhance(path="int8") and enhance(path="folded") (the int8 route quantizes once per call)

    python scripts/bench_int8.py [--reps 20] [--frames 1024,8192] [--enhance-reps 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import network_ref as nr, weights as W                   # noqa: E402
from tinyrecurrentunet_amd import network as hn                       # noqa: E402
from tinyrecurrentunet_amd.export import FoldedTRUNet                 # noqa: E402
from tinyrecurrentunet_amd.quantize import QuantizedTRUNet            # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", default="1024,8192")
    ap.add_argument("--enhance-reps", type=int, default=3)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    net = hn.TRUNet(input_size=4)
    net.load_state_dict(W.fill_state_dict(nr.TRUNet(input_size=4), seed=0).state_dict())
    net.cuda().eval()
    f32 = FoldedTRUNet.from_module(net)
    q8 = QuantizedTRUNet.from_module(net)
    print(json.dumps({"artefact": "int8", "bytes": q8.nbytes, "fp32_bytes": 4 * f32.blob.numel()}))
    for n in [int(v) for v in args.frames.split(",")]:
        x = torch.randn(n, 4, 257, generator=torch.Generator().manual_seed(n)).cuda()
        t8 = timed(lambda: q8(x), args.reps)
        t32 = timed(lambda: f32(x), args.reps)
        print(json.dumps({"case": "forward", "frames": n, "int8_ms": round(t8, 4), "fp32_x3_ms": round(t32, 4),
                          "speedup": round(t32 / t8, 3), "int8_x_real_time": round(n * 0.008 / (t8 * 1e-3), 1)}))
    g = np.random.default_rng(0)
    xs = [torch.tensor(g.standard_normal(160000) * 0.1, dtype=torch.float32).cuda() for _ in range(150)]
    with torch.no_grad():
        t8 = timed(lambda: net.enhance(xs, path="int8"), args.enhance_reps)
        t32 = timed(lambda: net.enhance(xs, path="folded"), args.enhance_reps)
    print(json.dumps({"case": "enhance 150 x 10 s", "int8_ms": round(t8, 2), "folded_ms": round(t32, 2),
                      "speedup": round(t32 / t8, 3), "int8_x_real_time": round(1500.0 / (t8 * 1e-3), 1)}))


if __name__ == "__main__":
    main()
