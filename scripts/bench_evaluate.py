"""Throughput of GPU scoring (tinyrecurrentunet_amd/evaluate.py) on one MI355X; prints one JSON line.

300 pairs of 10 s at 16 kHz (the size of the DNS no-reverb test set eval.py loops over): device-event time of one
evaluate() call (STOI, ESTOI, SI-SDR) after a warm-up call, as pairs/s and x real time; and the wall time of the same
pairs in the float64 restatement (tests/metrics_ref.py) on a pool of --cpu-workers processes.  The per-kernel split comes
from a separate run under rocprofv3 with --gpu-only:

    python scripts/bench_evaluate.py [--pairs 300] [--seconds 10] [--reps 5] [--cpu-workers 16]
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/bench_evaluate.py --gpu-only --reps 3
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tinyrecurrentunet_amd.evaluate import evaluate          # noqa: E402

SR = 16000


def pairs(n, seconds, seed=0):
    """speech-like clean signals (harmonics + noise, syllable envelope, silent stretches) and noisy estimates"""
    g = np.random.default_rng(seed)
    L = int(seconds * SR)
    t = np.arange(L) / SR
    xs, ys = [], []
    for i in range(n):
        ph = 2 * np.pi * np.cumsum(g.uniform(90, 200) * (1 + 0.1 * np.sin(2 * np.pi * 0.5 * t))) / SR
        v = sum(np.sin(h * ph) / h for h in range(1, 30)) + 0.3 * g.standard_normal(L)
        env = np.sin(2 * np.pi * g.uniform(3, 5) * t) ** 2 * (np.floor(t / 1.5) % 3 != 2)
        x = (0.2 * v * env).astype(np.float32)
        xs.append(x)
        ys.append((x + g.standard_normal(L) * 0.02 * (1 + i % 5)).astype(np.float32))
    return xs, ys


def _ref_one(args):
    import metrics_ref
    x, y = args
    return metrics_ref.metrics_ref(x.astype(np.float64), y.astype(np.float64), SR)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=300)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-workers", type=int, default=16)
    ap.add_argument("--gpu-only", action="store_true", help="skip the CPU restatement (profiling runs)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_evaluate.py measures the GPU call and needs the MI355X")
    xs, ys = pairs(args.pairs, args.seconds)
    X = [torch.from_numpy(x).cuda() for x in xs]
    Y = [torch.from_numpy(y).cuda() for y in ys]
    out = evaluate(X, Y)                                        # warm-up: code objects, caching allocator
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = evaluate(X, Y)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    med = float(np.median(ms))
    audio_s = args.pairs * args.seconds
    res = {"metric": "evaluate_pairs_per_s", "pairs": args.pairs, "seconds_each": args.seconds,
           "gpu_ms_median": round(med, 3), "gpu_ms_min": round(min(ms), 3), "reps": args.reps,
           "pairs_per_s": round(args.pairs / (med / 1e3), 1), "x_real_time": round(audio_s / (med / 1e3), 1),
           "mean_stoi": round(float(out["stoi"].mean()), 4), "mean_estoi": round(float(out["estoi"].mean()), 4),
           "mean_si_sdr": round(float(out["si_sdr"].mean()), 3)}
    if not args.gpu_only:
        t0 = time.perf_counter()
        with ProcessPoolExecutor(args.cpu_workers) as ex:
            ref = list(ex.map(_ref_one, zip(xs, ys), chunksize=4))
        cpu_s = time.perf_counter() - t0
        res.update({"cpu_workers": args.cpu_workers, "cpu_float64_s": round(cpu_s, 2),
                    "cpu_pairs_per_s": round(args.pairs / cpu_s, 2), "gpu_speedup_vs_cpu": round(cpu_s / (med / 1e3), 1),
                    "max_abs_stoi_diff": float(max(abs(r["stoi"] - v) for r, v in zip(ref, out["stoi"].tolist()))),
                    "max_abs_estoi_diff": float(max(abs(r["estoi"] - v) for r, v in zip(ref, out["estoi"].tolist()))),
                    "max_abs_si_sdr_diff": float(max(abs(r["si_sdr"] - v) for r, v in zip(ref, out["si_sdr"].tolist())))})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
