"""Time of the reverberant input stage on one MI355X; prints one JSON line per configuration.

What GpuPairLoader stages per batch with ``reverb=`` / ``snr_db=`` set: noise augmentation (trunet_augment_mix), RIR
convolution with an early-reflections target, SNR mixing and the peak guard (trunet_reverb_mix), timed together with device
events: --warmup calls, then --reps timed calls, median and p10 / p90; the two entry points are also timed alone.  Next to
it, scipy.signal.fftconvolve of the same batch (the convolution only) on a pool of --cpu-workers processes, which is what
the stage would cost in DataLoader workers.  The CPU part runs first, before the GPU is opened.

    python scripts/bench_reverb.py [--reps 50] [--warmup 10] [--cpu-workers 16] [--gpu-only]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR = 16000
CONFIGS = [(64, 64000, 16000), (64, 64000, 4000), (64, 96000, 24000)]      # B, L, RIR taps


def _cpu_one(args):
    from scipy.signal import fftconvolve
    x, h = args
    return fftconvolve(x, h)[:len(x)].astype(np.float32)


def cpu_seconds(x, h, workers, reps=3):
    best = None
    with ProcessPoolExecutor(workers) as ex:
        list(ex.map(_cpu_one, zip(x[:workers], h[:workers])))               # start the pool, import scipy
        for _ in range(reps):
            t0 = time.perf_counter()
            list(ex.map(_cpu_one, zip(x, h), chunksize=max(len(x) // workers, 1)))
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
    return best


def timed(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median": round(float(np.median(ms)), 4), "p10": round(float(np.percentile(ms, 10)), 4),
            "p90": round(float(np.percentile(ms, 90)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cpu-workers", type=int, default=16)
    ap.add_argument("--gpu-only", action="store_true", help="skip the CPU figure (profiling runs)")
    args = ap.parse_args()

    from tinyrecurrentunet_amd import dataset as ds
    data, cpu = [], []
    for B, Ln, K in CONFIGS:
        g = np.random.default_rng(B + Ln + K)
        x = (0.1 * g.standard_normal((B, Ln))).astype(np.float32)
        v = (0.05 * g.standard_normal((B, Ln))).astype(np.float32)
        rv = ds.Reverb(sample_rate=SR, max_rir_sec=K / SR, target="early")
        h = np.stack([rv.synthetic(b, K / SR, 3.0 + b % 10) for b in range(B)]).astype(np.float32)
        assert h.shape == (B, K)
        data.append((x, v, h, rv))
        cpu.append(None if args.gpu_only else cpu_seconds(x, h, args.cpu_workers))

    import torch
    from tinyrecurrentunet_amd import _lib as L
    if not torch.cuda.is_available():
        raise SystemExit("bench_reverb.py measures the GPU stage and needs the MI355X")
    aug = ds.DataAugment()
    for (B, Ln, K), (x, v, h, rv), cpu_s in zip(CONFIGS, data, cpu):
        random_params = np.stack([aug.params(8000.0 + 100 * (b % 20), 800.0 + 50 * (b % 8), -12.0 + 0.5 * (b % 14))
                                  for b in range(B)])
        clean = torch.from_numpy(x).cuda().unsqueeze(1)
        noise = torch.from_numpy(v).cuda()
        par = torch.from_numpy(random_params).cuda()
        rirs = torch.from_numpy(h).cuda()
        lens = torch.full((B,), K, dtype=torch.int32, device="cuda")
        snr = torch.linspace(0.0, 20.0, B, device="cuda")
        augd = torch.empty_like(noise)

        def augment():
            L.check(L.lib().trunet_augment_mix(L.ptr(noise), None, L.ptr(par), L.ptr(augd), None, B, Ln, L.stream()), "augment")

        def reverb():
            return rv(clean, rirs, lens, noise=augd, snr_db=snr)

        def stage():
            augment()
            return reverb()

        res = {"metric": "reverb_stage_ms", "B": B, "L": Ln, "rir_taps": K, "early_taps": rv.early_taps,
               "warmup": args.warmup, "reps": args.reps, "stage_ms": timed(stage, args.warmup, args.reps),
               "augment_ms": timed(augment, 3, args.reps), "reverb_mix_ms": timed(reverb, 3, args.reps),
               "workspace_mib": round(L.lib().trunet_reverb_workspace_bytes(B, Ln, K) / 2 ** 20, 1)}
        noisy, target = stage()
        assert bool(torch.isfinite(noisy).all()) and bool(torch.isfinite(target).all())
        if cpu_s is not None:
            res.update({"cpu_workers": args.cpu_workers, "cpu_fftconvolve_ms": round(cpu_s * 1e3, 2),
                        "gpu_speedup_vs_cpu": round(cpu_s * 1e3 / res["stage_ms"]["median"], 1)})
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
