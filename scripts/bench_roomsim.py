"""Time of the room simulator on one MI355X; prints one JSON line per configuration.

64 rooms drawn by ``RoomSim.draw()`` (rt60 uniform in 0.2 .. 1.0 s, 1 s of RIR at 16 kHz) at ism_ms = 50, 80 and 200:
``trunet_rir_ism`` alone, and followed by ``trunet_reverb_mix`` on 4 s signals with the early target, which is what
``Reverb(room=...)`` runs per batch.  Device events, --warmup calls, then --reps timed calls; median and p10 / p90.  Next to
it the only CPU alternative there is, the vectorised numpy restatement (tests/roomsim_ref.py) of the same rows on a pool of
--cpu-workers processes.  The CPU part runs first, before the GPU is opened.

    python scripts/bench_roomsim.py [--reps 50] [--warmup 10] [--cpu-workers 16] [--gpu-only]
"""
import argparse
import json
import os
import random
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SR, B, LN = 16000, 64, 64000
ISM_MS = (50.0, 80.0, 200.0)


def _cpu_one(args):
    import roomsim_ref as rr
    row, ism_ms = args
    o = rr.rir(row, fs=SR, ism_ms=ism_ms, max_rir_sec=1.0)
    return o["images"]


def cpu_seconds(rows, ism_ms, workers, reps=2):
    best, images = None, 0
    with ProcessPoolExecutor(workers) as ex:
        list(ex.map(_cpu_one, [(r, 10.0) for r in rows[:workers]]))           # start the pool, import numpy
        for _ in range(reps):
            t0 = time.perf_counter()
            images = sum(ex.map(_cpu_one, [(r, ism_ms) for r in rows]))
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
    return best, images


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
    random.seed(64)
    rows = [ds.RoomSim(sample_rate=SR).draw().numpy() for _ in range(B)]
    cpu = [None if args.gpu_only else cpu_seconds(rows, ms, args.cpu_workers) for ms in ISM_MS]

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_roomsim.py measures the GPU stage and needs the MI355X")
    g = np.random.default_rng(0)
    clean = torch.from_numpy((0.1 * g.standard_normal((B, 1, LN))).astype(np.float32)).cuda()
    noise = torch.from_numpy((0.05 * g.standard_normal((B, 1, LN))).astype(np.float32)).cuda()
    snr = torch.linspace(0.0, 20.0, B, device="cuda")
    rows_d = torch.from_numpy(np.stack(rows)).cuda()
    for ism_ms, cpu_r in zip(ISM_MS, cpu):
        sim = ds.RoomSim(sample_rate=SR, ism_ms=ism_ms)
        rv = ds.Reverb(sample_rate=SR, room=sim, target="early", early_ms=50.0)

        def simulate():
            return sim(rows_d)

        def stage():
            return rv(clean, rows_d, None, noise=noise, snr_db=snr)

        res = {"metric": "roomsim_ms", "B": B, "L": LN, "ism_ms": ism_ms, "n_c": sim.n_c, "rir_taps": sim.max_taps,
               "warmup": args.warmup, "reps": args.reps, "rir_ism_ms": timed(simulate, args.warmup, args.reps),
               "rir_ism_plus_reverb_mix_ms": timed(stage, args.warmup, args.reps)}
        h, lens = simulate()
        noisy, target = stage()
        assert bool(torch.isfinite(h).all()) and int(lens.min()) >= 3200
        assert bool(torch.isfinite(noisy).all()) and bool(torch.isfinite(target).all())
        if cpu_r is not None:
            res.update({"cpu_workers": args.cpu_workers, "cpu_numpy_ms": round(cpu_r[0] * 1e3, 1), "images": cpu_r[1],
                        "gpu_speedup_vs_cpu": round(cpu_r[0] * 1e3 / res["rir_ism_ms"]["median"], 1)})
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
