"""Throughput of the GPU resampler (tinyrecurrentunet_amd/resample.py, resample.hip) on one MI355X; prints one JSON line.

Device-event times, median of --reps after a warm-up (DESIGN section 3l quotes them):

    kernel    300 utterances of 10 s, one plane: 48 -> 16, 44.1 -> 16, 16 -> 48 and 16 -> 44.1 kHz, ms per launch and GB/s of
              input plus output; scipy.signal.resample_poly with the same taps on --cpu-workers processes
    ab        48 -> 16 kHz with identical taps: trunet_resample_rational against trunet_resample_ragged (evaluate's
              kernel, one global load per tap), alternating in one run
    taps      44.1 <-> 16 kHz with the tap table in LDS and read from L2
    enhance   enhance(fs=48000) against enhance at 16 kHz on the same recordings, already resampled
    loader    one GPU stage of the input pipeline, 64 x 4 s, from 48 kHz files with resample_to=16000 and from 16 kHz files

    python scripts/bench_resample.py [--only kernel,ab,taps,enhance,loader] [--utterances 300] [--seconds 10] [--reps 5]
"""
import argparse
import json
import multiprocessing
import os
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SECTIONS = ("kernel", "ab", "taps", "enhance", "loader")
_X = {}


def _cpu_init(n, p, q):
    from tinyrecurrentunet_amd.resample import design
    _X["x"] = np.random.default_rng(os.getpid()).standard_normal(n).astype(np.float32)
    _X["h"] = design(p, q)[0]
    _X["pq"] = (p, q)


def _cpu_one(_):
    from scipy.signal import resample_poly
    p, q = _X["pq"]
    return resample_poly(_X["x"], p, q, window=_X["h"]).shape[0]


def cpu_seconds(n, p, q, utterances, workers):
    """wall time of `utterances` resample_poly calls on a pool of `workers` processes, after one call per worker"""
    with ProcessPoolExecutor(workers, mp_context=multiprocessing.get_context("spawn"), initializer=_cpu_init,
                             initargs=(n, p, q)) as ex:
        list(ex.map(_cpu_one, range(4 * workers)))
        t0 = time.perf_counter()
        list(ex.map(_cpu_one, range(utterances), chunksize=2))
        return time.perf_counter() - t0


def timed(fn, reps):
    """device-event ms of fn(), `reps` times after one warm-up call"""
    import torch
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
    return ms


def stats(ms):
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def launch(rs, sig, offs, offs_d, nsig=1):
    return lambda: rs.packed(sig, offs, nsig, offs_d)


def setup(R, torch, fs_in, fs_out, utterances, seconds, **kw):
    rs = R.Resampler(fs_in, fs_out, "cuda", **kw)
    n = int(seconds * fs_in)
    outs, offs = rs.plan([n] * utterances)
    sig = torch.randn((1, utterances * n), device="cuda")
    return rs, n, sig, offs, torch.from_numpy(offs).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=",".join(SECTIONS))
    ap.add_argument("--utterances", type=int, default=300)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-workers", type=int, default=16)
    ap.add_argument("--gpu-only", action="store_true", help="skip scipy on the CPU")
    args = ap.parse_args()
    only = [s for s in args.only.split(",") if s]
    for s in only:
        if s not in SECTIONS:
            ap.error("unknown section %r" % s)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py measures GPU launches and needs the MI355X")
    from tinyrecurrentunet_amd import _lib as L, resample as R
    from tinyrecurrentunet_amd._lib import check, ptr
    U, S = args.utterances, args.seconds
    res = {"metric": "resample", "utterances": U, "seconds_each": S, "reps": args.reps}

    if "kernel" in only:
        res["kernel"] = {}
        for fs_in, fs_out in ((48000, 16000), (44100, 16000), (16000, 48000), (16000, 44100)):
            rs, n, sig, offs, offs_d = setup(R, torch, fs_in, fs_out, U, S)
            ms = timed(launch(rs, sig, offs, offs_d), args.reps)
            byts = 4 * (int(offs[0, -1]) + int(offs[1, -1]))
            row = dict(stats(ms), p=rs.p, q=rs.q, tile=rs.tile, taps_in_lds=rs.lds_taps,
                       gb_per_s=round(byts / (float(np.median(ms)) * 1e-3) / 1e9, 1),
                       x_real_time=round(U * S / (float(np.median(ms)) * 1e-3), 0))
            if not args.gpu_only:
                cpu = cpu_seconds(n, rs.p, rs.q, U, args.cpu_workers)
                row.update(cpu_workers=args.cpu_workers, scipy_ms=round(cpu * 1e3, 1),
                           gpu_speedup_vs_scipy=round(cpu * 1e3 / float(np.median(ms)), 1))
            res["kernel"]["%d->%d" % (fs_in, fs_out)] = row
            del sig

    if "ab" in only:
        # identical taps (design(1, 3): half = 48, 97 taps) through both kernels, alternating
        rs, n, sig, offs, offs_d = setup(R, torch, 48000, 16000, U, S)
        taps = torch.tensor(R.design(1, 3)[0], dtype=torch.float32, device="cuda")
        nI, nO = int(offs[0, -1]), int(offs[1, -1])
        old_out = torch.empty((1, nO), device="cuda")

        def old():
            check(L.lib().trunet_resample_ragged(ptr(sig), ptr(old_out), offs_d[0].data_ptr(), offs_d[1].data_ptr(),
                                                 ptr(taps), rs.half, rs.p, rs.q, U, nI, nO, 1, L.stream()), "resample_ragged")
        new = launch(rs, sig, offs, offs_d)
        old(), new()
        torch.cuda.synchronize()
        ms_old, ms_new = [], []
        for _ in range(args.reps):
            ms_old += timed(old, 1)
            ms_new += timed(new, 1)
        diff = float((rs.packed(sig, offs, 1, offs_d) - old_out).abs().max())
        res["ab_48_to_16"] = {"resample_ragged": stats(ms_old), "resample_rational": stats(ms_new),
                              "old_spread_ms": round(max(ms_old) - min(ms_old), 4),
                              "new_minus_old_ms": round(float(np.median(ms_new) - np.median(ms_old)), 4),
                              "max_abs_diff": diff}
        del sig, old_out

    if "taps" in only:
        res["taps"] = {}
        for fs_in, fs_out in ((44100, 16000), (16000, 44100)):
            row = {}
            for name, lds in (("lds", True), ("l2", False)):
                rs, n, sig, offs, offs_d = setup(R, torch, fs_in, fs_out, U, S, lds_taps=lds)
                row[name] = stats(timed(launch(rs, sig, offs, offs_d), args.reps))
                del sig
            res["taps"]["%d->%d" % (fs_in, fs_out)] = row

    if "enhance" in only:
        from tinyrecurrentunet_amd.enhance import enhance
        from tinyrecurrentunet_amd.network import TRUNet
        torch.manual_seed(0)
        net = TRUNet(input_size=4).cuda().eval()
        x48 = [0.1 * torch.randn(int(S * 48000), device="cuda") for _ in range(U)]
        x16 = R.resample(x48, 48000, 16000)
        res["enhance"] = {"fs_48000": stats(timed(lambda: enhance(net, x48, fs=48000), args.reps)),
                          "fs_16000": stats(timed(lambda: enhance(net, x16), args.reps))}
        res["enhance"]["resampling_share"] = round(1.0 - res["enhance"]["fs_16000"]["ms_median"] /
                                                   res["enhance"]["fs_48000"]["ms_median"], 4)
        del x48, x16

    if "loader" in only:
        from scipy.io.wavfile import write as wavwrite
        from tinyrecurrentunet_amd import dataset as ds
        res["loader"] = {}
        g = np.random.default_rng(0)
        with tempfile.TemporaryDirectory() as tmp:
            for rate, kw in ((48000, {"resample_to": 16000}), (16000, {})):
                root = os.path.join(tmp, str(rate))
                os.makedirs(os.path.join(root, "clean"))
                os.makedirs(os.path.join(root, "keyboard"))
                for i in range(64):
                    wavwrite(os.path.join(root, "clean", "fileid_%d.wav" % i), rate,
                             (3000 * g.standard_normal(4 * rate)).astype(np.int16))
                wavwrite(os.path.join(root, "keyboard", "k.wav"), rate, (1000 * g.standard_normal(4 * rate)).astype(np.int16))
                loader = ds.load_CleanNoisyPairDataset(root, "training", 0, 64, rate, num_workers=0, **kw)
                batch = next(iter(loader.loader))
                side = torch.cuda.Stream()

                def stage():
                    side.wait_stream(torch.cuda.current_stream())
                    out = loader._stage(batch, side)
                    torch.cuda.current_stream().wait_event(out[3])
                    return out
                key = "from_%d%s" % (rate, "_resample_to_16000" if kw else "")
                res["loader"][key] = dict(stats(timed(stage, args.reps)), clean_shape=list(stage()[0].shape))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
