"""Cost of a stream pool at 48 and 44.1 kHz (tinyrecurrentunet_amd/streaming.py: StreamPool(fs=); resample.py:
StreamResampler, resample.hip) on one MI355X; prints one JSON line.

Device events around a call, median of --reps after a warm-up, as bench_resample.py does it (DESIGN section 3m quotes them):

    pool        --sessions sessions in steady state, one 20 ms packet each per call: pool.feed at 48 kHz (960 samples) and at
                44.1 kHz (882) against the unchanged pool.feed at 16 kHz (320), the three alternating in one run
    resampler   StreamResampler.feed alone on such packets, its plan copy and two launches without the host's planning,
                and Resampler on the same samples in one offline call: 48 -> 16, 44.1 -> 16, 16 -> 48 and 16 -> 44.1 kHz,
                alternating

    python scripts/bench_stream_resample.py [--only pool,resampler] [--sessions 1024] [--reps 5] [--cin 4] [--tgru]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SECTIONS = ("pool", "resampler")
PACKET_MS = 20


def timed_once(fn):
    """(device-event ms, host ms until the call returned) of one fn()"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    host = (time.perf_counter() - t0) * 1e3
    b.synchronize()
    return a.elapsed_time(b), host


def stats(ms):
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def alternate(fns, reps, warmup):
    """{name: fn} -> {name: stats}; the calls alternate, `warmup` untimed rounds first"""
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    dev, host = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            d, h = timed_once(fn)
            dev[k].append(d)
            host[k].append(h)
    return {k: dict(stats(dev[k]), host_ms_median=round(float(np.median(host[k])), 4)) for k in fns}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=",".join(SECTIONS))
    ap.add_argument("--sessions", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=12, help="untimed calls per pool: the sessions reach their steady state")
    ap.add_argument("--cin", type=int, default=4)
    ap.add_argument("--tgru", action="store_true")
    args = ap.parse_args()
    only = [s for s in args.only.split(",") if s]
    for s in only:
        if s not in SECTIONS:
            ap.error("unknown section %r" % s)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream_resample.py measures GPU launches and needs the MI355X")
    from tinyrecurrentunet_amd import resample as R
    S = args.sessions
    res = {"metric": "stream_resample", "sessions": S, "packet_ms": PACKET_MS, "reps": args.reps, "cin": args.cin,
           "tgru": args.tgru}
    ids = list(range(S))

    if "pool" in only:
        from tinyrecurrentunet_amd.network import TRUNet
        torch.manual_seed(0)
        net = TRUNet(input_size=args.cin, use_tgru=args.tgru).cuda().eval()
        fns = {}
        for fs in (16000, 48000, 44100):
            n = fs * PACKET_MS // 1000
            pool = net.stream_pool(S, fs=fs)
            assert pool.open(S) == ids
            packed = 0.1 * torch.randn(S * n, device="cuda")
            lens = np.full(S, n, dtype=np.int64)
            fns["fs_%d" % fs] = (lambda pool=pool, packed=packed, lens=lens: pool.feed((packed, lens), ids))
        row = alternate(fns, args.reps, args.warmup)
        for fs in (48000, 44100):
            row["fs_%d" % fs]["over_16000_ms"] = round(row["fs_%d" % fs]["ms_median"] - row["fs_16000"]["ms_median"], 4)
        row["spread_16000_ms"] = round(row["fs_16000"]["ms_max"] - row["fs_16000"]["ms_min"], 4)
        res["pool"] = row

    if "resampler" in only:
        res["resampler"] = {}
        for fs_in, fs_out in ((48000, 16000), (44100, 16000), (16000, 48000), (16000, 44100)):
            n = fs_in * PACKET_MS // 1000
            sr = R.StreamResampler(fs_in, fs_out, S)
            rs = R.Resampler(fs_in, fs_out, "cuda")
            packed = torch.randn(S * n, device="cuda")
            lens = np.full(S, n, dtype=np.int64)
            outs, offs = rs.plan([n] * S)
            offs_d = torch.from_numpy(offs).cuda()
            sr.feed((packed, lens), ids)                                    # past the look-ahead: every call owes its share
            idv = np.arange(S, dtype=np.int64)
            fixed = sr.plan(lens, idv)                                      # one plan again and again: the copy and the launches
            row = alternate({"stream_feed": lambda: sr.feed((packed, lens), ids),
                             "stream_launches_only": lambda: sr.run(fixed, packed, idv),
                             "offline_one_call": lambda: rs.packed(packed.view(1, -1), offs, 1, offs_d)}, args.reps, args.warmup)
            row.update(p=sr.p, q=sr.q, history=sr.H, samples_in=S * n, outputs_per_call=int(offs[1, -1]))
            res["resampler"]["%d->%d" % (fs_in, fs_out)] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
