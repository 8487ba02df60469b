"""Cost of the band above 8 kHz in a stream pool at 48 kHz (tinyrecurrentunet_amd/stream_highband.py, stream_highband.hip;
StreamPool(highband=)) on one MI355X; prints one JSON line.  DESIGN section 3r quotes the figures.

Device events around a call, median of --reps after a warm-up, as bench_stream_resample.py does it:

    modes       --sessions sessions in steady state, one 20 ms packet (960 samples) each per call: pool.feed with
                highband "drop", "keep" and "follow", the three alternating in one process; the yardstick of the new modes
                is "drop" in the same run
    launches    what "keep" and "follow" add on the device alone: the plan copy and the launches of StreamHighband.run on
                such a call (pairing, the lo plane of the up-resampler, gains, join, commit), one plan reused, without the
                host's planning

Each section runs in a child process of its own under --timeout seconds; the first that fails ends the run.  The yardstick of
"drop" itself is the commit before: scripts/bench_stream_resample.py --only pool there and here, a process each, alternating.

    python scripts/bench_stream_highband.py [--only modes,launches] [--sessions 1024] [--reps 7] [--cin 4] [--tgru]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SECTIONS = ("modes", "launches")
MODES = ("drop", "keep", "follow")
FS, PACKET_MS = 48000, 20


def section(name, args):
    import torch
    from bench_stream_resample import alternate
    from tinyrecurrentunet_amd.network import TRUNet
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream_highband.py measures GPU launches and needs the MI355X")
    S, n = args.sessions, FS * PACKET_MS // 1000
    ids = list(range(S))
    idv = np.arange(S, dtype=np.int64)
    lens = np.full(S, n, dtype=np.int64)
    torch.manual_seed(0)
    net = TRUNet(input_size=args.cin, use_tgru=args.tgru).cuda().eval()
    packed = 0.1 * torch.randn(S * n, device="cuda")
    pools = {}
    for mode in MODES:
        pools[mode] = net.stream_pool(S, fs=FS, highband=mode)
        assert pools[mode].open(S) == ids
    if name == "modes":
        row = alternate({m: (lambda pool=pools[m]: pool.feed((packed, lens), ids)) for m in MODES}, args.reps, args.warmup)
        for m in MODES[1:]:
            row[m]["over_drop_ms"] = round(row[m]["ms_median"] - row["drop"]["ms_median"], 4)
        row["spread_drop_ms"] = round(row["drop"]["ms_max"] - row["drop"]["ms_min"], 4)
        return row
    fns = {}
    for m in MODES[1:]:
        pool = pools[m]
        for _ in range(args.warmup):                                    # the sessions reach their steady state
            pool.feed((packed, lens), ids)
        pd, p16, pu, ph = pool._plan_feed_at(lens, idv)                 # one plan again and again: the copy and the launches
        x16, y16, up_y = (0.1 * torch.randn(k, device="cuda") for k in (pd.n_out, pu.n_in, pu.n_out))
        fns[m] = (lambda hb=pool._hb, a=(ph, pu, packed, x16, y16, up_y, idv): hb.run(*a))
        fns[m + "_up_plane_alone"] = (lambda up=pool._hb.up_lo, pu=pu, y16=y16: up.run(pu, y16, idv))
    row = alternate(fns, args.reps, args.warmup)
    row.update(samples_in=S * n, outputs_per_call=pu.n_out, paired_per_call=ph.n_paired, blocks_per_call=ph.n_blocks,
               x_line_floats=pools["keep"]._hb.xcap)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=",".join(SECTIONS))
    ap.add_argument("--section", default=None, help="run this one section in this process (what the children are given)")
    ap.add_argument("--sessions", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=12, help="untimed calls per pool: the sessions reach their steady state")
    ap.add_argument("--cin", type=int, default=4)
    ap.add_argument("--tgru", action="store_true")
    ap.add_argument("--timeout", type=int, default=240, help="seconds a section's process may take")
    args = ap.parse_args()
    if args.section is not None:
        if args.section not in SECTIONS:
            ap.error("unknown section %r" % args.section)
        print(json.dumps(section(args.section, args)))
        return
    only = [s for s in args.only.split(",") if s]
    for s in only:
        if s not in SECTIONS:
            ap.error("unknown section %r" % s)
    res = {"metric": "stream_highband", "fs": FS, "sessions": args.sessions, "packet_ms": PACKET_MS, "reps": args.reps,
           "cin": args.cin, "tgru": args.tgru}
    for s in only:
        cmd = [sys.executable, os.path.abspath(__file__), "--section", s, "--sessions", str(args.sessions), "--reps",
               str(args.reps), "--warmup", str(args.warmup), "--cin", str(args.cin)] + (["--tgru"] if args.tgru else [])
        out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.timeout, check=True)      # a failure ends the run
        res[s] = json.loads(out.stdout.decode().strip().splitlines()[-1])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
