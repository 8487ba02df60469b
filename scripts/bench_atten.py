"""Cost of the attenuation limit (tinyrecurrentunet_amd/atten.py, csrc/atten.hip; the atten_lim_db keyword) on one MI355X;
prints one JSON line.  DESIGN section 3s quotes the figures.

Device events around a call, median and spread of --reps after a warm-up, as bench_stream_highband.py does it.  The
yardstick is the same call with atten_lim_db=None in the same run: that call is the code without the feature.

    pool16, pool48   --sessions sessions in steady state, one 20 ms packet each per call (320 samples at 16 kHz, 960 at 48
                     kHz): pool.feed without and with a limit, the two alternating in one process
    launches         what the limit adds on the device alone: trunet_stream_atten on such a call at 16 kHz, one plan
                     reused, without the host's planning
    enhance          enhance on --utterances x --seconds s at 16 kHz without and with a limit, alternating

Each section runs in a child process of its own under --timeout seconds; the first that fails ends the run.

    python scripts/bench_atten.py [--only pool16,pool48,launches,enhance] [--sessions 1024] [--reps 7] [--cin 4] [--tgru]
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

SECTIONS = ("pool16", "pool48", "launches", "enhance")
PACKET_MS, LIMIT_DB = 20, 12.0


def _over(row, a, b):
    row["over_none_ms"] = round(row[b]["ms_median"] - row[a]["ms_median"], 4)
    row["over_none_share"] = round(row["over_none_ms"] / row[a]["ms_median"], 4)
    row["spread_none_ms"] = round(row[a]["ms_max"] - row[a]["ms_min"], 4)
    return row


def section(name, args):
    import torch
    from bench_stream_resample import alternate
    from tinyrecurrentunet_amd.network import TRUNet
    if not torch.cuda.is_available():
        raise SystemExit("bench_atten.py measures GPU launches and needs the MI355X")
    torch.manual_seed(0)
    net = TRUNet(input_size=args.cin, use_tgru=args.tgru).cuda().eval()
    if name == "enhance":
        from tinyrecurrentunet_amd.enhance import enhance
        xs = [0.1 * torch.randn(int(16000 * args.seconds), device="cuda") for _ in range(args.utterances)]
        row = alternate({"none": lambda: enhance(net, xs), "limit": lambda: enhance(net, xs, atten_lim_db=LIMIT_DB)},
                        args.reps, 2)
        row.update(utterances=args.utterances, seconds=args.seconds)
        return _over(row, "none", "limit")
    fs = 48000 if name == "pool48" else 16000
    S, n = args.sessions, fs * PACKET_MS // 1000
    ids = list(range(S))
    lens = np.full(S, n, dtype=np.int64)
    packed = 0.1 * torch.randn(S * n, device="cuda")
    pools = {"none": net.stream_pool(S, fs=fs), "limit": net.stream_pool(S, fs=fs, atten_lim_db=LIMIT_DB)}
    for pool in pools.values():
        assert pool.open(S) == ids
    if name != "launches":
        row = alternate({k: (lambda pool=pool: pool.feed((packed, lens), ids)) for k, pool in pools.items()}, args.reps,
                        args.warmup)
        row.update(fs=fs, samples_per_call=S * n)
        return _over(row, "none", "limit")
    from tinyrecurrentunet_amd.atten import plan_atten
    from tinyrecurrentunet_amd.streaming import plan_feed
    pool = pools["limit"]
    for _ in range(args.warmup):                                        # the sessions reach their steady state
        pool.feed((packed, lens), ids)
    idv = np.arange(S, dtype=np.int64)
    plan = plan_feed(pool._hops, pool._pend, lens, idv)                 # one plan again and again: the launch alone
    off = np.cumsum(lens) - lens
    table, _ = plan_atten(idv, pool._dry_count(idv), off, lens, 128 * np.asarray(plan.out_off), plan.lengths,
                          np.zeros(S, dtype=bool), False)
    tab = torch.from_numpy(table).cuda()
    out = 0.1 * torch.randn(plan.n_out * 128, device="cuda")
    row = alternate({"stream_atten": lambda: pool._atten(tab, packed, S * n, out, plan.n_out * 128)}, args.reps, args.warmup)
    row.update(samples_in=S * n, outputs_per_call=plan.n_out * 128)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=",".join(SECTIONS))
    ap.add_argument("--section", default=None, help="run this one section in this process (what the children are given)")
    ap.add_argument("--sessions", type=int, default=1024)
    ap.add_argument("--utterances", type=int, default=150)
    ap.add_argument("--seconds", type=float, default=10.0)
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
    res = {"metric": "atten_lim", "limit_db": LIMIT_DB, "sessions": args.sessions, "packet_ms": PACKET_MS, "reps": args.reps,
           "cin": args.cin, "tgru": args.tgru}
    for s in only:
        cmd = [sys.executable, os.path.abspath(__file__), "--section", s, "--sessions", str(args.sessions), "--utterances",
               str(args.utterances), "--seconds", str(args.seconds), "--reps", str(args.reps), "--warmup", str(args.warmup),
               "--cin", str(args.cin)] + (["--tgru"] if args.tgru else [])
        out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.timeout, check=True)      # a failure ends the run
        res[s] = json.loads(out.stdout.decode().strip().splitlines()[-1])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
