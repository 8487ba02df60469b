"""Cost of StreamPool.feed (tinyrecurrentunet_amd/streaming.py) against the step-based glue a user of the pool writes without
it, on one MI355X; one JSON line per case and configuration.

Cases (16 kHz, C_in 4; every session is in steady state and gets one packet per call):
  a   1024 live sessions, 160-sample packets (10 ms RTP): one pool.feed() per call against the glue: a remainder per session
      on the device, and one pool.step() per whole hop the remainders hold (one or two per call, five per four calls)
  b   bursts: 64 sessions, one packet of 1 s each: one pool.feed() against 125 pool.step()s
  c   1024 sessions, 128-sample packets: pool.feed() against pool.step(), the price of the extra stages when there is
      nothing to batch
The glue is the cheapest one possible: all sessions get packets of the same size, so the remainders are one (sessions, r)
tensor and a step takes a column block of it; glue for packets of different sizes per session costs more.  Both sides run
on pools of the same class and weights, alternated window by window in one process; device events around each window of
--window calls, after a warm-up; median and spread of the per-call time over the windows, and the ratio feed / glue.
Configurations: stateless fp32, with the time-recurrent block, int8.

    python scripts/bench_pool_feed.py [--cases a,b,c] [--configs fp32,tgru,int8] [--windows 8] [--window 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tinyrecurrentunet_amd.network import TRUNet                      # noqa: E402
from tinyrecurrentunet_amd.streaming import HOP                        # noqa: E402

SR = 16000
CONFIGS = {"fp32": (False, {}), "tgru": (True, {}), "int8": (False, {"int8": True})}
CASES = {"a": (1024, 160, 20), "b": (64, SR, 2), "c": (1024, HOP, 20)}       # sessions, packet, default calls per window


def window_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def spread(v):
    v = np.asarray(v)
    return dict(median_ms=round(float(np.median(v)), 4), min_ms=round(float(v.min()), 4), max_ms=round(float(v.max()), 4),
                p10_ms=round(float(np.percentile(v, 10)), 4), p90_ms=round(float(np.percentile(v, 90)), 4))


class StepGlue:
    """what feed replaces: keep what does not fill a hop, cut whole hops out of it, one step per hop depth"""

    def __init__(self, pool, ids):
        self.pool, self.ids = pool, ids
        self.rem = torch.zeros((len(ids), 0), device="cuda")
        self.steps = 0

    def __call__(self, packets):                             # packets (sessions, P)
        buf = torch.cat([self.rem, packets], 1) if self.rem.shape[1] else packets
        k = buf.shape[1] // HOP
        outs = [self.pool.step(buf[:, HOP * d:HOP * (d + 1)], self.ids)[0] for d in range(k)]
        self.rem = buf[:, HOP * k:]
        self.steps += k
        return outs


def run_case(case, config, args):
    S, P, window = CASES[case]
    window = args.window or window
    use_tgru, kw = CONFIGS[config]
    torch.manual_seed(0)
    net = TRUNet(input_size=4, use_tgru=use_tgru).cuda().eval()
    packets = torch.randn((S, P), device="cuda") * 0.1
    flat, lens = packets.reshape(-1), np.full(S, P, dtype=np.int64)
    pool_f, pool_s = net.stream_pool(S, **kw), net.stream_pool(S, **kw)
    ids_f, ids_s = pool_f.open(S), pool_s.open(S)
    glue = StepGlue(pool_s, ids_s)
    feed = lambda: pool_f.feed((flat, lens), ids_f)
    warm = max(4, -(-8 * HOP // P))                          # both past their first frames, artefacts and scratch built
    for _ in range(warm):
        feed()
        glue(packets)
    assert pool_f.hops(ids_f[0]) == pool_s.hops(ids_s[0]) and pool_f.hops(ids_f[0]) >= 4
    torch.cuda.synchronize()
    tf, tg, s0 = [], [], glue.steps
    for _ in range(args.windows):
        tf.append(window_ms(feed, window))
        tg.append(window_ms(lambda: glue(packets), window))
    steps_per_call = (glue.steps - s0) / (args.windows * window)
    t0 = time.perf_counter()                                 # host time of a call that does not wait for the device
    for _ in range(window):
        feed()
    host_ms = (time.perf_counter() - t0) * 1e3 / window
    torch.cuda.synchronize()
    rec = dict(case=case, config=config, sessions=S, packet=P, timed_calls=args.windows * window, window=window,
               feed=spread(tf), step_glue=spread(tg), ratio=round(float(np.median(tf) / np.median(tg)), 4),
               glue_steps_per_call=round(steps_per_call, 3),
               feed_x_realtime=round(S * P / SR / (float(np.median(tf)) * 1e-3)),
               glue_x_realtime=round(S * P / SR / (float(np.median(tg)) * 1e-3)), feed_host_issue_ms=round(host_ms, 4))
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--configs", default="fp32,tgru,int8")
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--window", type=int, default=0, help="calls per window (default: 20, 2 for case b)")
    args = ap.parse_args()
    with torch.no_grad():
        for case in args.cases.split(","):
            for config in args.configs.split(","):
                run_case(case, config, args)


if __name__ == "__main__":
    main()
