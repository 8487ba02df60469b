"""Cost of the stream pool (tinyrecurrentunet_amd/streaming.py: StreamPool) on one MI355X; one JSON line per case.

Cases (16 kHz, hops of 128 samples, 1024 slots, C_in 4):
  a   all slots live in steady state: one pool.step() of 1024 rows against one AudioStream(net, 1024).push() on the same
      weights, alternated window by window in the same process; per configuration (stateless fp32, with the time-recurrent
      block, int8) the median and the spread of the per-step time over the windows, and the ratio pool / lockstep
  b   churn: sessions of 2-30 s that start at random and end at arbitrary sample counts, for at least --seconds of
      simulated audio per slot: steps/s, x real time (live audio seconds per wall second), the share of steps that needed a
      second pass and the share of the time spent in close()
Device events around each timed window, after a warm-up; the windows of case a hold --window steps each.

    python scripts/bench_pool.py [--cases a,b] [--slots 1024] [--windows 12] [--window 20] [--seconds 20]
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
from tinyrecurrentunet_amd.streaming import AudioStream, HOP           # noqa: E402

SR = 16000


def window_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def spread(v):
    v = np.asarray(v)
    return dict(median_ms=round(float(np.median(v)), 4), min_ms=round(float(v.min()), 4), max_ms=round(float(v.max()), 4),
                p10_ms=round(float(np.percentile(v, 10)), 4), p90_ms=round(float(np.percentile(v, 90)), 4))


def case_a(args):
    S = args.slots
    for name, use_tgru, kw in (("fp32", False, {}), ("tgru", True, {}), ("int8", False, {"int8": True})):
        torch.manual_seed(0)
        net = TRUNet(input_size=4, use_tgru=use_tgru).cuda().eval()
        chunk = torch.randn((S, HOP), device="cuda") * 0.1
        pool = net.stream_pool(S, **kw)
        ids = pool.open(S)
        lock = AudioStream(net, S, tgru=use_tgru, **kw)
        for _ in range(8):                                   # both past their first frames, artefacts and scratch built
            pool.step(chunk, ids)
            lock.push(chunk)
        torch.cuda.synchronize()
        tp, tl = [], []
        for _ in range(args.windows):
            tp.append(window_ms(lambda: pool.step(chunk, ids), args.window))
            tl.append(window_ms(lambda: lock.push(chunk), args.window))
        t0 = time.perf_counter()                             # host time of a step that does not wait for the device
        for _ in range(args.window):
            pool.step(chunk, ids)
        host_ms = (time.perf_counter() - t0) * 1e3 / args.window
        torch.cuda.synchronize()
        rec = dict(case="a", config=name, slots=S, timed_steps=args.windows * args.window, window=args.window,
                   pool=spread(tp), lockstep=spread(tl), ratio=round(float(np.median(tp) / np.median(tl)), 4),
                   pool_x_realtime=round(S * HOP / SR / (float(np.median(tp)) * 1e-3)),
                   lockstep_x_realtime=round(S * HOP / SR / (float(np.median(tl)) * 1e-3)),
                   pool_host_issue_ms=round(host_ms, 4))
        print(json.dumps(rec), flush=True)


def case_b(args):
    S = args.slots
    torch.manual_seed(0)
    g = np.random.default_rng(0)
    net = TRUNet(input_size=4).cuda().eval()
    pool = net.stream_pool(S)
    steps = int(args.seconds * SR / HOP)
    noise = torch.randn(SR * 4, device="cuda") * 0.1        # every session reads from this, from its own moving offset
    off = torch.arange(HOP, device="cuda")
    slot_of = np.full(S, -1)                                # lane -> slot, -1: the lane waits
    left = np.zeros(S, dtype=np.int64)                      # samples the lane's session still has to send
    wait = g.integers(0, 250, S)                            # steps until the lane's next session starts
    start = g.integers(0, SR * 2, S)
    sent = np.zeros(S, dtype=np.int64)                      # hops the lane's session has sent

    def run(n_steps, timed):
        second = closes = sessions = samples = 0
        close_ev = []
        for _ in range(n_steps):
            for lane in np.nonzero((slot_of < 0) & (wait <= 0))[0]:
                (slot_of[lane],) = pool.open(1)
                left[lane] = int(g.uniform(2, 30) * SR) + int(g.integers(0, HOP))
                sent[lane] = 0
            wait[:] -= 1
            live = np.nonzero((slot_of >= 0) & (left >= HOP))[0]
            if len(live):
                second += int((sent[live] == 2).any())          # a session at its third hop: frames 0 and 1
                idx = torch.from_numpy((start[live] + left[live] % (SR * 2 - HOP))[:, None]).cuda() + off[None, :]
                pool.step(noise[idx], slot_of[live])
                left[live] -= HOP
                sent[live] += 1
                samples += HOP * len(live)
            done = np.nonzero((slot_of >= 0) & (left < HOP))[0]
            if len(done):
                tails = [noise[:int(r)] if r else None for r in left[done]]
                if timed:
                    close_ev.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
                    close_ev[-1][0].record()
                pool.close(slot_of[done], tails)
                if timed:
                    close_ev[-1][1].record()
                samples += int(left[done].sum())
                closes += 1
                sessions += len(done)
                slot_of[done] = -1
                wait[done] = g.integers(0, 250, len(done))
        return second, closes, sessions, close_ev, samples

    run(300, False)                                         # warm-up: sessions in every phase of their life
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    second, closes, sessions, close_ev, samples = run(steps, True)
    b.record()
    b.synchronize()
    close_ms = sum(e0.elapsed_time(e1) for e0, e1 in close_ev)
    ms, wall = a.elapsed_time(b), time.perf_counter() - t0
    rec = dict(case="b", slots=S, steps=steps, simulated_s_per_slot=round(steps * HOP / SR, 2), total_ms=round(ms, 1),
               wall_s=round(wall, 3), steps_per_s=round(steps / ms * 1e3, 1), audio_s=round(samples / SR, 1),
               x_realtime=round(samples / SR / (ms * 1e-3)), second_pass_share=round(second / steps, 4),
               sessions_closed=sessions, close_calls=closes, close_time_share=round(close_ms / ms, 4))
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a,b")
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--windows", type=int, default=12)
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=20.0)
    args = ap.parse_args()
    with torch.no_grad():
        for case in args.cases.split(","):
            {"a": case_a, "b": case_b}[case](args)


if __name__ == "__main__":
    main()
