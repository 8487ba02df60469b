"""Cost of carrying the band above 8 kHz around the network (tinyrecurrentunet_amd/highband.py, highband.hip) on one
MI355X; prints one JSON line.

Device-event times, median of --reps after a warm-up, min and max beside it (DESIGN section 3p quotes them):

    kernels   --utterances recordings of --seconds at --fs, packed: trunet_highband_gains and trunet_highband_join ("keep"
              and "follow") alone on preallocated buffers, and the 16 kHz -> fs resample launch of the same run, one plane
              and the two planes rejoin asks for; ms per launch and GB/s of what each reads and writes
    enhance   enhance(fs=--fs) with highband "drop", "keep" and "follow", alternating in one process

    python scripts/bench_highband.py [--only kernels,enhance] [--utterances 300] [--seconds 10] [--fs 48000] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SECTIONS = ("kernels", "enhance")


def timed_once(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternating(fns, reps):
    """{name: fn} -> {name: [ms] * reps}: one warm-up call each, then the functions take turns"""
    import torch
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(timed_once(fn))
    return ms


def stats(ms, nbytes=None):
    row = {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
    if nbytes is not None:
        row["gb_per_s"] = round(nbytes / (float(np.median(ms)) * 1e-3) / 1e9, 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=",".join(SECTIONS))
    ap.add_argument("--utterances", type=int, default=300)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--fs", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    only = [s for s in args.only.split(",") if s]
    for s in only:
        if s not in SECTIONS:
            ap.error("unknown section %r" % s)
    if args.reps < 1:
        ap.error("--reps must be at least 1")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_highband.py measures GPU launches and needs the MI355X")
    from tinyrecurrentunet_amd import _lib as L, highband as HB, resample as R
    from tinyrecurrentunet_amd._lib import check, ptr
    U, S, fs = args.utterances, args.seconds, args.fs
    pd, qd = R.ratio(fs, 16000)
    if pd >= qd:
        ap.error("--fs must lie above 16000")
    res = {"metric": "highband", "utterances": U, "seconds_each": S, "fs": fs, "reps": args.reps}

    if "kernels" in only:
        n = int(S * fs)
        n16 = R.out_length(n, pd, qd)
        T = HB.n_frames(n16)
        up = R.resampler(16000, fs, "cuda")
        _, plan = up.plan([n16] * U)
        offs = np.zeros((5, U + 1), dtype=np.int64)
        offs[:3] = plan
        offs[3] = np.arange(U + 1) * n
        offs[4] = np.arange(U + 1) * T
        nS, nU, nF, nT = (int(offs[i, -1]) for i in (0, 1, 3, 4))
        offs_d = torch.from_numpy(offs).cuda()
        lo = torch.randn(nS, device="cuda")
        y16 = lo * torch.rand(nS, device="cuda")
        x = torch.randn(nF, device="cuda")
        sig2 = torch.stack([y16, lo])
        ups = up.packed(sig2, plan, 2, offs_d)
        g = torch.empty(nT, device="cuda")
        energy = torch.empty((nT, 2), device="cuda")
        out = torch.empty(nF, device="cuda")
        lib, st, taps = L.lib(), L.stream(), HB._taps(lo.device)

        def gains():
            check(lib.trunet_highband_gains(ptr(lo), ptr(y16), offs_d[0].data_ptr(), offs_d[4].data_ptr(), ptr(taps),
                                            ptr(energy), ptr(g), U, nS, nT, HB.floor_gain(-30.0), st), "highband_gains")

        def join(mode):
            return lambda: check(lib.trunet_highband_join(ptr(ups[0]), ptr(ups[1]), ptr(x), ptr(g), ptr(out),
                                                          offs_d[3].data_ptr(), offs_d[1].data_ptr(), offs_d[4].data_ptr(), U,
                                                          nF, nU, nT, pd, qd, mode, st), "highband_join")
        ms = alternating({"gains": gains, "join_keep": join(HB.KEEP), "join_follow": join(HB.FOLLOW),
                          "resample_up_1_plane": lambda: up.packed(sig2[:1], plan, 1, offs_d),
                          "resample_up_2_planes": lambda: up.packed(sig2, plan, 2, offs_d)}, args.reps)
        res["kernels"] = {
            "samples_at_fs": nF, "samples_at_16k": nS, "frames": nT,
            "gains": stats(ms["gains"], 4 * (2 * nS + 3 * nT)),
            "join_keep": stats(ms["join_keep"], 16 * nF),
            "join_follow": stats(ms["join_follow"], 16 * nF + 4 * nT),
            "resample_up_1_plane": stats(ms["resample_up_1_plane"], 4 * (nS + nU)),
            "resample_up_2_planes": stats(ms["resample_up_2_planes"], 8 * (nS + nU))}
        del lo, y16, x, sig2, ups, out

    if "enhance" in only:
        from tinyrecurrentunet_amd.enhance import enhance
        from tinyrecurrentunet_amd.network import TRUNet
        torch.manual_seed(0)
        net = TRUNet(input_size=4).cuda().eval()
        xs = [0.1 * torch.randn(int(S * fs), device="cuda") for _ in range(U)]
        ms = alternating({m: (lambda m=m: enhance(net, xs, fs=fs, highband=m)) for m in HB.MODES}, args.reps)
        res["enhance"] = {m: stats(ms[m]) for m in HB.MODES}
        base = res["enhance"]["drop"]["ms_median"]
        for m in ("keep", "follow"):
            res["enhance"][m]["added_ms"] = round(res["enhance"][m]["ms_median"] - base, 4)
            res["enhance"][m]["added_share"] = round(res["enhance"][m]["ms_median"] / base - 1.0, 4)
        res["enhance"]["drop_spread_ms"] = round(res["enhance"]["drop"]["ms_max"] - res["enhance"]["drop"]["ms_min"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
