"""Time of the intelligibility loss on one MI355X; prints one JSON line per measurement.

At 64 x 64000 (the benchmarked batch, 16 kHz), forward plus backward of the term alone:
  kernels      stoi_loss.forward_packed + loss_value + backward_packed: the launches the fused loss tail adds
  node         the same through STOILoss and autograd (packing and the node's bookkeeping included)
  composition  the torch restatement of the same chain (tests/stoi_loss_ref.py's operations, batched) on the same device
               with autograd, float32 up to the bands and float64 segments; its silence mask comes from the kernels
then the train step of bench.py's default configuration with and without stoi_lambda, alternating in one process.  Device
events around --reps calls after --warmup calls: median and p10 / p90.

    python scripts/bench_stoi_loss.py [--reps 30] [--warmup 5] [--extended] [--no-step] [--no-composition]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, LEN, FS = 64, 64000, 16000


def stats(ms):
    return {"median": round(float(np.median(ms)), 4), "p10": round(float(np.percentile(ms, 10)), 4),
            "p90": round(float(np.percentile(ms, 90)), 4)}


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
    return stats(ms)


def composition_loss(est, clean, kept, extended):
    """the chain in batched torch ops for equal-length rows that all keep the same number of frames (the benchmark's
    synthetic batch keeps every frame): est, clean (B, L) fp32, kept (B, K) int64 -> -mean score"""
    import torch
    from tinyrecurrentunet_amd import evaluate as ev
    dev = est.device
    p, q = ev.ratio(FS)
    h, half = ev.kaiser_filter(p, q)
    h = torch.tensor(h, dtype=torch.float32, device=dev)
    win = torch.tensor(ev.window(), dtype=torch.float32, device=dev)
    edges = [int(e) for e in ev.band_edges()]
    eps = float(np.finfo(np.float64).eps)

    def resample(x):                                         # upsample by p, filter, keep every q-th sample
        n_out = -(-x.shape[1] * p // q)
        up = torch.zeros((x.shape[0], 1, x.shape[1] * p), dtype=x.dtype, device=dev)
        up[:, 0, ::p] = x
        y = torch.nn.functional.conv1d(up, (p * h).flip(0)[None, None], padding=half)
        return y[:, 0, ::q][:, :n_out]

    def tob(x10):
        fr = win * x10.unfold(1, ev.N_FRAME, ev.HOP)[:, :ev.n_frames(x10.shape[1])]
        fr = torch.gather(fr, 1, kept[:, :, None].expand(-1, -1, ev.N_FRAME))
        K = fr.shape[1]
        sil = torch.zeros((fr.shape[0], K + 1, ev.HOP), dtype=fr.dtype, device=dev)
        sil[:, :K] += fr[:, :, :ev.HOP]
        sil[:, 1:] += fr[:, :, ev.HOP:]
        sil = sil.reshape(fr.shape[0], -1)
        st = win * sil.unfold(1, ev.N_FRAME, ev.HOP)[:, :K - 1]
        spec = torch.fft.rfft(st, ev.NFFT, dim=2)
        pw = spec.real ** 2 + spec.imag ** 2
        a = torch.stack([pw[:, :, edges[k]:edges[k + 1]].sum(dim=2) for k in range(ev.NUMBAND)], dim=2)
        return torch.sqrt(a.clamp_min(1e-30)).double()

    X = tob(resample(clean)).unfold(1, ev.SEG, 1)            # (B, nseg, 15, 30)
    Y = tob(resample(est)).unfold(1, ev.SEG, 1)
    if extended:
        def rc(a):
            a = a - a.mean(dim=3, keepdim=True)
            a = a / (a.norm(dim=3, keepdim=True) + eps)
            a = a - a.mean(dim=2, keepdim=True)
            return a / (a.norm(dim=2, keepdim=True) + eps)
        s = (rc(X) * rc(Y)).sum(dim=(2, 3)).mean(dim=1) / ev.SEG
    else:
        u = Y * X.norm(dim=3, keepdim=True) / (Y.norm(dim=3, keepdim=True) + eps)
        yp = torch.minimum(u, X * (1 + 10 ** (15 / 20)))
        dx, dy = X - X.mean(dim=3, keepdim=True), yp - yp.mean(dim=3, keepdim=True)
        d = (dx * dy).sum(dim=3) / ((dx.norm(dim=3) + eps) * (dy.norm(dim=3) + eps))
        s = d.mean(dim=(1, 2))
    return -s.mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--extended", action="store_true", help="ESTOI instead of STOI")
    ap.add_argument("--no-step", action="store_true", help="skip the train-step measurement")
    ap.add_argument("--no-composition", action="store_true", help="skip the torch composition")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_stoi_loss.py measures GPU kernels and needs the MI355X")
    import bench
    from tinyrecurrentunet_amd import evaluate as ev, stoi_loss as stl
    dev = torch.device("cuda")
    clean, noisy = bench.synth(B, LEN, 1234, dev)
    x, y = clean[:, 0].contiguous(), noisy[:, 0].contiguous()
    one = torch.ones(1, device=dev)
    p, q = ev.ratio(FS)
    lens = [LEN] * B

    def kernels():
        r = stl.forward_packed(y.reshape(-1), x.reshape(-1), lens, p, q, args.extended)
        stl.loss_value(r)
        return r, stl.backward_packed(r, one)

    f = stl.STOILoss(extended=args.extended, fs=FS)

    def node():
        yg = y.detach().requires_grad_(True)
        loss = f(yg, x)
        loss.backward()
        return loss, yg.grad

    res = {"metric": "stoi_loss_fwd_bwd_ms", "B": B, "L": LEN, "extended": args.extended, "warmup": args.warmup,
           "reps": args.reps}
    r, _ = kernels()
    nF = r.tot[3]
    ln, gn = node()
    res["segments_per_utterance"] = int(r.segments[0])
    res["mean_score"] = float(-ln)
    res["kernels_ms"] = timed(kernels, args.warmup, args.reps)
    res["forward_only_ms"] = timed(lambda: stl.loss_value(stl.forward_packed(y.reshape(-1), x.reshape(-1), lens, p, q,
                                                                             args.extended)), args.warmup, args.reps)
    res["node_ms"] = timed(node, args.warmup, args.reps)
    K = int(r.segments[0]) + ev.SEG
    if not args.no_composition and bool((r.segments == r.segments[0]).all()) and K == nF // B:
        kept = torch.arange(K, device=dev)[None].expand(B, -1).contiguous()

        def composition():
            yg = y.detach().requires_grad_(True)
            loss = composition_loss(yg, x, kept, args.extended)
            loss.backward()
            return loss, yg.grad
        lc, gc = composition()
        res["composition_ms"] = timed(composition, args.warmup, args.reps)
        res["loss_diff_vs_composition"] = float(abs(ln - lc))
        res["grad_max_diff_vs_composition"] = float((gn - gc).abs().max() / gc.abs().max())
        res["composition_over_kernels"] = round(res["composition_ms"]["median"] / res["kernels_ms"]["median"], 1)
    print(json.dumps(res), flush=True)

    if args.no_step:
        return
    from tinyrecurrentunet_amd import network as hn, optim, stft_loss as sl, util
    torch.manual_seed(0)
    net = hn.TRUNet(input_size=4).to(dev).train()
    opt = optim.FusedAdamW(net.parameters(), lr=4e-4)
    mr = sl.MultiResolutionSTFTLoss(**bench.STFT_CFG).to(dev)

    def step(**kw):
        opt.zero_grad()
        loss, _ = util.loss_fn(net, (clean, noisy), ell_p=1, ell_p_lambda=1, stft_lambda=1, mrstftloss=mr, **kw)
        loss.backward()
        opt.step()

    extra = dict(stoi_lambda=0.5, stoi_config={"extended": args.extended})
    for _ in range(3):
        step()
        step(**extra)
    torch.cuda.synchronize()
    reps = max(args.reps // 2, 8)
    ms = {"without": [], "with": []}
    for _ in range(reps):                                    # alternating, so that drift of the clocks hits both alike
        for key, kw in (("without", {}), ("with", extra)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step(**kw)
            b.record()
            b.synchronize()
            ms[key].append(a.elapsed_time(b))
    out = {"metric": "train_step_ms", "B": B, "L": LEN, "extended": args.extended, "reps": reps,
           "without_term_ms": stats(ms["without"]), "with_term_ms": stats(ms["with"])}
    out["added_ms"] = round(out["with_term_ms"]["median"] - out["without_term_ms"]["median"], 4)
    out["added_share_of_step"] = round(out["added_ms"] / out["without_term_ms"]["median"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
