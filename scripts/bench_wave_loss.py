"""Time of the time-domain loss terms on one MI355X; prints one JSON line per measurement.

At 64 x 64000 (the benchmarked batch), forward plus backward of the cosine term and the SI-SDR term together:
  kernels      the three launches of csrc/wave_loss.hip through the entry points, buffers reused (what the fused loss tail adds)
  node         the same through cos_loss.wave_loss and autograd (allocations and the node's bookkeeping included)
  composition  the same terms composed from torch ops on the same device, with autograd
for the reference's g (four segments in the first 4062 samples) and for 504-sample segments tiling the row; then
util.loss_fn forward plus backward with and without the terms.  Device events around --reps calls after --warmup calls:
median and p10 / p90.

    python scripts/bench_wave_loss.py [--reps 50] [--warmup 10] [--no-loss-fn]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, LEN = 64, 64000


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
    ap.add_argument("--no-loss-fn", action="store_true", help="skip the whole-step measurement")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_wave_loss.py measures GPU kernels and needs the MI355X")
    from tinyrecurrentunet_amd import cos_loss as cl
    rng = np.random.default_rng(0)
    y = torch.tensor(0.1 * rng.standard_normal((B, LEN)) + 0.01, dtype=torch.float32).cuda()
    x = (y + 0.05 * torch.tensor(rng.standard_normal((B, LEN)), dtype=torch.float32).cuda()).contiguous()
    one = torch.ones(1, device="cuda")
    cos_lambda, si_lambda, cos_eps, si_eps = 0.5, 0.01, 1e-5, 1e-8

    for name, g in (("reference g", list(cl.DEFAULT_G)), ("uniform 504", cl.CosSimLoss.uniform(504, LEN).g)):
        plan = cl.wave_plan(LEN, g, True, x.device)
        grad = torch.zeros_like(x)

        def kernels():
            _, _, coef = cl.wave_forward(x, y, plan, cos_lambda, cos_eps, si_lambda, si_eps)
            cl.wave_backward(x, y, plan, coef, one, grad)

        def node():
            xg = x.detach().requires_grad_(True)
            loss, _, _ = cl.wave_loss(xg, y, g=g, cos_lambda=cos_lambda, cos_eps=cos_eps, si_sdr_lambda=si_lambda,
                                      si_sdr_eps=si_eps)
            loss.backward()
            return loss, xg.grad

        def composition():
            xg = x.detach().requires_grad_(True)
            loss = cos_lambda * cl.cos_sim_loss_torch(xg, y, g, cos_eps) + si_lambda * cl.si_sdr_loss_torch(xg, y, si_eps)
            loss.backward()
            return loss, xg.grad

        (ln, gn), (lc, gc) = node(), composition()
        res = {"metric": "wave_loss_fwd_bwd_ms", "B": B, "L": LEN, "g": name, "segments": len(g), "work_items": plan.n_items,
               "warmup": args.warmup, "reps": args.reps,
               "kernels_ms": timed(kernels, args.warmup, args.reps), "node_ms": timed(node, args.warmup, args.reps),
               "composition_ms": timed(composition, args.warmup, args.reps),
               "loss_rel_diff_vs_composition": float(abs(ln - lc) / abs(lc)),
               "grad_max_diff_vs_composition": float((gn - gc).abs().max() / gc.abs().max())}
        res["composition_over_kernels"] = round(res["composition_ms"]["median"] / res["kernels_ms"]["median"], 1)
        print(json.dumps(res), flush=True)

    if args.no_loss_fn:
        return
    from tinyrecurrentunet_amd import network as hn, stft_loss as sl, util
    torch.manual_seed(0)
    net = hn.TRUNet(input_size=4).cuda().train()
    mr = sl.MultiResolutionSTFTLoss().cuda()
    X = (y.unsqueeze(1), x.unsqueeze(1))
    extra = dict(cos_lambda=cos_lambda, cos_config={"g": cl.CosSimLoss.uniform(504, LEN).g}, si_sdr_lambda=si_lambda)

    def step(**kw):
        net.zero_grad(set_to_none=True)
        loss, _ = util.loss_fn(net, X, ell_p=1, ell_p_lambda=1, stft_lambda=1, mrstftloss=mr, **kw)
        loss.backward()

    reps = max(args.reps // 5, 5)
    res = {"metric": "loss_fn_fwd_bwd_ms", "B": B, "L": LEN, "reps": reps,
           "without_terms_ms": timed(step, 3, reps), "with_terms_ms": timed(lambda: step(**extra), 3, reps)}
    res["added_ms"] = round(res["with_terms_ms"]["median"] - res["without_terms_ms"]["median"], 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
