"""GPU: the intelligibility loss (tinyrecurrentunet_amd/stoi_loss.py).  Its gradient against autograd
through the float64 restatement (tests/stoi_loss_ref.py) under the project's rule gru_ref.close, with e32 / rel32 from the
float32 restatement on the same inputs; the forward against evaluate() bit for bit; independence of batch-mates, order,
padding and run; the degenerate inputs; the term inside util.loss_fn, fused and composed; a few optimiser steps."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gru_ref as GR            # noqa: E402
import stoi_loss_cases as SC    # noqa: E402

pytestmark = pytest.mark.gpu

TOL_STOI = 1e-5                 # test_evaluate_gpu.py's absolute bar for STOI / ESTOI


def _loss():
    from tinyrecurrentunet_amd import stoi_loss
    return stoi_loss


def run(names, extended, fs, padded=False, nan_pad=True, up=1.0):
    """the loss of the named pairs as one batch, times ``up`` -> (loss, [gradient per utterance (cpu)], scores, segments)"""
    f = _loss().STOILoss(extended=extended, fs=fs)
    pairs = [SC.pair(n) for n in names]
    if padded:
        lens = [p[0].shape[0] for p in pairs]
        est = torch.full((len(pairs), max(lens) + 37), float("nan") if nan_pad else 0.0)
        cl = est.clone()
        for b, (y, x) in enumerate(pairs):
            est[b, :lens[b]], cl[b, :lens[b]] = y, x
        est = est.cuda().requires_grad_(True)
        loss = f(est, cl.cuda(), lengths=lens)
        (loss * up).backward()
        g = est.grad.cpu()
        assert bool((g[torch.arange(g.shape[1])[None, :] >= torch.tensor(lens)[:, None]] == 0).all()), "gradient in the padding"
        grads = [g[b, :n] for b, n in enumerate(lens)]
    else:
        ys = [p[0].cuda().requires_grad_(True) for p in pairs]
        loss = f(ys, [p[1].cuda() for p in pairs])
        (loss * up).backward()
        grads = [y.grad.cpu() for y in ys]
    scores, segments = f.scores
    return loss.detach().cpu(), grads, scores.cpu(), segments.cpu()


@pytest.mark.parametrize("extended", [False, True], ids=["stoi", "estoi"])
@pytest.mark.parametrize("name", SC.GRAD_CASES)
def test_gradient_matches_float64_autograd(name, extended):
    fs, _, _, _, _, K, segs = SC.CASES[name]
    r = SC.ref(name, extended)
    loss, (g,), scores, segments = run([name], extended, fs)
    tag = "stoi_loss %s %s K=%d" % (name, "estoi" if extended else "stoi", K)
    assert int(segments[0]) == segs == r["r64"]["segments"]
    if segs == 0:
        SC.report("%s: no segment, score %.3g, max|g| %.3g" % (tag, float(scores[0]), float(g.abs().max())))
        assert float(scores[0]) == 1e-5 and bool((g == 0).all())
        return
    d = g.double() - r["g64"]
    d32 = r["g32"].double() - r["g64"]
    nrm = float(r["g64"].norm())
    err, e32, rel, rel32 = float(d.abs().max()), float(d32.abs().max()), float(d.norm()) / nrm, float(d32.norm()) / nrm
    SC.report("%s: gradient max error %.3e (e32 %.3e, bound %.3e, max|ref| %.3e), relative L2 %.3e (rel32 %.3e, bound %.3e); "
              "score error %.2e" % (tag, err, e32, 4 * e32 + 2e-6 * float(r["g64"].abs().max()),
                                    float(r["g64"].abs().max()), rel, rel32, 4 * rel32 + 1e-6,
                                    abs(float(scores[0]) - float(r["r64"]["score"].detach()))))
    assert abs(float(scores[0]) - float(r["r64"]["score"].detach())) <= TOL_STOI
    GR.close(g, r["g64"], r["g32"], tag)


@pytest.mark.parametrize("fs, names", [(16000, ("k31_16k", "k30_16k", "mid_16k")), (10000, ("k32_10k", "k30_10k")),
                                       (48000, ("lead_48k",)), (8000, ("k32_8k",))])
def test_forward_is_evaluate_bit_for_bit(fs, names):
    from tinyrecurrentunet_amd.evaluate import evaluate
    ev = evaluate([SC.pair(n)[1].cuda() for n in names], [SC.pair(n)[0].cuda() for n in names], fs=fs)
    for extended, key in ((False, "stoi"), (True, "estoi")):
        loss, _, scores, segments = run(names, extended, fs)
        assert torch.equal(scores, ev[key].cpu()) and torch.equal(segments, ev["segments"].cpu())
        want = np.float32(-np.mean(scores.numpy()))
        assert loss.dtype == torch.float32 and float(loss) == float(want), (float(loss), float(want))


@pytest.mark.parametrize("extended", [False, True], ids=["stoi", "estoi"])
def test_gradient_is_independent_of_batch_mates_order_padding_and_run(extended):
    names = ("k31_16k", "k30_16k", "mid_16k", "k30_16k")
    _, grads, scores, _ = run(names, extended, 16000)
    assert bool((grads[1] == 0).all()) and float(scores[1]) == 1e-5
    # each pair alone: the batch mean divides by B = 4, so the lone pair's loss carries the cotangent 1 / 4 and both runs
    # multiply by the same -1 / 4 (the factor enters the kernels as the product of the cotangent and -1 / B)
    for i, n in enumerate(names[:3]):
        _, alone, s1, _ = run((n,), extended, 16000, up=0.25)
        assert torch.equal(alone[0], grads[i]), n
        assert torch.equal(s1[0], scores[i])
    _, rev, srev, _ = run(names[::-1], extended, 16000)
    for i in range(4):
        assert torch.equal(rev[3 - i], grads[i]) and torch.equal(srev[3 - i], scores[i])
    _, again, _, _ = run(names, extended, 16000)
    _, pad, spad, _ = run(names, extended, 16000, padded=True)
    for i in range(4):
        assert torch.equal(again[i], grads[i]) and torch.equal(pad[i], grads[i])
    assert torch.equal(spad, scores)


@pytest.mark.parametrize("extended", [False, True], ids=["stoi", "estoi"])
def test_degenerate_inputs(extended):
    f = _loss().STOILoss(extended=extended, fs=16000)
    x = SC.pair("mid_16k")[1].cuda()
    # an all-zero estimate: finite, exactly zero gradient
    y = torch.zeros_like(x).requires_grad_(True)
    loss = f([y], [x])
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool((y.grad == 0).all())
    assert int(f.scores[1][0]) == SC.CASES["mid_16k"][6]
    # the estimate equal to the clean signal: score 1, everything finite
    y = x.clone().requires_grad_(True)
    loss = f([y], [x])
    loss.backward()
    assert bool(torch.isfinite(y.grad).all()) and abs(float(f.scores[0][0]) - 1.0) <= TOL_STOI
    assert abs(float(loss) + 1.0) <= TOL_STOI
    # an all-zero clean signal: every frame energy equals the threshold's maximum, so evaluate keeps them all and every
    # correlation is 0 / eps: the score is evaluate's (and the restatement's) 0, not the 1e-5 of "no segment", and the
    # gradient is exactly zero
    from tinyrecurrentunet_amd.evaluate import evaluate
    y = SC.pair("mid_16k")[0].cuda().requires_grad_(True)
    loss = f([y], [torch.zeros_like(x)])
    loss.backward()
    want = evaluate([torch.zeros_like(x)], [y.detach()], fs=16000)["estoi" if extended else "stoi"]
    assert torch.equal(f.scores[0], want) and float(want[0]) == 0.0 and bool((y.grad == 0).all())


class _FixedNet(torch.nn.Module):
    """stands where the network stands in util.loss_fn and returns its one parameter: the loss tail then starts from a
    tensor the CPU reference knows"""

    def __init__(self, out):
        super().__init__()
        self.out = torch.nn.Parameter(out.clone())

    def forward(self, feats):
        return self.out


def _tail(extended, fused, monkeypatch, **kw):
    from tinyrecurrentunet_amd import util
    monkeypatch.setattr(util, "FUSED_LOSS", fused)
    net_out, clean = SC.tail_inputs()
    net = _FixedNet(net_out).cuda()
    X = (clean[:, None].cuda(), clean[:, None].cuda())
    loss, info = util.loss_fn(net, X, 1, 1, 0, None, pcen=False, stoi_config={"extended": extended}, **kw)
    return net, loss, info


@pytest.mark.parametrize("extended", [False, True], ids=["stoi", "estoi"])
def test_loss_tail_fused_and_composed_match_the_restated_tail(extended, monkeypatch):
    r64, r32 = SC.tail_ref(extended, torch.float64), SC.tail_ref(extended, torch.float32)
    got = {}
    for fused in (True, False):
        net, loss, info = _tail(extended, fused, monkeypatch, stoi_lambda=SC.TAIL_LAMBDA)
        loss.backward(retain_graph=not fused)
        g = net.out.grad.clone()
        tag = "stoi_loss tail %s %s" % ("estoi" if extended else "stoi", "fused" if fused else "composed")
        assert set(info) == {"l1", "stoi"} and not info["stoi"].requires_grad
        e_loss = abs(float(loss) - float(r64["loss"]))
        e_term = abs(float(info["stoi"]) - SC.TAIL_LAMBDA * float(r64["stoi"]))
        d, d32 = g.cpu().double() - r64["g_net"], r32["g_net"].double() - r64["g_net"]
        SC.report("%s: loss error %.2e, term error %.2e, gradient max error %.3e (e32 %.3e), relative L2 %.3e (rel32 %.3e)"
                  % (tag, e_loss, e_term, float(d.abs().max()), float(d32.abs().max()),
                     float(d.norm() / r64["g_net"].norm()), float(d32.norm() / r64["g_net"].norm())))
        # the loss is one fp32 number.  On top of the fp32 restatement's own error (which sums in float64) come the fp32
        # roundings of the kernels' sums, U = 2^-24 each relative to the magnitude of the terms: the L1 block sums of 256
        # samples (a random walk of 16 U), the column sum, the division, the term, its weight and the addition: 2^-19
        mag = abs(float(r64["loss"])) + SC.TAIL_LAMBDA * abs(float(r64["stoi"]))
        assert e_loss <= 4 * abs(float(r32["loss"]) - float(r64["loss"])) + 2.0 ** -19 * mag
        assert e_term <= SC.TAIL_LAMBDA * TOL_STOI
        GR.close(g, r64["g_net"], r32["g_net"], tag)
        if not fused:
            # a second backward on the retained graph gives the same gradient
            net.out.grad = None
            loss.backward()
            assert torch.equal(net.out.grad, g)
        got[fused] = (loss.detach(), g)


def test_loss_tail_without_the_term_is_unchanged_bit_for_bit(monkeypatch):
    from tinyrecurrentunet_amd import util
    for fused in (True, False):
        monkeypatch.setattr(util, "FUSED_LOSS", fused)
        net_out, clean = SC.tail_inputs()
        X = (clean[:, None].cuda(), clean[:, None].cuda())
        res = []
        for kw in ({}, dict(stoi_lambda=0), dict(stoi_lambda=0.0, stoi_config={"extended": True})):
            net = _FixedNet(net_out).cuda()
            loss, info = util.loss_fn(net, X, 1, 1, 0, None, pcen=False, **kw)
            loss.backward()
            res.append((loss.detach(), info, net.out.grad))
        for loss, info, g in res[1:]:
            assert set(info) == set(res[0][1]) == {"l1"}
            assert torch.equal(loss, res[0][0]) and torch.equal(g, res[0][2]) and torch.equal(info["l1"], res[0][1]["l1"])


def _l2rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def test_loss_fn_with_si_sdr_and_the_frames_last_boundary(monkeypatch):
    """the term next to the STFT loss and SI-SDR on the real network: the fused tail (with the frames-last boundary, and
    without it) against the composition, at the bars of the fused-versus-composition tests of the rest of the loss
    (test_wave_loss_gpu.py: 2e-6 relative loss, 2e-5 relative L2 gradient)"""
    from oracle import network_ref as nr, weights as W
    from tinyrecurrentunet_amd import network as hn, stft_loss as sl, util
    B, length = 2, 8192
    clean, noisy = W.synth_pairs(B, length, seed=9)
    net = hn.TRUNet(input_size=4)
    net.load_state_dict(W.fill_state_dict(nr.TRUNet(input_size=4), seed=1).state_dict())
    net.cuda().train()
    cfg = dict(fft_sizes=[512, 1024, 2048], hop_sizes=[50, 120, 240], win_lengths=[240, 600, 1200], sc_lambda=0.5,
               mag_lambda=0.5, band="full")
    mr = sl.MultiResolutionSTFTLoss(**cfg).cuda()
    X = (clean.cuda(), noisy.cuda())

    def step(**kw):
        net.zero_grad(set_to_none=True)
        loss, info = util.loss_fn(net, X, ell_p=1, ell_p_lambda=1, stft_lambda=1, mrstftloss=mr, **kw)
        loss.backward()
        return loss.detach(), info, net.decoder[5].LastTrCNN[3].weight.grad.clone()
    extra = dict(stoi_lambda=0.5, stoi_config={"extended": True}, si_sdr_lambda=0.01)
    got = {}
    for key, fused, flb in (("fl", True, "1"), ("fused", True, "0"), ("composed", False, "0")):
        monkeypatch.setattr(util, "FUSED_LOSS", fused)
        monkeypatch.setenv("TRUNET_FL_BOUNDARY", flb)
        got[key] = step(**extra)
        assert set(got[key][1]) == {"l1", "stft_sc", "stft_mag", "si_sdr", "stoi"}
    lc, ic, gc = got["composed"]
    for key in ("fl", "fused"):
        lf, inf, gf = got[key]
        e_loss, e_grad = abs(float(lf) - float(lc)) / abs(float(lc)), _l2rel(gf, gc)
        SC.report("stoi_loss loss_fn %s vs composition: loss %.2e grad %.2e; stoi term %.6g" % (key, e_loss, e_grad,
                                                                                                  float(inf["stoi"])))
        assert abs(float(inf["stoi"]) - float(ic["stoi"])) <= 2e-6 * abs(float(ic["stoi"]))
        assert e_loss < 2e-6 and e_grad < 2e-5
    # the term did enter the loss and the gradient
    monkeypatch.setattr(util, "FUSED_LOSS", True)
    l0, _, g0 = step(si_sdr_lambda=0.01)
    assert abs(float(got["fused"][0]) - (float(l0) + float(got["fused"][1]["stoi"]))) < 1e-5 * abs(float(l0))
    assert not torch.equal(got["fused"][2], g0)


def test_a_few_optimiser_steps_raise_the_score():
    """sign and wiring end to end, no quality claim: Adam on the STOI term alone raises the STOI of a fixed batch"""
    from oracle import network_ref as nr, weights as W
    from tinyrecurrentunet_amd import dataset as ds, network as hn, util
    B, length = 2, 8192
    clean, noisy = W.synth_pairs(B, length, seed=9)
    clean, noisy = clean[:, 0].cuda().contiguous(), noisy[:, 0].cuda().contiguous()
    net = hn.TRUNet(input_size=4)
    net.load_state_dict(W.fill_state_dict(nr.TRUNet(input_size=4), seed=1).state_dict())
    net.cuda().train()
    f = _loss().STOILoss()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    hist = []
    for _ in range(6):
        feats = ds.stft_features(noisy, pcen=True)
        den, _ = util.denoise(net(feats), clean, feats.shape[0] // B)
        loss = f(den, clean)
        hist.append(-float(loss))
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    SC.report("stoi_loss optimiser steps: mean STOI " + " ".join("%.4f" % v for v in hist))
    assert hist[-1] > hist[0]
