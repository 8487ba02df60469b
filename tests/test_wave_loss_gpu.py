"""GPU: the time-domain loss terms (csrc/wave_loss.hip) against float64 torch on the CPU on the same fp32
inputs -- F.cosine_similarity per segment and the SI-SDR expression, with autograd.

Bars (from a CPU emulation of the prescribed arithmetic -- fp64 sums, fp32 coefficients, fp32 A y + B x + C -- which differs
from float64 autograd by at most 1.8e-8 relative in the loss and 1.1e-6 of max|g| in the gradient at 20 dB):
vals and terms 1e-6 relative (one fp32 rounding is 6e-8), gradient 1e-5 of max|g| of the tensor."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tinyrecurrentunet_amd import cos_loss as cl

pytestmark = pytest.mark.gpu

DEFAULT_G = [508, 1016, 2032, 4062]
SHAPES = {"whole": (4224, DEFAULT_G), "clipped": (2944, DEFAULT_G), "empty": (1920, DEFAULT_G),
          "uniform": (8064, cl.CosSimLoss.uniform(504, 8064).g), "odd": (4224, [3, 510, 1021, 4001])}
MODES = {"cos": (1.0, 0.0), "si_sdr": (0.0, 1.0), "both": (0.7, 0.05)}
UP = 2.5                                  # upstream gradient
COS_EPS, SI_EPS = 1e-5, 1e-8


def make_pair(B, length, snr_db, seed):
    """y = 0.1 N(0,1) + 0.01 (the DC offset exercises the centring), x = y + noise at snr_db"""
    rng = np.random.default_rng(seed)
    y = 0.1 * rng.standard_normal((B, length)) + 0.01
    n = rng.standard_normal((B, length))
    n *= np.sqrt(np.mean(y * y, 1, keepdims=True) / np.mean(n * n, 1, keepdims=True) / 10.0 ** (snr_db / 10.0))
    return torch.tensor(y + n, dtype=torch.float32), torch.tensor(y, dtype=torch.float32)


def ref64(x, y, g, cos_lambda, si_lambda, up=UP):
    """float64 on the CPU -> (weighted sum, L_cos, mean SI-SDR, terms (B, m + 1), d (up * weighted sum) / d x)"""
    x64, y64 = x.double().requires_grad_(True), y.double()
    B, length = x.shape
    b = [0] + [min(v, length) for v in g]
    cols = []
    for s, e in zip(b, b[1:]):
        cols.append(torch.ones(B, dtype=torch.float64) if e <= s else
                    1.0 - F.cosine_similarity(x64[:, s:e], y64[:, s:e], dim=1, eps=COS_EPS))
    cos_terms = torch.stack(cols, 1)
    l_cos = cos_terms.mean(0).mean()
    xm, ym = x64 - x64.mean(1, keepdim=True), y64 - y64.mean(1, keepdim=True)
    sxy, sxx, syy = (xm * ym).sum(1), (xm * xm).sum(1), (ym * ym).sum(1)
    live = syy > 0
    p = sxy * sxy / torch.where(live, syy, torch.ones_like(syy))
    sisdr = torch.where(live, 10.0 * torch.log10((p + SI_EPS) / (sxx - p + SI_EPS)), torch.zeros_like(syy))
    total = cos_lambda * l_cos - si_lambda * sisdr.mean()
    (up * total).backward()
    return (float(total.detach()), float(l_cos.detach()), float(sisdr.mean().detach()),
            torch.cat([cos_terms, sisdr[:, None]], 1).detach(), x64.grad)


def run_gpu(x, y, g, cos_lambda, si_lambda, up=UP, grad=True):
    xg = x.cuda().requires_grad_(grad)
    loss, vals, terms = cl.wave_loss(xg, y.cuda(), g=g, cos_lambda=cos_lambda, cos_eps=COS_EPS, si_sdr_lambda=si_lambda,
                                     si_sdr_eps=SI_EPS)
    if grad:
        (up * loss).backward()
    return loss.detach().cpu(), vals.cpu(), terms.cpu(), (xg.grad.cpu() if grad else None)


def relerr(got, want):
    return abs(float(got) - want) / max(abs(want), 1e-300)


def check_against_ref(x, y, g, cos_lambda, si_lambda, tag):
    want, l_cos, msi, terms64, g64 = ref64(x, y, g, cos_lambda, si_lambda)
    loss, vals, terms, grad = run_gpu(x, y, g, cos_lambda, si_lambda)
    m = len(g) if cos_lambda > 0 else 0
    assert vals.shape == (5,) and terms.shape == (x.shape[0], m + 1) and grad.shape == x.shape
    e_loss = relerr(loss, want)
    e_cos = relerr(vals[1], l_cos) if cos_lambda > 0 else 0.0
    e_si = relerr(vals[2], msi) if si_lambda > 0 else 0.0
    cols = terms64[:, :-1] if cos_lambda > 0 else terms64[:, :0]
    t64 = torch.cat([cols, terms64[:, -1:] if si_lambda > 0 else torch.zeros(x.shape[0], 1, dtype=torch.float64)], 1)
    e_terms = float(((terms.double() - t64).abs() / t64.abs().clamp_min(1e-300)).max())
    e_grad = float((grad.double() - g64).abs().max() / g64.abs().max())
    print("WAVEPARITY %s loss %.2e L_cos %.2e si_sdr %.2e terms %.2e grad %.2e" % (tag, e_loss, e_cos, e_si, e_terms, e_grad))
    assert float(vals[0]) == float(loss)
    assert e_loss < 1e-6 and e_cos < 1e-6 and e_si < 1e-6 and e_terms < 1e-6, (tag, e_loss, e_cos, e_si, e_terms)
    assert relerr(vals[3], cos_lambda * l_cos) < 1e-6 or cos_lambda == 0
    assert relerr(vals[4], -si_lambda * msi) < 1e-6 or si_lambda == 0
    assert e_grad < 1e-5, (tag, e_grad)
    assert torch.isfinite(grad).all()
    return grad


@pytest.mark.parametrize("snr_db", [0, 5, 20])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_terms_and_gradient_vs_float64(shape, snr_db):
    """each term alone and both together, upstream gradient 2.5, B = 3"""
    length, g = SHAPES[shape]
    x, y = make_pair(3, length, snr_db, seed=length + snr_db)
    for mode, (cos_lambda, si_lambda) in MODES.items():
        grad = check_against_ref(x, y, g, cos_lambda, si_lambda, "%s/%ddB/%s" % (shape, snr_db, mode))
        if mode == "cos":
            covered = min(g[-1], length)
            assert float(grad[:, covered:].abs().max()) == 0 if covered < length else True
            assert float(grad[:, :g[0]].abs().max()) > 0
    if shape == "empty":                       # the empty segment's term is exactly 1
        _, _, terms, _ = run_gpu(x, y, g, 1.0, 0.0)
        assert torch.equal(terms[:, 3], torch.ones(3))


def test_degenerate_rows_match_torch_and_stay_finite():
    """an estimate that is exactly zero on one segment (|x| <= eps: the a_x = 0 branch), and a clean row of zeros (its
    SI-SDR row is skipped)"""
    x, y = make_pair(3, 4224, 5, seed=77)
    x[0, 508:1016] = 0.0
    y[1] = 0.0
    for mode, (cos_lambda, si_lambda) in MODES.items():
        grad = check_against_ref(x, y, DEFAULT_G, cos_lambda, si_lambda, "degenerate/" + mode)
        if mode == "si_sdr":
            assert float(grad[1].abs().max()) == 0
    _, _, terms, _ = run_gpu(x, y, DEFAULT_G, 1.0, 1.0)
    assert float(terms[0, 1]) == 1.0 and float(terms[1, 4]) == 0.0 and torch.equal(terms[1, :4], torch.ones(4))


def test_a_row_does_not_depend_on_its_batch_mates():
    """row b of a batch of 4: terms bit for bit those of the row alone; gradient row x 4 bit for bit the B = 1 gradient
    (1/B is a power of two, so the scaling commutes with every rounding)"""
    g = [3, 510, 1021, 4001]
    x, y = make_pair(4, 4224, 5, seed=5)
    _, _, terms4, grad4 = run_gpu(x, y, g, 0.7, 0.05, up=1.0)
    for b in range(4):
        _, _, terms1, grad1 = run_gpu(x[b:b + 1], y[b:b + 1], g, 0.7, 0.05, up=1.0)
        assert torch.equal(terms4[b], terms1[0]), b
        assert torch.equal(grad4[b] * 4.0, grad1[0]), b


def test_results_repeat_bit_for_bit_and_the_forward_alone_gives_the_same_values():
    length, g = SHAPES["uniform"]
    x, y = make_pair(3, length, 5, seed=6)
    first = run_gpu(x, y, g, 0.7, 0.05)
    again = run_gpu(x, y, g, 0.7, 0.05)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    with torch.no_grad():
        loss, vals, terms, _ = run_gpu(x, y, g, 0.7, 0.05, grad=False)
    assert torch.equal(vals, first[1]) and torch.equal(terms, first[2]) and torch.equal(loss, first[0])


def test_rows_that_are_not_16_byte_aligned_take_the_scalar_kernels():
    """L = 4223: rows start at odd offsets, so neither the sums nor the gradient may use the vector path"""
    x, y = make_pair(3, 4223, 5, seed=8)
    check_against_ref(x, y, [3, 510, 1021, 4001], 0.7, 0.05, "unaligned/both")


def test_modules_run_on_the_kernels_and_agree_with_their_cpu_composition():
    x, y = make_pair(3, 4224, 5, seed=9)
    for mod in (cl.CosSimLoss(), cl.SISDRLoss()):
        xc = x.clone().requires_grad_(True)
        lc = mod(xc, y)
        lc.backward()
        xg = x.cuda().requires_grad_(True)
        lg = mod(xg, y.cuda())
        assert lg.is_cuda and lg.dim() == 0 and lg.requires_grad
        lg.backward()
        assert abs(float(lg.detach()) - float(lc.detach())) < 1e-5 * abs(float(lc.detach()))
        assert float((xg.grad.cpu() - xc.grad).abs().max()) < 1e-4 * float(xc.grad.abs().max())


def _l2rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def test_loss_fn_with_the_terms_fused_vs_composition_and_unchanged_without_them(monkeypatch):
    """the terms inside the fused tail against the composition (TRUNET_FUSED_LOSS=0, which adds them through the two
    modules): 2e-6 relative loss, 2e-5 relative L2 gradient (the bars of the fused-versus-composition test of the rest of
    the loss); without the keywords, and with both lambdas 0, loss and gradient are bit for bit today's"""
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
    extra = dict(cos_lambda=0.5, cos_config={"g": cl.CosSimLoss.uniform(504, 8064).g}, si_sdr_lambda=0.01)

    def step(**kw):
        net.zero_grad(set_to_none=True)
        loss, info = util.loss_fn(net, X, ell_p=1, ell_p_lambda=1, stft_lambda=1, mrstftloss=mr, **kw)
        loss.backward()
        return loss.detach(), info, net.decoder[5].LastTrCNN[3].weight.grad.clone()
    got = {}
    for fused in (True, False):
        monkeypatch.setattr(util, "FUSED_LOSS", fused)
        got[fused] = step(**extra)
        assert set(got[fused][1]) == {"l1", "stft_sc", "stft_mag", "cos", "si_sdr"}
        assert all(not v.requires_grad for v in got[fused][1].values())
    (lf, inf_f, gf), (lc, inf_c, gc) = got[True], got[False]
    e_loss, e_grad = abs(float(lf) - float(lc)) / abs(float(lc)), _l2rel(gf, gc)
    print("WAVEPARITY loss_fn fused vs composition: loss %.2e grad %.2e; terms cos %.6g si_sdr %.6g"
          % (e_loss, e_grad, float(inf_f["cos"]), float(inf_f["si_sdr"])))
    for k in ("cos", "si_sdr"):
        assert abs(float(inf_f[k]) - float(inf_c[k])) <= 2e-6 * abs(float(inf_c[k])), k
    assert e_loss < 2e-6, (float(lf), float(lc))
    assert e_grad < 2e-5, e_grad
    # the terms did enter the loss
    monkeypatch.setattr(util, "FUSED_LOSS", True)
    l0, info0, g0 = step()
    assert abs(float(lf) - (float(l0) + float(inf_f["cos"]) + float(inf_f["si_sdr"]))) < 1e-5 * abs(float(lf))
    assert float(inf_f["cos"]) > 0 and not torch.equal(gf, g0)
    for kw in (dict(cos_lambda=0, si_sdr_lambda=0), dict(cos_lambda=0.0, cos_config=extra["cos_config"], si_sdr_lambda=0.0,
                                                         si_sdr_eps=1e-6), dict(cos_config=extra["cos_config"])):
        l1, info1, g1 = step(**kw)
        assert set(info1) == set(info0) == {"l1", "stft_sc", "stft_mag"}
        assert torch.equal(l1, l0) and torch.equal(g1, g0)
