"""Plain torch restatements of the BatchNorm bookkeeping and block-boundary contracts of include/trunet_hip.h
(elementwise.hip: trunet_bn_finalize_fwd / _bwd, trunet_bn_eval_affine, trunet_relu_bwd_stats, trunet_from_frames_last_affine,
trunet_conv_first_fwd, trunet_sumsq; gemm_conv.hip: trunet_reduce_partials), in the kernels' layouts:

    finalize_fwd   a, b = sum_g partials[g][c][0 / 1];  mean = a / count;  var = max(b / count - mean^2, 0)   (biased)
                   rstd = 1 / sqrt(var + eps);  scale = gamma rstd;  shift = beta - mean scale
                   running_mean = (1 - m) running_mean + m mean;  running_var = (1 - m) running_var + m unb,
                   unb = var count / (count - 1) for count > 1, var otherwise;  the int64 counter rises by 1
    finalize_bwd   a, b = sum_g partials;  m1 = a / count;  m2 = rstd b / count
                   dgamma = rstd b;  dbeta = a;  ca = gamma rstd;  cb = -gamma rstd^2 m2
                   cc = -gamma rstd m1 + gamma rstd^2 m2 mean            (dz = ca dy + cb z + cc)
    eval_affine    scale = gamma / sqrt(running_var + eps);  shift = beta - running_mean scale
    relu_bwd_stats dy[c][l][n] *= [sc[c] z + sh[c] > 0] for n < N ([z > 0] with sc None), 0 for n >= N;
                   sums (sum dy, sum dy (z - mean[c])) of the result over the frames < N
    from_frames_last_affine   y[n][c][l] = max(scale[c] x[c][l][n] + shift[c], relu ? 0 : -inf) for n < N
    conv_first     y[co][lo][n] = relu(b[co] + sum_{ci,k} w[co][ci][k] x[ci][lo S + k - S/2][n])   (padding S/2, NOT K/2)
    reduce_partials out[i] (+)= sum_g partials[g][i]
    sumsq          sum g^2

dtype = float64 is the reference (of the fp32 INPUTS: eps and momentum are the fp32 values the C ABI receives).  float32 is
the yardstick for the outputs that have fp32 summation behind them, in two plain orders per function (`order`); for the
finalize functions float32 means the whole formula in fp32 -- no kernel does that, it is there to show what the double
accumulation buys (tests/test_bn_ref_cpu.py).

`mut` names ONE deliberate error (MUTANTS); tests/test_bn_ref_cpu.py passes each through the comparison of the GPU test in
place of kernel output."""
import torch
import torch.nn.functional as F

MUTANTS = ("mask_ge", "mask_raw", "count_pad", "no_mean", "var_unbiased", "cc_sign", "cb_no_rstd", "pad_k2", "clip_last_tap",
           "chan_div", "drop_parts_256", "running_var_biased")
RELU_PARTS = 16            # trunet_relu_bwd_stats_nparts()
K_FIRST = 5


def f32(v):
    """the fp32 value a C float argument carries, as a double"""
    return float(torch.tensor(v, dtype=torch.float32).double())


def _chain(t):
    """ONE strictly sequential chain in t's dtype over the last axis"""
    acc = torch.zeros(t.shape[:-1], dtype=t.dtype)
    for i in range(t.shape[-1]):
        acc = acc + t[..., i]
    return acc


def _sum_parts(p, dtype, order, mut):
    """sum over the leading (parts) axis"""
    if mut == "drop_parts_256":
        p = p[:256]
    p = p.to(dtype)
    return _chain(p.movedim(0, -1)) if order == "seq" else p.sum(0)


def finalize_fwd(partials, count, gamma, beta, eps, momentum, running_mean=None, running_var=None, dtype=torch.float64,
                 order="blocked", mut=None):
    """partials [nparts][C][2] fp32.  Returns {scale, shift, mean, rstd, var (biased, clamped), running_mean, running_var
    (None without running statistics), nbt_inc}."""
    assert order in ("blocked", "seq") and (mut is None or mut in MUTANTS)
    s = _sum_parts(partials, dtype, order, mut)
    cnt, eps, mom = float(count), f32(eps), f32(momentum)
    mean = s[:, 0] / cnt
    var = (s[:, 1] / cnt - mean * mean).clamp_min(0)
    unb = var * cnt / (cnt - 1.0) if cnt > 1.0 else var
    if mut == "var_unbiased":
        var, unb = unb, var
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma.to(dtype) * rstd
    out = {"scale": scale, "shift": beta.to(dtype) - mean * scale, "mean": mean, "rstd": rstd, "var": var,
           "running_mean": None, "running_var": None, "nbt_inc": 1}
    if running_mean is not None:
        out["running_mean"] = (1.0 - mom) * running_mean.to(dtype) + mom * mean
        # running_var_biased: the normalisation is right, running_var alone takes the biased variance at count > 1
        out["running_var"] = (1.0 - mom) * running_var.to(dtype) + mom * (var if mut == "running_var_biased" else unb)
    return out


def finalize_bwd(partials, count, gamma, mean, rstd, dtype=torch.float64, order="blocked", mut=None):
    """partials [nparts][C][2] = sum dy, sum dy (z - mean).  Returns {dgamma, dbeta, ca, cb, cc}."""
    assert order in ("blocked", "seq") and (mut is None or mut in MUTANTS)
    s = _sum_parts(partials, dtype, order, mut)
    cnt = float(count)
    a, b = s[:, 0], s[:, 1]
    r, g, mu = rstd.to(dtype), gamma.to(dtype), mean.to(dtype)
    m1, m2 = a / cnt, r * b / cnt
    cb = -g * r * m2 if mut == "cb_no_rstd" else -g * r * r * m2
    second = g * r * r * m2 * mu
    return {"dgamma": r * b, "dbeta": a, "ca": g * r, "cb": cb, "cc": -g * r * m1 + (-second if mut == "cc_sign" else second)}


def eval_affine(gamma, beta, running_mean, running_var, eps, dtype=torch.float64):
    scale = gamma.to(dtype) / torch.sqrt(running_var.to(dtype) + f32(eps))
    return {"scale": scale, "shift": beta.to(dtype) - running_mean.to(dtype) * scale}


def relu_items(t, parts=RELU_PARTS):
    """[C][L][NP] -> [C][parts][J][8 * 128]: the elements workgroup g of trunet_relu_bwd_stats visits, in its order (item
    it = nt L + l is 128 frames of one row; workgroup g takes items g 8 + ly + j 8 parts, ly < 8), zeros for missing items"""
    Cn, L, NP = t.shape
    ntn = NP // 128
    items = L * ntn
    x = t.view(Cn, L, ntn, 128).permute(0, 2, 1, 3).reshape(Cn, items, 128)
    J = -(-items // (8 * parts))
    x = torch.cat([x, torch.zeros(Cn, J * 8 * parts - items, 128, dtype=t.dtype)], 1)
    return x.view(Cn, J, parts, 8 * 128).permute(0, 2, 1, 3).contiguous()


def relu_bwd_stats(dy, z, sc, sh, mean, N, dtype=torch.float64, order="blocked", mut=None):
    """dy, z [C][L][NP]; sc, sh, mean [C] or None.  Returns {dy (masked), parts [RELU_PARTS][C][2], s1, s2 [C]} (the sums
    are zeros with mean None).  order: `seq` = one chain per workgroup over its elements, `blocked` = torch sums per
    128-frame item, then over the items; the parts are added in double either way, as trunet_bn_finalize_bwd does."""
    assert order in ("blocked", "seq") and (mut is None or mut in MUTANTS)
    Cn, L, NP = dy.shape
    d, zz = dy.to(dtype), z.to(dtype)
    col = lambda v: v.to(dtype)[:, None, None]
    zero = torch.zeros((), dtype=dtype)
    pre = zz if (sc is None or mut == "mask_raw") else col(sc) * zz + col(sh)
    live = (torch.arange(NP) < N)[None, None, :]
    mask = (pre >= 0 if mut == "mask_ge" else pre > 0) & live
    out = torch.where(mask, d, zero)
    res = {"dy": out, "parts": torch.zeros(RELU_PARTS, Cn, 2, dtype=dtype), "s1": torch.zeros(Cn, dtype=dtype),
           "s2": torch.zeros(Cn, dtype=dtype)}
    if mean is None:
        return res
    sel = (pre > 0) | ~live if mut == "count_pad" else mask                      # count_pad: frames >= N enter the sums
    cen = zz if mut == "no_mean" else zz - col(mean)
    t1, t2 = relu_items(torch.where(sel, d, zero)), relu_items(torch.where(sel, d * cen, zero))
    if order == "seq":
        p1, p2 = _chain(t1.flatten(2)), _chain(t2.flatten(2))
    else:
        p1 = t1.view(Cn, RELU_PARTS, -1, 128).sum(-1).sum(-1)
        p2 = t2.view(Cn, RELU_PARTS, -1, 128).sum(-1).sum(-1)
    res["parts"] = torch.stack([p1.t(), p2.t()], -1)
    res["s1"], res["s2"] = p1.double().sum(1).to(dtype), p2.double().sum(1).to(dtype)
    return res


def from_frames_last_affine(x, N, scale, shift, relu, dtype=torch.float64, mut=None):
    """x [C][L][NP] -> y [N][C][L]"""
    Cn, L, NP = x.shape
    ch = torch.arange(Cn * L) // ((L + 1) if mut == "chan_div" else L)
    v = x.to(dtype).reshape(Cn * L, NP) * scale.to(dtype)[ch][:, None] + shift.to(dtype)[ch][:, None]
    if relu:
        v = v.clamp_min(0)
    return v[:, :N].t().reshape(N, Cn, L).contiguous()


def lout_first(Lin, S, K=K_FIRST):
    return (Lin + 2 * (S // 2) - K) // S + 1


def conv_first(x, w, b, S, dtype=torch.float64, order="blocked", mut=None):
    """x [Cin][Lin][NP], w [Cout][Cin][K], b [Cout] -> y [Cout][Lout][NP].  `blocked` is F.conv1d(padding = S // 2) + ReLU
    (the reference's StandardConv1d); `seq` -- and every mutant -- is one sequential fma-free chain over (ci, k) from the
    bias, with explicit row gathers."""
    assert order in ("blocked", "seq") and (mut is None or mut in MUTANTS)
    Cin, Lin, NP = x.shape
    Cout, _, K = w.shape
    Lo = lout_first(Lin, S, K)
    xx, ww, bb = x.to(dtype), w.to(dtype), b.to(dtype)
    if order == "blocked" and mut is None:
        y = F.conv1d(xx.permute(2, 0, 1), ww, bb, stride=S, padding=S // 2)
        assert y.shape == (NP, Cout, Lo)
        return torch.relu(y).permute(1, 2, 0).contiguous()
    pad = K // 2 if mut == "pad_k2" else S // 2
    l_end = Lin - 1 if mut == "clip_last_tap" else Lin
    acc = bb[:, None, None].expand(Cout, Lo, NP).clone()
    lo = torch.arange(Lo)
    for ci in range(Cin):
        for k in range(K):
            li = lo * S + k - pad
            ok = (li >= 0) & (li < l_end)
            rows = torch.where(ok[:, None], xx[ci][li.clamp(0, Lin - 1)], torch.zeros((), dtype=dtype))     # [Lo][NP]
            acc = acc + ww[:, ci, k, None, None] * rows[None]
    return torch.relu(acc)


def reduce_partials(partials, out0=None, dtype=torch.float64, order="blocked", mut=None):
    """partials [nparts][numel]; out0 [numel] with accumulate = 1, None with accumulate = 0"""
    t = _sum_parts(partials, dtype, order, mut)
    return t if out0 is None else out0.to(dtype) + t


def sumsq(g, dtype=torch.float64, order="blocked"):
    v = g.to(dtype)
    return _chain(v * v) if order == "seq" else (v * v).sum()
