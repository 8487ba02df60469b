"""Plain torch restatement of the loss tail of include/trunet_hip.h (fft.hip): the multi-resolution STFT loss kernels
(trunet_stft_mag / _mag_bwd, trunet_stft_loss_fwd / _fwdgrad / _bwd_gather), the gradient gather (trunet_loss_grad_gather),
the scalar end (trunet_reduce_cols, trunet_loss_finalize), the L1 term (trunet_l1_grad) and the phase-aware mask + iSTFT
with its backward (trunet_mask_istft_fwd / _bwd).  Written from the header's contracts with explicit index maps and an
explicit DFT matrix; torch.stft / torch.istft appear nowhere (tests/test_losstail_ref_cpu.py holds this file to autograd
through them).

    frames     F = 1 + L // hop;  frame f, tap i reads x[reflect(f hop + i - n/2)],  reflect: j -> |j|, j >= L -> 2 (L-1) - j
    window     Hann(wl) (periodic) zero-padded to n, left = (n - wl) // 2
    spectrum   X[k] = sum_i w[i] frame[i] e^{-2 pi j k i / n},  k <= n/2;   px = re^2 + im^2,  xm = sqrt(max(px, 1e-7))
    partials   per frame:  sum_k (ym - xm)^2,  sum_k ym^2,  sum_k |log ym - log xm|
    gradient   fr_sc[f][i]  = w[left + i] Re sum_k Gs[k] e^{+2 pi j k (left + i) / n},  Gs = (xm - ym) X / xm
               fr_mag[f][i] = the same with Gm = sign(log xm - log ym) X / xm^2;  Gs = Gm = 0 where px <= 1e-7 (the clamp
               passes no gradient at or below its floor), sign(0) = 0
    gather     the adjoint of the reflect pad as a SCATTER: frames overlap-added into the padded line, the line folded back
               onto the samples through the index map the staging reads with (one map for both directions)
    algebra    trunet_loss_finalize: see `loss_finalize`
    mask       A = 10^(2.5 (clamp(c0, -1, 1) + 1) - 3.75),  S = sigmoid(beta (atan2(c2, c3) - atan2(c6, c7))),
               X = S A e^{j atan2(c2, c3)}, the imaginary part of DC and Nyquist dropped
    iSTFT      frame = irfft(X) (1 / 512 inside), overlap-add at hop 128 into the line padded by 256, every sample divided
               by the number of frames that cover it, samples [256, 256 + L)
    L1         l1_partials[b][blk] = sum over 256 samples of |audio - clean| (the last block of L = 128 odd has 128)

CONTRACT of the mask backward (`mask_bwd`, by hand): the gradient of a phase pair is ZERO where the pair is exactly
(0, 0) -- c2^2 + c3^2 == 0 zeroes g2, g3 and c6^2 + c7^2 == 0 zeroes g6, g7 (torch's atan2 backward is NaN there; the
kernel's 0 is deliberate) -- and the clamp passes its gradient on the CLOSED interval -1 <= c0 <= 1.

dtype = float64 is the reference.  float32 is the yardstick, in two orders of the same restatement: `dft` (the fp32 DFT
matrix product) and `fft` (torch.fft in fp32 on the same staged frames; fr_sc and fr_mag out of ONE inverse transform, as
trunet_stft_loss_fwdgrad's one pass has them); `yardstick` keeps, element by element, the one further from the reference.  The spectra of x and y come from two separate, identical transforms and frames that are equal
as inputs get equal spectra (a matrix product need not give equal rows equal results), so x == y decides sign(0) in every
dtype the way exact arithmetic does.

Counted roundings of trunet_loss_finalize (U = 2^-24; the column sums are exact doubles up to D = 2^-50 sum|terms|):
    vals[1] = (float) |sum / count|                                     1 rounding            2 U |ref|
    vals[4] = (float) (1 / count)                                       1                     2 U |ref|
    S_j = (float) sum;  r_j = sqrtf(S_j): U/2 carried + U               1.5 U each
    sc_i = r1 / r2: 1.5 + 1.5 + 1 = 4 U;   mag_i = S3 / (float) count: U + U + U = 3 U;   the sums over i are double
    vals[2] = (float) scs * lam_sc / nres * lam:  4 + 1 + 3 = 8 roundings                    9 U |ref|
    vals[3] = (float) mgs * lam_mag / nres * lam: 3 + 1 + 3 = 7                              8 U |ref|
    vals[0] = (float) l1 + (vals[2] + vals[3]): the terms' own roundings and two additions    12 U (|l1| + |sc| + |mag|)
    c_sc  = lam * lam_sc / nres / (r1 r2): (1.5 + 1.5 + 1) + 3 = 7                            8 U |ref|;  exactly 0 at S1 == 0
    c_mag = lam * lam_mag / nres / (float) count: 3 + 1 = 4                                   5 U |ref|
(bounds are (r + 1) U |ref| as in tests/bn_cases.py).  trunet_reduce_cols is ONE rounding of the exact column sum
(2 U |ref| + D sum|terms|) and trunet_l1_grad is exact bits.

`mut` names ONE deliberate error (MUTANTS); tests/test_losstail_ref_cpu.py passes each through the comparison of the GPU
test in place of kernel output."""
import functools
import math

import torch

MUTANTS = ("reflect_right_off1", "no_left_reflect", "frames_ceil", "win_left_ceil", "clamp_passes_grad", "mag_sign_flipped",
           "sign0_is_plus", "dc_weight_2", "nyquist_imag_kept", "env_uncapped", "env_always_4", "gather_drops_last_frame",
           "coef_swapped", "l1_tail_block_dropped", "clamp_open_interval")
FLOOR = 1e-7
NF, HOPF, BINS = 512, 128, 257
f64 = torch.float64


def f32(v):
    """the fp32 value a C float argument carries, as a double"""
    return float(torch.tensor(v, dtype=torch.float32).double())


# ---------------------------------------------------------------------------------------------- staging
def nframes(L, hop, mut=None):
    return 1 + (-(-L // hop) if mut == "frames_ceil" else L // hop)


def pad_map(L, n, hop, mut=None):
    """sample index of every position of the reflect-padded line (position p is sample p - n/2), long enough for all
    frames.  The one index map of the staging (read) and of the gradient's fold (index_add)."""
    F = nframes(L, hop, mut)
    j = torch.arange((F - 1) * hop + n) - n // 2
    if mut == "no_left_reflect":
        j = j.clamp_min(0)
    j = j.abs()
    over = 2 * (L - 1) - j + (1 if mut == "reflect_right_off1" else 0)
    j = torch.where(j >= L, over, j)
    return j.clamp(0, L - 1)          # no effect on the contract's map (L > n/2); keeps the mutants inside the signal


def window(n, wl, dtype, mut=None):
    """(padded window [n], left)"""
    left = (n - wl + 1) // 2 if mut == "win_left_ceil" else (n - wl) // 2
    w = torch.zeros(n, dtype=f64)
    w[left:left + wl] = torch.hann_window(wl, dtype=f64)
    return w.to(dtype), left


def stage(x, n, hop, wl, dtype, mut=None):
    """x (B, L) -> windowed frames (B, F, n)"""
    L = x.shape[1]
    idx = pad_map(L, n, hop, mut)
    w, _ = window(n, wl, dtype, mut)
    return x.to(dtype)[:, idx].unfold(1, n, hop) * w


@functools.lru_cache(maxsize=None)
def dft_matrices(n, dtype):
    """C[k][i] = cos(2 pi k i / n), S[k][i] = sin(2 pi k i / n), k <= n/2, from exact integer phases in double"""
    ph = (torch.arange(n // 2 + 1)[:, None] * torch.arange(n)[None, :]) % n
    ang = ph.to(f64) * (2.0 * math.pi / n)
    return torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)


def spectrum(fr, order):
    """frames (..., n) real -> (re, im) (..., n/2 + 1)"""
    n = fr.shape[-1]
    if order == "fft":
        Z = torch.fft.fft(fr, dim=-1)[..., :n // 2 + 1]
        return Z.real.contiguous(), Z.imag.contiguous()
    Cm, Sm = dft_matrices(n, fr.dtype)
    return fr @ Cm.t(), -(fr @ Sm.t())


def half_inverse(gre, gim, n, order):
    """a[i] = Re sum_{k <= n/2} G[k] e^{+2 pi j k i / n}: the adjoint of `spectrum` (no Hermitian doubling: the loss sees
    the bins k <= n/2 once each)"""
    if order == "fft":
        G = torch.zeros(gre.shape[:-1] + (n,), dtype=torch.complex128 if gre.dtype == f64 else torch.complex64)
        G[..., :n // 2 + 1] = torch.complex(gre, gim)
        return torch.fft.ifft(G, dim=-1, norm="forward").real.contiguous()
    Cm, Sm = dft_matrices(n, gre.dtype)
    return gre @ Cm - gim @ Sm


def spectra(x, y, n, hop, wl, dtype, order, mut=None):
    """(Xre, Xim, Yre, Yim), each (B, F, n/2 + 1).  Two separate transforms; frames equal as inputs get equal spectra."""
    fx, fy = stage(x, n, hop, wl, dtype, mut), stage(y, n, hop, wl, dtype, mut)
    xr, xi = spectrum(fx, order)
    yr, yi = spectrum(fy, order)
    same = (fx == fy).all(-1, keepdim=True)
    return torch.where(same, yr, xr), torch.where(same, yi, xi), yr, yi


def mags(re, im):
    px = re * re + im * im
    return px, torch.sqrt(px.clamp_min(FLOOR))


# ---------------------------------------------------------------------------------------------- gather
def ola_scatter(fr, L, n, hop, wl, order="dft", mut=None):
    """fr (B, F, wl) windowed gradient frames -> (B, L): overlap-add into the padded line, then the fold.  `order`: the
    frames are added in ascending (`dft`) or descending (`fft`) order -- the two fp32 orders of this stage."""
    B, F, _ = fr.shape
    _, left = window(n, wl, fr.dtype, mut)
    idx = pad_map(L, n, hop, mut)
    line = torch.zeros(B, idx.numel(), dtype=fr.dtype)
    fs = range(F - 1 if mut == "gather_drops_last_frame" else F)
    for f in (reversed(fs) if order == "fft" else fs):
        line[:, f * hop + left:f * hop + left + wl] += fr[:, f]
    g = torch.zeros(B, L, dtype=fr.dtype)
    own = torch.arange(L) + n // 2                        # the positions that ARE the samples first, then the reflections
    own = own[own < idx.numel()]                          # (hop > n/2 can leave the last samples outside every frame)
    g[:, :own.numel()] += line[:, own]
    rest = torch.ones(idx.numel(), dtype=torch.bool)
    rest[own] = False
    g.index_add_(1, idx[rest], line[:, rest])
    return g


# ---------------------------------------------------------------------------------------------- the STFT kernels
def stft_all(x, y, n, hop, wl, dtype=f64, order="dft", mut=None, coef=None, gmag=None):
    """Everything the five STFT entry points write, for x (predicted), y (target) (B, L) fp32:
    xmag, ymag (B, F, n/2+1); partials (B F, 3); fr_sc, fr_mag (B, F, wl); g_sc, g_mag (B, L) = OLA of the two;
    with coef (2): bwd_frames (B, F, wl), bwd_gx (B, L) of trunet_stft_loss_bwd_gather;
    with gmag (B, F, n/2+1): magbwd_frames, magbwd_gx of trunet_stft_mag_bwd."""
    assert order in ("dft", "fft") and (mut is None or mut in MUTANTS)
    B, L = x.shape
    xr, xi, yr, yi = spectra(x, y, n, hop, wl, dtype, order, mut)
    px, xm = mags(xr, xi)
    _, ym = mags(yr, yi)
    F = xm.shape[1]
    d = ym - xm
    dl = torch.log(xm) - torch.log(ym)
    out = {"xmag": xm, "ymag": ym, "px": px, "dl": dl, "xre": xr, "xim": xi, "yre": yr, "yim": yi,
           "partials": torch.stack([(d * d).sum(-1), (ym * ym).sum(-1), dl.abs().sum(-1)], -1).reshape(B * F, 3)}
    zero = torch.zeros((), dtype=dtype)
    live = torch.ones_like(px, dtype=torch.bool) if mut == "clamp_passes_grad" else px > FLOOR
    sg = torch.sign(dl)
    if mut == "sign0_is_plus":
        sg = torch.where(dl == 0, torch.ones((), dtype=dtype), sg)
    if mut == "mag_sign_flipped":
        sg = -sg
    w, left = window(n, wl, dtype, mut)
    ws = w[left:left + wl]

    def frames_of(g_xm):
        """per-bin cotangent of xm -> windowed frames over the window's support"""
        gre = torch.where(live, g_xm * xr / xm, zero)
        gim = torch.where(live, g_xm * xi / xm, zero)
        return half_inverse(gre, gim, n, order)[..., left:left + wl] * ws

    if order == "fft":
        # trunet_stft_loss_fwdgrad's contract is ONE pass: both tables come out of one inverse transform (two real
        # sequences share a complex one: Z = Herm(Gs) + j Herm(Gm)), so the rounding error of either table is relative to
        # the LARGER of the two spectra -- |Gm| = 1 / xm is hundreds of times |Gs| at a weak bin.  The transform order of
        # the yardstick does the same; in exact arithmetic it is the two separate inverses of the `dft` order.
        def herm(g_xm):
            G = torch.zeros(px.shape[:-1] + (n,), dtype=torch.complex128 if dtype == f64 else torch.complex64)
            h = 0.5 * torch.complex(torch.where(live, g_xm * xr / xm, zero), torch.where(live, g_xm * xi / xm, zero))
            G[..., 1:n // 2] = h[..., 1:n // 2]
            G[..., n // 2 + 1:] = torch.conj(h[..., 1:n // 2]).flip(-1)
            G[..., 0], G[..., n // 2] = 2.0 * h[..., 0].real, 2.0 * h[..., n // 2].real
            return G
        z = torch.fft.ifft(herm(xm - ym) + 1j * herm(sg / xm), dim=-1, norm="forward")[..., left:left + wl]
        out["fr_sc"], out["fr_mag"] = z.real * ws, z.imag * ws
    else:
        out["fr_sc"], out["fr_mag"] = frames_of(xm - ym), frames_of(sg / xm)
    out["g_sc"] = ola_scatter(out["fr_sc"], L, n, hop, wl, order, mut)
    out["g_mag"] = ola_scatter(out["fr_mag"], L, n, hop, wl, order, mut)
    if coef is not None:
        c_sc, c_mag = (coef[1], coef[0]) if mut == "coef_swapped" else (coef[0], coef[1])
        out["bwd_frames"] = frames_of(c_sc.to(dtype) * (xm - ym) + c_mag.to(dtype) * sg / xm)
        out["bwd_gx"] = ola_scatter(out["bwd_frames"], L, n, hop, wl, order, mut)
    if gmag is not None:
        if gmag.shape[1] < F:                             # frames_ceil: the extra frame has no cotangent
            gmag = torch.cat([gmag, torch.zeros(B, F - gmag.shape[1], gmag.shape[2])], 1)
        out["magbwd_frames"] = frames_of(gmag.to(dtype))
        out["magbwd_gx"] = ola_scatter(out["magbwd_frames"], L, n, hop, wl, order, mut)
    return out


def loss_grad_gather(res, audio, clean, vals, g_loss, dtype=f64, order="dft", mut=None):
    """res: list of (fr_sc, fr_mag (B, F, wl) fp32, n, hop, wl); vals fp32 (5 + 2 nres); g_loss a number.  (B, L):
    g_loss (vals[4] sign(audio - clean) + sum_r (vals[5 + 2r] OLA_r(fr_sc_r) + vals[6 + 2r] OLA_r(fr_mag_r)))"""
    B, L = audio.shape
    v = vals.to(dtype)
    total = v[4] * torch.sign(audio.to(dtype) - clean.to(dtype))
    for r, (fs, fm, n, hop, wl) in enumerate(res):
        a, b = (6, 5) if mut == "coef_swapped" else (5, 6)
        total = total + v[a + 2 * r] * ola_scatter(fs.to(dtype), L, n, hop, wl, order, mut) \
            + v[b + 2 * r] * ola_scatter(fm.to(dtype), L, n, hop, wl, order, mut)
    return torch.as_tensor(g_loss, dtype=dtype) * total


# ---------------------------------------------------------------------------------------------- the scalar end
def reduce_cols(parts, dtype=f64):
    """parts (rows, ncols) -> (ncols)"""
    return parts.to(dtype).sum(0)


def loss_finalize(l1_partials, l1_count, parts, counts, sc_lambda, mag_lambda, stft_lambda, dtype=f64):
    """l1_partials (n_l1) fp32; parts: list of (rows_i, 3) fp32; counts: list.  Returns vals (5 + 2 nres):
    [0] loss [1] l1 [2] stft_lambda lam_sc sum_i sc_i / nres [3] the same for mag [4] 1 / l1_count
    [5 + 2i] c_sc_i = stft_lambda lam_sc / (nres sqrt(S1) sqrt(S2)), 0 at S1 == 0   [6 + 2i] c_mag_i = stft_lambda lam_mag /
    (nres count_i);  sc_i = sqrt(S1) / sqrt(S2), mag_i = S3 / count_i.  The lambdas are the fp32 values the C struct carries."""
    lsc, lmg, lam = f32(sc_lambda), f32(mag_lambda), f32(stft_lambda)
    nres = len(parts)
    vals = torch.zeros(5 + 2 * nres, dtype=dtype)
    l1 = (l1_partials.to(dtype).sum() / l1_count).abs()
    scs, mgs = torch.zeros((), dtype=dtype), torch.zeros((), dtype=dtype)
    for i, (p, cnt) in enumerate(zip(parts, counts)):
        S = p.to(dtype).sum(0)
        r1, r2 = torch.sqrt(S[0]), torch.sqrt(S[1])
        scs, mgs = scs + r1 / r2, mgs + S[2] / cnt
        vals[5 + 2 * i] = lam * lsc / nres / (r1 * r2) if float(S[0]) > 0 else 0.0
        vals[6 + 2 * i] = lam * lmg / nres / cnt
    div = nres if nres > 0 else 1
    vals[2], vals[3] = scs * lsc / div * lam, mgs * lmg / div * lam
    vals[1], vals[4] = l1, 1.0 / l1_count
    vals[0] = l1 + (vals[2] + vals[3])
    return vals


def l1_grad(den, clean, scale):
    """exact: scale * sign(den - clean) in the inputs' own fp32"""
    return scale * torch.sign(den - clean)


# ---------------------------------------------------------------------------------------------- mask + iSTFT
def env_count(T, mut=None):
    """number of frames covering every position of the padded line (length 128 (T - 1) + 512)"""
    P = HOPF * (T - 1) + NF
    if mut == "env_always_4":
        return torch.full((P,), 4.0, dtype=f64)
    cnt = torch.zeros(P + NF, dtype=f64)
    for t in range(T + 3 if mut == "env_uncapped" else T):          # uncapped: as if the frames went on past T - 1
        cnt[HOPF * t:HOPF * t + NF] += 1
    return cnt[:P]


def _mask_vals(o, beta, dtype):
    c = [o[:, k].to(dtype) for k in range(8)]
    A = torch.pow(torch.tensor(10.0, dtype=dtype), 2.5 * (c[0].clamp(-1, 1) + 1.0) - 3.75)
    pm, pn = torch.atan2(c[2], c[3]), torch.atan2(c[6], c[7])
    S = torch.sigmoid(beta * (pm - pn))
    return c, A, S, pm


def _irfft_frames(re, im, order, dtype):
    """(N, 257) half spectra (imaginary DC / Nyquist already dropped) -> (N, 512), 1 / 512 inside"""
    if order == "fft":
        return torch.fft.irfft(torch.complex(re, im), n=NF, dim=-1)
    Cm, Sm = dft_matrices(NF, dtype)
    wk = torch.full((BINS,), 2.0, dtype=dtype)
    wk[0] = wk[NF // 2] = 1.0
    return ((re * wk) @ Cm - (im * wk) @ Sm) / NF


def mask_istft_fwd(net_out, T, beta, clean=None, dtype=f64, order="dft", mut=None):
    """net_out (B T, 8, 257) fp32 -> {frames (B, T, 512), audio (B, L), l1 (B ceil(L / 256)) with clean}"""
    assert order in ("dft", "fft") and (mut is None or mut in MUTANTS)
    B, L = net_out.shape[0] // T, HOPF * (T - 1)
    beta = f32(beta)
    c, A, S, pm = _mask_vals(net_out, beta, dtype)
    M = S * A
    re, im = M * torch.cos(pm), M * torch.sin(pm)
    leak = im[:, NF // 2].clone()
    im[:, 0] = 0
    im[:, NF // 2] = 0
    frames = _irfft_frames(re, im, order, dtype).view(B, T, NF)
    if mut == "nyquist_imag_kept":
        # two frames share one complex transform: an imaginary Nyquist part that is kept lands, as a real part, in the
        # partner frame (2i <-> 2i + 1)
        lk = leak.view(B, T)
        alt = torch.tensor([1.0, -1.0], dtype=dtype).repeat(NF // 2) / NF
        for t in range(T):
            p = t ^ 1
            if p < T:
                frames[:, t] += (-1.0 if t % 2 == 0 else 1.0) * lk[:, p, None] * alt
    line = torch.zeros(B, L + NF, dtype=dtype)
    for t in range(T):
        line[:, HOPF * t:HOPF * t + NF] += frames[:, t]
    audio = (line / env_count(T, mut).to(dtype))[:, NF // 2:NF // 2 + L]
    out = {"frames": frames, "audio": audio}
    if clean is not None:
        nb = -(-L // 256)
        ad = torch.zeros(B, nb * 256, dtype=dtype)
        ad[:, :L] = (audio - clean.to(dtype)).abs()
        l1 = ad.view(B, nb, 256).sum(-1)
        if mut == "l1_tail_block_dropped" and L % 256:
            l1[:, -1] = 0
        out["l1"] = l1.reshape(-1)
    return out


def mask_istft_bwd(g_audio, net_out, T, beta, dtype=f64, order="dft", mut=None):
    """g_audio (B, L), net_out (B T, 8, 257) -> g_net (B T, 8, 257), by hand (the CONTRACT in the module docstring)"""
    assert order in ("dft", "fft") and (mut is None or mut in MUTANTS)
    B, L = g_audio.shape
    beta = f32(beta)
    gl = torch.zeros(B, L + NF, dtype=dtype)
    gl[:, NF // 2:NF // 2 + L] = g_audio.to(dtype)
    gl = gl / env_count(T, mut).to(dtype)
    gf = gl.unfold(1, NF, HOPF).reshape(B * T, NF)                # frame t = positions [128 t, 128 t + 512)
    gr, gi = spectrum(gf, order)
    wk = torch.full((BINS,), 2.0 / NF, dtype=dtype)
    if mut != "dc_weight_2":
        wk[0] = wk[NF // 2] = 1.0 / NF
    dRe, dIm = wk * gr, wk * gi
    dIm[:, 0] = 0
    dIm[:, NF // 2] = 0
    c, A, S, pm = _mask_vals(net_out, beta, dtype)
    r2m, r2n = c[2] * c[2] + c[3] * c[3], c[6] * c[6] + c[7] * c[7]
    cm, sm = torch.cos(pm), torch.sin(pm)
    M = S * A
    dM = dRe * cm + dIm * sm
    du = dM * A * S * (1.0 - S)
    dpm = M * (dIm * cm - dRe * sm) + beta * du
    dpn = -beta * du
    inside = (c[0] > -1) & (c[0] < 1) if mut == "clamp_open_interval" else (c[0] >= -1) & (c[0] <= 1)
    zero = torch.zeros((), dtype=dtype)
    g = torch.zeros(net_out.shape, dtype=dtype)
    g[:, 0] = torch.where(inside, dM * S * A * (2.5 * math.log(10.0)), zero)
    okm, okn = r2m > 0, r2n > 0
    sm2, sn2 = torch.where(okm, r2m, torch.ones((), dtype=dtype)), torch.where(okn, r2n, torch.ones((), dtype=dtype))
    g[:, 2] = torch.where(okm, dpm * c[3] / sm2, zero)
    g[:, 3] = torch.where(okm, -dpm * c[2] / sm2, zero)
    g[:, 6] = torch.where(okn, dpn * c[7] / sn2, zero)
    g[:, 7] = torch.where(okn, -dpn * c[6] / sn2, zero)
    return g


def yardstick(ref64, a, b):
    """element by element the fp32 result further from the reference"""
    return torch.where((b.double() - ref64).abs() > (a.double() - ref64).abs(), b, a)
