"""The loss tail (fft.hip: mask + iSTFT, L1, the STFT-loss kernels, the fused loss algebra and the gradient gather) through
the C ABI against tests/losstail_ref.py: seeded inputs, launches, the comparison and the report lines of
tests/test_losstail_gpu.py.  tests/test_losstail_ref_cpu.py feeds the same `judge_*` functions with the restatement (and
with its mutants) in place of kernel output.

Every family has  *_inputs(case) -> c,  *_gpu(c) -> got,  *_emul(c, mut) -> got (no GPU),  judge_*(c, got).

Launch hygiene (tests/bn_cases.py's `Sent`): every output and scratch buffer is prefilled with NaN and has a sentinel region
behind it in the same allocation; every element of every output is compared.

Tolerances: convt_ref.close (c = 4, f = 8 * 2^-24) with the yardstick = the element-wise worse of the two fp32 orders of
the restatement (`dft`, `fft`), measured on the same inputs against float64, never against the kernel.  Derived bounds:
trunet_reduce_cols one rounding, trunet_l1_grad exact bits, trunet_loss_finalize its counted roundings
(tests/losstail_ref.py).

CONDITIONS the STFT generator asserts (tests/test_losstail_ref_cpu.py checks them for every case), so that the reference
alone decides every branch and no element is left out of a comparison; MARGIN = 16, dX = the yardstick's spectral error
|X_fp32 - X_fp64| as the root mean square over the bins of the same frame (the worse of the two orders; a transform spreads
its rounding error evenly over the bins, so a bin's own error is a sample of it), measured on the same inputs:
    floor   every bin has X == 0 exactly, or | |X| - sqrt(1e-7) | > MARGIN dX      (px > 1e-7 decides the gradient)
    sign    every bin has log xm - log ym == 0 exactly, or |log xm - log ym| > MARGIN (dX / xm + dY / ym), with dX or dY
            zero where that magnitude sits on the floor                              (its sign is the gradient)
    l1      trunet_l1_grad and trunet_loss_grad_gather take audio and clean as INPUTS: the sign of an fp32 difference is
            the sign of the exact difference, so the yardstick's error for it is 0 and the condition holds with any margin
            (asserted: the fp32 and the fp64 sign agree in every element)
    stable  in every output of STABLE_OUT the transform order (`fft`) is inside convt_ref.close of float64 with the matrix order (`dft`)
            as the only yardstick.  The gradient of |X| has the direction X / |X|, which amplifies the transform's error by
            1 / |X|: in a draw where ONE bin far below its frame's level carries an output's largest error, the two orders
            are two samples of one random error and either can be the lucky one; such a draw is replaced, so that the
            worse-of-two yardstick of every case stands on more than one bin
Seeds are tried in order from SEEDS; a case for which none qualifies fails loudly."""
import functools
import hashlib
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bn_cases as BC  # noqa: E402
import convt_cases as CC  # noqa: E402
import convt_ref as CR  # noqa: E402
import losstail_ref as R  # noqa: E402

U, D = BC.U, BC.D
NAN = BC.NAN
f64 = torch.float64
PARITY = "parity_losstail.txt"
MARGIN = 16.0
SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)
AMP = 0.3
Sent = BC.Sent
rejected = BC.rejected


class Judge(BC.Judge):
    """tests/bn_cases.py's collector (convt_ref.close and element-wise derived bounds), reporting to parity_losstail.txt"""

    def close(self, name, got, ref64, yard):
        if tuple(got.shape) != tuple(ref64.shape):
            self.fails.append("%s %s: shape %s, expected %s" % (self.tag, name, tuple(got.shape), tuple(ref64.shape)))
            return
        super().close(name, got, ref64, yard)

    def bits(self, name, got, want):
        self.exact(got.shape == want.shape and torch.equal(got, want), "%s differs from its exact value" % name)

    def done(self):
        if not self.quiet:
            CC.report("%s: kernel error / e_y / bound  %s" % (self.tag, "  ".join(self.figs)), PARITY)
        assert not self.fails, "\n".join(self.fails)


def _gen(*key):
    return torch.Generator().manual_seed(int(hashlib.sha1(repr(key).encode()).hexdigest()[:8], 16))


def _rn(g, *s):
    return torch.randn(*s, generator=g, dtype=torch.float32)


def _lib():
    from tinyrecurrentunet_amd import _lib as Lb
    return Lb, Lb.lib()


def _tw(n):
    from tinyrecurrentunet_amd import _lib as Lb
    return Lb.twiddles(n, torch.device("cuda"))


def _cpu(d):
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d.items()}


def same_bits(a, b, what):
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), "%s: %s differs on a repeat launch" % (what, k)


# ============================================================================================== the STFT kernels
# (n, hop, wl, L): the compile-time instances n = 512 / 1024 / 2048 at L = n/2 + 1 (both reflections land on interior
# samples and overlap) and at a second L; wl == n; odd wl; the runtime-sized path at n = 8 (odd log2), 64 (wl == n,
# L = n/2 + 1), 128 (hop > wl: samples no frame covers), 256 (odd n - wl at L = n/2 + 1)
STFT_SHAPES = ((512, 50, 240, 257), (512, 128, 512, 640), (1024, 120, 600, 513), (1024, 120, 601, 1500), (2048, 240, 1200, 1025),
               (2048, 240, 1200, 2400), (8, 3, 5, 37), (64, 16, 64, 33), (128, 40, 30, 200), (256, 64, 255, 129))
# the regimes run where a frame's support is a proper part of the signal
REGIME_SHAPES = ((512, 128, 512, 640), (1024, 120, 601, 1500), (2048, 240, 1200, 2400), (8, 3, 5, 37), (128, 40, 30, 200))
# noise; y / x / both exactly zero over a whole frame support; x == y over one (sign(0)); x == y everywhere; `faint`: x at
# 1e-6 and y at 1e-3 over one support, so that 0 < px <= 1e-7 while |Y| is off its floor (the clamp's gradient branch with a
# non-zero spectrum behind it)
REGIMES = ("noise", "silence_y", "silence_x", "silence_xy", "equal_bins", "identical", "faint")
STFT_CASES = [s + ("noise",) for s in STFT_SHAPES] + [s + (r,) for s in REGIME_SHAPES for r in REGIMES[1:]]
STFT_B = 2
STFT_OUT = ("xmag", "ymag", "partials", "fr_sc", "fr_mag", "bwd_frames", "bwd_gx", "magbwd_frames", "magbwd_gx", "fused_gx")
# the outputs of the `stable` condition: fr_sc and what is built on it are left out -- there the transform order carries,
# by construction, the cross-talk of the shared inverse transform (tests/losstail_ref.py) and the matrix order does not
STABLE_OUT = ("xmag", "ymag", "partials", "fr_mag", "bwd_frames", "bwd_gx", "magbwd_frames", "magbwd_gx")


def stft_id(case):
    return "n%d-h%d-w%d-L%d-%s" % case


def frame_support(n, hop, wl, L, f):
    """the samples frame f's window support reads (reflections included)"""
    left = (n - wl) // 2
    return R.pad_map(L, n, hop)[f * hop + left:f * hop + left + wl].unique()


def _stft_draw(case, seed):
    n, hop, wl, L, regime = case
    g = _gen("stft", case, seed)
    c = types.SimpleNamespace(case=case, n=n, hop=hop, wl=wl, L=L, regime=regime, B=STFT_B, F=1 + L // hop,
                              left=(n - wl) // 2, seed=seed)
    c.x, c.y = AMP * _rn(g, c.B, L), AMP * _rn(g, c.B, L)
    # the stretch: the support of a middle frame in signal 0, of frame 0 (the left reflection) in signal 1
    c.stretch = [frame_support(n, hop, wl, L, c.F // 2), frame_support(n, hop, wl, L, 0)]
    for b, s in enumerate(c.stretch):
        if regime in ("silence_y", "silence_xy"):
            c.y[b, s] = 0.0
        if regime in ("silence_x", "silence_xy"):
            c.x[b, s] = 0.0
        if regime == "equal_bins":
            c.x[b, s] = c.y[b, s]
        if regime == "faint":
            c.x[b, s], c.y[b, s] = 1e-6 * _rn(g, s.numel()), 1e-3 * _rn(g, s.numel())
    if regime == "identical":
        c.x = c.y.clone()
    c.gmag = _rn(g, c.B, c.F, n // 2 + 1)
    c.coef = torch.tensor([0.37, 2.3e-3]) * (0.5 + torch.rand(2, generator=g))
    return c


def stft_conditions(c):
    """the floor and sign conditions of the module docstring; returns the list of violations ([] = the case qualifies)"""
    r, bad = c.ref64, []
    for s, (re, im) in (("X", ("xre", "xim")), ("Y", ("yre", "yim"))):
        mag = torch.sqrt(r[re] ** 2 + r[im] ** 2)
        d = torch.zeros_like(mag[..., :1])
        for o in (c.o_dft, c.o_fft):
            d = torch.maximum(d, torch.sqrt(((o[re].double() - r[re]) ** 2 + (o[im].double() - r[im]) ** 2).mean(-1, keepdim=True)))
        setattr(c, "d" + s, d)
        setattr(c, "abs" + s, mag)
        if s == "X":
            ok = (mag == 0) | ((mag - R.FLOOR ** 0.5).abs() > MARGIN * d)
            if not bool(ok.all()):
                bad.append("floor: %d bins" % int((~ok).sum()))
    onx, ony = c.absX ** 2 > R.FLOOR, c.absY ** 2 > R.FLOOR
    ddl = torch.where(onx, c.dX / r["xmag"], 0.0) + torch.where(ony, c.dY / r["ymag"], 0.0)
    ok = (r["dl"] == 0) | (r["dl"].abs() > MARGIN * ddl)
    if not bool(ok.all()):
        bad.append("sign: %d bins" % int((~ok).sum()))
    for k in STABLE_OUT:
        try:
            CR.close(c.o_fft[k], r[k], c.o_dft[k], k)
        except AssertionError as e:
            bad.append("stable: %s" % e)
    c.min_floor = float(((c.absX - R.FLOOR ** 0.5).abs() / (MARGIN * c.dX + 1e-300))[c.absX > 0].min()) if bool((c.absX > 0).any()) else float("inf")
    nz = r["dl"] != 0
    c.min_sign = float((r["dl"].abs() / (MARGIN * ddl + 1e-300))[nz].min()) if bool(nz.any()) else float("inf")
    return bad


def _stft_refs(c):
    kw = dict(coef=c.coef, gmag=c.gmag)
    c.ref64 = R.stft_all(c.x, c.y, c.n, c.hop, c.wl, f64, "dft", **kw)
    c.o_dft = R.stft_all(c.x, c.y, c.n, c.hop, c.wl, torch.float32, "dft", **kw)
    c.o_fft = R.stft_all(c.x, c.y, c.n, c.hop, c.wl, torch.float32, "fft", **kw)
    for o in (c.ref64, c.o_dft, c.o_fft):
        o["fused_gx"] = c.coef[0].to(o["g_sc"].dtype) * o["g_sc"] + c.coef[1].to(o["g_sc"].dtype) * o["g_mag"]
    c.yard = {k: R.yardstick(c.ref64[k], c.o_dft[k], c.o_fft[k]) for k in STFT_OUT}


@functools.lru_cache(maxsize=None)
def stft_inputs(case):
    """cached: shared between tests, left unchanged"""
    tried = []
    for seed in SEEDS:
        c = _stft_draw(case, seed)
        _stft_refs(c)
        bad = stft_conditions(c)
        if not bad:
            # the reference alone decides: both fp32 orders take every branch the way float64 does
            for o in (c.o_dft, c.o_fft):
                assert torch.equal(o["px"] > R.FLOOR, c.ref64["px"] > R.FLOOR), case
                assert torch.equal(torch.sign(o["dl"]).double(), torch.sign(c.ref64["dl"])), case
            return c
        tried.append("seed %d: %s" % (seed, ", ".join(bad)))
    raise AssertionError("%s: no seed of %s meets the generator's conditions\n%s" % (stft_id(case), SEEDS, "\n".join(tried)))


def stft_gpu(c):
    """the five STFT entry points and, on fwdgrad's own tables, trunet_loss_grad_gather with one resolution
    (audio == clean: the L1 term is exactly 0; g_loss = 1; vals[5], vals[6] = coef) -> fused_gx"""
    Lb, lib = _lib()
    s = Sent()
    n, hop, wl, L, B, F = c.n, c.hop, c.wl, c.L, c.B, c.F
    x, y = s.put(c.x), s.put(c.y)
    win = s.put(R.window(n, wl, torch.float32)[0])
    tw = _tw(n)
    gmag, coef = s.put(c.gmag), s.put(c.coef, tail=16)
    o = {"xmag": s.out(B, F, n // 2 + 1), "ymag": s.out(B, F, n // 2 + 1), "partials": s.out(B * F, 3),
         "partials_fg": s.out(B * F, 3), "fr_sc": s.out(B, F, wl), "fr_mag": s.out(B, F, wl), "bwd_frames": s.out(B, F, wl),
         "bwd_gx": s.out(B, L), "magbwd_frames": s.out(B, F, wl), "magbwd_gx": s.out(B, L), "fused_gx": s.out(B, L)}
    p, st = Lb.ptr, Lb.stream()
    Lb.check(lib.trunet_stft_mag(p(x), p(y), p(win), p(tw), p(o["xmag"]), p(o["ymag"]), B, L, n, hop, st), "stft_mag")
    Lb.check(lib.trunet_stft_mag_bwd(p(x), p(win), p(tw), p(gmag), p(o["magbwd_frames"]), p(o["magbwd_gx"]), B, L, n, hop, wl,
                                     st), "stft_mag_bwd")
    Lb.check(lib.trunet_stft_loss_fwd(p(x), p(y), p(win), p(tw), p(o["partials"]), B, L, n, hop, st), "stft_loss_fwd")
    Lb.check(lib.trunet_stft_loss_fwdgrad(p(x), p(y), p(win), p(tw), p(o["partials_fg"]), p(o["fr_sc"]), p(o["fr_mag"]), B, L,
                                          n, hop, wl, st), "stft_loss_fwdgrad")
    Lb.check(lib.trunet_stft_loss_bwd_gather(p(x), p(y), p(win), p(tw), p(coef), p(o["bwd_frames"]), p(o["bwd_gx"]), B, L, n,
                                             hop, wl, st), "stft_loss_bwd_gather")
    vals = s.put(torch.cat([torch.zeros(5), c.coef]), tail=16)
    one = s.put(torch.ones(1), tail=16)
    a = Lb.LossGatherArgs()
    a.nres = 1
    a.fr_sc[0], a.fr_mag[0], a.n[0], a.hop[0], a.win_length[0] = p(o["fr_sc"]), p(o["fr_mag"]), n, hop, wl
    Lb.check(lib.trunet_loss_grad_gather(a, p(x), p(x), p(vals), p(one), p(o["fused_gx"]), B, L, st), "loss_grad_gather")
    s.check(stft_id(c.case))
    return _cpu(o)


def stft_emul(c, mut=None):
    if mut is None:
        o = {k: c.ref64[k].float() for k in STFT_OUT}
    else:
        r = R.stft_all(c.x, c.y, c.n, c.hop, c.wl, f64, "dft", mut, coef=c.coef, gmag=c.gmag)
        cs, cm = (c.coef[1], c.coef[0]) if mut == "coef_swapped" else (c.coef[0], c.coef[1])
        r["fused_gx"] = cs.double() * r["g_sc"] + cm.double() * r["g_mag"]
        o = {k: r[k].float() for k in STFT_OUT}
    o["partials_fg"] = o["partials"].clone()
    return o


def judge_stft(c, got, quiet=False):
    j = Judge("STFT " + stft_id(c.case), quiet)
    for k in STFT_OUT:
        j.close(k, got[k], c.ref64[k], c.yard[k])
    # the kernel comment's promise: the same reductions in the same order
    j.exact(got["partials_fg"].shape == got["partials"].shape and
            torch.equal(got["partials_fg"].view(torch.int32), got["partials"].view(torch.int32)),
            "stft_loss_fwdgrad's partials are not bit-equal to stft_loss_fwd's")
    if c.regime == "identical" and tuple(got["partials"].shape) == (c.B * c.F, 3):
        j.exact(bool((got["partials"][:, 0] == 0).all()) and bool((got["partials"][:, 2] == 0).all()),
                "x == y: S1 / S3 partial sums are not exactly 0")
        for k in ("fr_sc", "fr_mag", "bwd_gx", "fused_gx"):
            j.exact(bool((got[k] == 0).all()), "x == y: %s is not exactly 0" % k)
    j.done()


# ============================================================================================== the gradient gather
GATHER_L = 1100            # > 2048 / 2; 1100 % 256 != 0; L % hop == 0 for hop 50, != 0 for the others
GATHER_RES = ((1024, 120, 601), (8, 3, 5), (2048, 240, 1200), (512, 50, 240), (128, 40, 30), (512, 128, 512), (64, 16, 64),
              (1024, 120, 600))
GATHER_CASES = (0, 1, 3, 8)
GATHER_B = 2
GATHER_EQ = (100, 200)      # audio == clean on this stretch: an exactly zero L1 term


def gather_inputs(nres):
    return _gather_inputs(nres)


@functools.lru_cache(maxsize=None)
def _gather_inputs(nres):
    g = _gen("gather", nres)
    B, L = GATHER_B, GATHER_L
    c = types.SimpleNamespace(case=nres, nres=nres, B=B, L=L, g_loss=2.5)
    c.audio, c.clean = AMP * _rn(g, B, L), AMP * _rn(g, B, L)
    c.clean[:, GATHER_EQ[0]:GATHER_EQ[1]] = c.audio[:, GATHER_EQ[0]:GATHER_EQ[1]]
    c.res = [(_rn(g, B, 1 + L // hop, wl), _rn(g, B, 1 + L // hop, wl), n, hop, wl) for n, hop, wl in GATHER_RES[:nres]]
    c.vals = _rn(g, 5 + 2 * nres)
    c.vals[4] = 1.0 / (B * L)
    # the l1 condition: an fp32 difference has the sign of the exact difference
    assert torch.equal(torch.sign(c.audio - c.clean).double(), torch.sign(c.audio.double() - c.clean.double()))
    c.ref64 = R.loss_grad_gather(c.res, c.audio, c.clean, c.vals, c.g_loss)
    a, b = (R.loss_grad_gather(c.res, c.audio, c.clean, c.vals, c.g_loss, torch.float32, o) for o in ("dft", "fft"))
    c.yard = R.yardstick(c.ref64, a, b)
    return c


def gather_gpu(c):
    Lb, lib = _lib()
    s = Sent()
    audio, clean, vals = s.put(c.audio), s.put(c.clean), s.put(c.vals, tail=16)
    gl = s.put(torch.tensor([c.g_loss]), tail=16)
    out = s.out(c.B, c.L)
    a = Lb.LossGatherArgs()
    a.nres = c.nres
    keep = []
    for i, (fs, fm, n, hop, wl) in enumerate(c.res):
        keep += [s.put(fs), s.put(fm)]
        a.fr_sc[i], a.fr_mag[i], a.n[i], a.hop[i], a.win_length[i] = Lb.ptr(keep[-2]), Lb.ptr(keep[-1]), n, hop, wl
    Lb.check(lib.trunet_loss_grad_gather(a, Lb.ptr(audio), Lb.ptr(clean), Lb.ptr(vals), Lb.ptr(gl), Lb.ptr(out), c.B, c.L,
                                         Lb.stream()), "loss_grad_gather")
    s.check("gather nres %d" % c.nres)
    return _cpu({"g_audio": out})


def gather_emul(c, mut=None):
    return {"g_audio": R.loss_grad_gather(c.res, c.audio, c.clean, c.vals, c.g_loss, mut=mut).float()}


def judge_gather(c, got, quiet=False):
    j = Judge("LOSS-GRAD-GATHER nres%d" % c.nres, quiet)
    j.close("g_audio", got["g_audio"], c.ref64, c.yard)
    if c.nres == 0:
        j.exact(bool((got["g_audio"][:, GATHER_EQ[0]:GATHER_EQ[1]] == 0).all()), "audio == clean: the L1 term is not exactly 0")
    j.done()


# ============================================================================================== mask + iSTFT
MASK_T = (2, 3, 4, 5, 9)       # the envelope limited by T (2, 3), the first interior sample (4, 5), many blocks (9); L = 128 odd: 2, 4
MASK_REGIMES = ("generic", "c0_edge", "zero_pairs", "neg_axis")
MASK_B = 3
MASK_CASES = [(T, beta, clean, r) for iT, T in enumerate(MASK_T) for iR, r in enumerate(MASK_REGIMES)
              for beta, clean in (((0.5, 1), (2.0, 0)) if (iT + iR) % 2 == 0 else ((2.0, 1), (0.5, 0)))]


def mask_id(case):
    return "T%d-beta%.1f-clean%d-%s" % case


@functools.lru_cache(maxsize=None)
def mask_inputs(case):
    T, beta, with_clean, regime = case
    g = _gen("mask", case)
    B, L = MASK_B, R.HOPF * (T - 1)
    c = types.SimpleNamespace(case=case, T=T, beta=beta, regime=regime, B=B, L=L, with_clean=bool(with_clean))
    o = 0.7 * _rn(g, B * T, 8, R.BINS)
    pick = torch.rand(B * T, R.BINS, generator=g)
    if regime == "c0_edge":
        for lo, v in ((0.0, 1.0), (0.2, -1.0), (0.4, 1.7), (0.5, -2.3)):            # exactly +-1, and beyond
            o[:, 0][(pick >= lo) & (pick < lo + 0.1 + 0.1 * (v in (1.0, -1.0)))] = v
    elif regime == "zero_pairs":
        for lo, chans in ((0.0, (2, 3)), (0.1, (6, 7)), (0.2, (2, 3, 6, 7))):       # mixture, noise, both
            for ch in chans:
                o[:, ch][(pick >= lo) & (pick < lo + 0.1)] = 0.0
    elif regime == "neg_axis":
        for lo, (s, cch), z in ((0.0, (2, 3), 0.0), (0.1, (2, 3), -0.0), (0.2, (6, 7), 0.0), (0.3, (6, 7), -0.0)):
            m = (pick >= lo) & (pick < lo + 0.1)
            o[:, s][m] = z                                                          # sin = +0 / -0: the angle is +pi / -pi
            o[:, cch][m] = -o[:, cch][m].abs() - 0.05
    # DC and Nyquist of every frame: a large mask with a phase well off the real axis, so that the imaginary part the
    # transform must drop -- and the weight these two bins get in the backward -- is far above any tolerance
    for k in (0, R.NF // 2):
        o[:, 0, k], o[:, 2, k], o[:, 3, k], o[:, 6, k], o[:, 7, k] = 0.9, 1.0, 0.2, 0.3, 1.0
    c.net_out = o
    c.clean = AMP * _rn(g, B, L) if with_clean else None
    c.g_audio = _rn(g, B, L)
    c.nparts = B * (-(-L // 256))
    kw = dict(clean=c.clean)
    c.ref64 = R.mask_istft_fwd(o, T, beta, dtype=f64, **kw)
    fa, fb = (R.mask_istft_fwd(o, T, beta, dtype=torch.float32, order=od, **kw) for od in ("dft", "fft"))
    c.ref64["g_net"] = R.mask_istft_bwd(c.g_audio, o, T, beta)
    fa["g_net"], fb["g_net"] = (R.mask_istft_bwd(c.g_audio, o, T, beta, torch.float32, od) for od in ("dft", "fft"))
    c.yard = {k: R.yardstick(c.ref64[k], fa[k], fb[k]) for k in c.ref64}
    return c


def mask_gpu(c):
    Lb, lib = _lib()
    s = Sent()
    B, T, L = c.B, c.T, c.L
    assert lib.trunet_mask_istft_l1_nparts(B, L) == c.nparts
    net, tw = s.put(c.net_out), _tw(R.NF)
    o = {"frames": s.out(B, T, R.NF), "audio": s.out(B, L), "g_net": s.out(B * T, 8, R.BINS)}
    clean = l1 = None
    if c.with_clean:
        clean, l1 = s.put(c.clean), s.out(c.nparts, tail=64)
        o["l1"] = l1
    ga = s.put(c.g_audio)
    p = Lb.ptr
    Lb.check(lib.trunet_mask_istft_fwd(p(net), p(o["frames"]), p(o["audio"]), p(clean), p(l1), p(tw), B, T, L, c.beta,
                                       Lb.stream()), "mask_istft_fwd")
    Lb.check(lib.trunet_mask_istft_bwd(p(ga), p(net), p(o["g_net"]), p(tw), B, T, L, c.beta, Lb.stream()), "mask_istft_bwd")
    s.check(mask_id(c.case))
    return _cpu(o)


def mask_emul(c, mut=None):
    o = R.mask_istft_fwd(c.net_out, c.T, c.beta, clean=c.clean, mut=mut)
    o["g_net"] = R.mask_istft_bwd(c.g_audio, c.net_out, c.T, c.beta, mut=mut)
    return {k: v.float() for k, v in o.items()}


def judge_mask(c, got, quiet=False):
    j = Judge("MASK-ISTFT " + mask_id(c.case), quiet)
    for k in c.ref64:
        j.close(k, got[k], c.ref64[k], c.yard[k])
    if "g_net" in got and got["g_net"].shape == c.net_out.shape:
        g, o = got["g_net"], c.net_out
        j.exact(bool((g[:, [1, 4, 5]] == 0).all()), "channels 1, 4, 5 have a gradient")
        zm, zn = (o[:, 2] == 0) & (o[:, 3] == 0), (o[:, 6] == 0) & (o[:, 7] == 0)
        j.exact(bool((g[:, 2][zm] == 0).all()) and bool((g[:, 3][zm] == 0).all()), "a zero mixture phase pair has a gradient")
        j.exact(bool((g[:, 6][zn] == 0).all()) and bool((g[:, 7][zn] == 0).all()), "a zero noise phase pair has a gradient")
        j.exact(bool((g[:, 0][(o[:, 0] < -1) | (o[:, 0] > 1)] == 0).all()), "a clamped c0 has a gradient")
    j.done()


# ============================================================================================== reduce_cols / loss_finalize / l1_grad
ROWS = (1, 1023, 1024, 1025, 4096, 4097, 8197)          # the 4096-row main loop against its tail loop
RC_CASES = [(r, nc) for r in ROWS for nc in (1, 3)]


def rc_inputs(case):
    rows, ncols = case
    c = types.SimpleNamespace(case=case, rows=rows, ncols=ncols, parts=_rn(_gen("rc", case), rows, ncols))
    c.ref64 = R.reduce_cols(c.parts)
    return c


def rc_gpu(c):
    Lb, lib = _lib()
    s = Sent()
    parts, out = s.put(c.parts), s.out(c.ncols, tail=16)
    Lb.check(lib.trunet_reduce_cols(Lb.ptr(parts), c.rows, c.ncols, Lb.ptr(out), Lb.stream()), "reduce_cols")
    s.check("reduce_cols %s" % (c.case,))
    return _cpu({"out": out, "parts": parts})


def rc_emul(c, mut=None):
    return {"out": c.ref64.float(), "parts": c.parts.clone()}


def judge_rc(c, got, quiet=False):
    j = Judge("REDUCE-COLS rows%d-cols%d" % c.case, quiet)
    j.within("out", got["out"], c.ref64, 2 * U * c.ref64.abs() + D * c.parts.double().abs().sum(0))      # one rounding
    j.exact(torch.equal(got["parts"], c.parts), "the partial table was modified")
    j.done()


# (rows of the L1 column, nres, stft_lambda, zero_s1): resolution i has max(1, rows - 17 i) rows
FIN_CASES = [(r, (0, 1, 3, 8)[i % 4], 1.0, 0) for i, r in enumerate(ROWS)] + \
            [(1025, 3, 0.0, 0), (4097, 8, 0.7, 0), (8197, 1, 1.0, 0), (1024, 3, 1.0, 1), (1, 8, 0.7, 1)]
SC_LAMBDA, MAG_LAMBDA = 0.3, 0.8          # different on purpose: a swap shows


def fin_id(case):
    return "rows%d-nres%d-lam%.1f-zero%d" % case


def fin_inputs(case):
    rows, nres, lam, zero_s1 = case
    g = _gen("fin", case)
    c = types.SimpleNamespace(case=case, rows=rows, nres=nres, lam=lam, zero_s1=zero_s1)
    c.l1p = torch.rand(rows, generator=g) * 20.0
    c.l1_count = float(rows * 256 - 7)
    c.parts = [torch.rand(max(1, rows - 17 * i), 3, generator=g) * torch.tensor([3.0, 40.0, 900.0]) for i in range(nres)]
    c.counts = [float(p.shape[0] * (257 + 256 * (i % 3))) for i, p in enumerate(c.parts)]
    if zero_s1:
        c.parts[nres // 2][:, 0] = 0.0        # the prediction equals the target in every bin of this resolution
        c.parts[nres // 2][:, 2] = 0.0
    c.ref64 = R.loss_finalize(c.l1p, c.l1_count, c.parts, c.counts, SC_LAMBDA, MAG_LAMBDA, lam)
    return c


def fin_gpu(c):
    """two launches on ONE scratch buffer (zero before the first): vals, loss_out and the scratch after each"""
    import ctypes
    Lb, lib = _lib()
    s = Sent()
    nb = lib.trunet_loss_scratch_bytes()
    assert nb % 4 == 0
    scratch = s.put(torch.zeros(nb // 4), tail=16)
    a = Lb.LossArgs()
    l1p = s.put(c.l1p, tail=16)
    a.l1_partials, a.n_l1, a.nres, a.l1_count = Lb.ptr(l1p), c.rows, c.nres, c.l1_count
    a.sc_lambda, a.mag_lambda, a.stft_lambda = SC_LAMBDA, MAG_LAMBDA, c.lam
    keep = []
    for i, pt in enumerate(c.parts):
        keep.append(s.put(pt))
        a.parts[i], a.nrows[i], a.count[i] = Lb.ptr(keep[-1]), pt.shape[0], c.counts[i]
    got = {}
    for run in (1, 2):
        vals, loss = s.out(5 + 2 * c.nres, tail=16), s.out(1, tail=16)
        Lb.check(lib.trunet_loss_finalize(ctypes.byref(a), Lb.ptr(loss), Lb.ptr(vals), scratch.data_ptr(), Lb.stream()),
                 "loss_finalize")
        torch.cuda.synchronize()
        got["vals%d" % run], got["loss%d" % run], got["scratch%d" % run] = vals.cpu(), loss.cpu(), scratch.cpu()
    s.check("loss_finalize " + fin_id(c.case))
    return got


def fin_emul(c, mut=None):
    v = c.ref64.float()
    z = torch.zeros(17 * 2)
    return {"vals1": v, "vals2": v.clone(), "loss1": v[:1].clone(), "loss2": v[:1].clone(), "scratch1": z, "scratch2": z.clone()}


def judge_fin(c, got, quiet=False):
    """the counted roundings of tests/losstail_ref.py's docstring"""
    j = Judge("LOSS-FINALIZE " + fin_id(c.case), quiet)
    r = c.ref64
    bnd = torch.zeros_like(r)
    bnd[0] = 12 * U * (r[1].abs() + r[2].abs() + r[3].abs())
    bnd[1] = 2 * U * r[1].abs() + D * float(c.l1p.double().abs().sum()) / c.l1_count
    bnd[2], bnd[3], bnd[4] = 9 * U * r[2].abs(), 8 * U * r[3].abs(), 2 * U * r[4].abs()
    for i in range(c.nres):
        bnd[5 + 2 * i], bnd[6 + 2 * i] = 8 * U * r[5 + 2 * i].abs(), 5 * U * r[6 + 2 * i].abs()
    j.within("vals", got["vals1"], r, bnd)
    j.exact(torch.equal(got["loss1"], got["vals1"][:1]), "loss_out differs from vals[0]")
    if c.zero_s1:
        j.exact(float(got["vals1"][5 + 2 * (c.nres // 2)]) == 0.0, "S1 == 0: c_sc is not exactly 0")
    j.exact(torch.equal(got["vals1"].view(torch.int32), got["vals2"].view(torch.int32)) and torch.equal(got["loss1"], got["loss2"]),
            "the second launch on the same scratch gives other bits")
    for run in (1, 2):
        j.exact(BC.is_pos_zero(got["scratch%d" % run]), "the scratch buffer is not all zero after launch %d" % run)
    j.done()


L1_N = (1, 255, 256, 257, 1100)
L1_SCALE = 0.37


def l1_inputs(n):
    g = _gen("l1", n)
    c = types.SimpleNamespace(case=n, n=n, den=AMP * _rn(g, n), clean=AMP * _rn(g, n))
    c.clean[n // 3:n // 2 + 1] = c.den[n // 3:n // 2 + 1]
    assert torch.equal(torch.sign(c.den - c.clean).double(), torch.sign(c.den.double() - c.clean.double()))
    c.want = R.l1_grad(c.den, c.clean, torch.tensor(L1_SCALE))
    return c


def l1_gpu(c):
    Lb, lib = _lib()
    s = Sent()
    den, clean, scale, out = s.put(c.den, tail=16), s.put(c.clean, tail=16), s.put(torch.tensor([L1_SCALE]), tail=16), s.out(c.n, tail=64)
    Lb.check(lib.trunet_l1_grad(Lb.ptr(den), Lb.ptr(clean), Lb.ptr(scale), Lb.ptr(out), c.n, Lb.stream()), "l1_grad")
    s.check("l1_grad %d" % c.n)
    return _cpu({"g": out})


def l1_emul(c, mut=None):
    return {"g": c.want.clone()}


def judge_l1(c, got, quiet=False):
    j = Judge("L1-GRAD n%d" % c.n, quiet)
    j.bits("g", got["g"], c.want)
    j.exact(bool((got["g"][c.n // 3:c.n // 2 + 1] == 0).all()), "den == clean: the gradient is not 0")
    j.done()


# ============================================================================================== x == y through the fused chain
IDENT_L = 1100
IDENT_RES = ((512, 50, 240), (1024, 120, 600), (2048, 240, 1200))       # the workload's three resolutions


def identical_chain_gpu():
    """x == y everywhere: trunet_stft_loss_fwdgrad per resolution -> trunet_loss_finalize -> trunet_loss_grad_gather with
    audio == clean.  Returns {vals, g_audio}."""
    import ctypes
    Lb, lib = _lib()
    s = Sent()
    B, L = 2, IDENT_L
    xc = AMP * _rn(_gen("identical"), B, L)
    x, y = s.put(xc), s.put(xc.clone())
    a, ga = Lb.LossArgs(), Lb.LossGatherArgs()
    nb = -(-L // 256)
    l1p = s.put(torch.zeros(B * nb), tail=16)                          # audio == clean: every |audio - clean| block sum is 0
    a.l1_partials, a.n_l1, a.nres, a.l1_count = Lb.ptr(l1p), B * nb, len(IDENT_RES), float(B * L)
    a.sc_lambda, a.mag_lambda, a.stft_lambda = 0.5, 0.5, 1.0
    ga.nres = len(IDENT_RES)
    keep = []
    for i, (n, hop, wl) in enumerate(IDENT_RES):
        F = 1 + L // hop
        win = s.put(R.window(n, wl, torch.float32)[0])
        part, fs, fm = s.out(B * F, 3), s.out(B, F, wl), s.out(B, F, wl)
        keep += [win, part, fs, fm]
        Lb.check(lib.trunet_stft_loss_fwdgrad(Lb.ptr(x), Lb.ptr(y), Lb.ptr(win), Lb.ptr(_tw(n)), Lb.ptr(part), Lb.ptr(fs),
                                              Lb.ptr(fm), B, L, n, hop, wl, Lb.stream()), "stft_loss_fwdgrad")
        a.parts[i], a.nrows[i], a.count[i] = Lb.ptr(part), B * F, float(B * F * (n // 2 + 1))
        ga.fr_sc[i], ga.fr_mag[i], ga.n[i], ga.hop[i], ga.win_length[i] = Lb.ptr(fs), Lb.ptr(fm), n, hop, wl
    scratch = s.put(torch.zeros(lib.trunet_loss_scratch_bytes() // 4), tail=16)
    vals, loss, g = s.out(5 + 2 * len(IDENT_RES), tail=16), s.out(1, tail=16), s.out(B, L)
    one = s.put(torch.tensor([2.5]), tail=16)
    Lb.check(lib.trunet_loss_finalize(ctypes.byref(a), Lb.ptr(loss), Lb.ptr(vals), scratch.data_ptr(), Lb.stream()), "loss_finalize")
    Lb.check(lib.trunet_loss_grad_gather(ga, Lb.ptr(x), Lb.ptr(y), Lb.ptr(vals), Lb.ptr(one), Lb.ptr(g), B, L, Lb.stream()),
             "loss_grad_gather")
    s.check("identical chain")
    return _cpu({"vals": vals, "g_audio": g, "loss": loss})
