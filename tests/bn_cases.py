"""The BatchNorm statistics chain and the block-boundary kernels through the C ABI against tests/bn_ref.py: seeded inputs,
launches, the comparison, and the report lines of tests/test_bn_chain_gpu.py.  tests/test_bn_ref_cpu.py feeds the same
`judge_*` functions with the restatement (and with its mutants) in place of kernel output.

Every family has  *_inputs(case) -> c,  *_gpu(c) -> got,  *_emul(c, mut) -> got (no GPU),  judge_*(c, got).

Launch hygiene: every output is prefilled with NaN, every per-channel vector and every partial image has a sentinel row
behind it, and `Sent.check` asserts after each launch that no sentinel moved.

Tolerances (U = 2^-24, D = 2^-50), derived, never tuned:
  one rounding   an output that is ONE fp32 rounding of a double expression (mean, rstd, dgamma, dbeta, ca, cb, cc,
                 reduce_partials with accumulate = 0, sumsq), against the same expression in float64 of the same fp32
                 inputs: 2 U |ref| + D sum|terms|.  U |ref| is the rounding (the factor 2 is all the slack there is);
                 D sum|terms| is the evaluation order of the double expression (hipcc contracts to fma, the sums run
                 over 256 threads and a tree), carried through the expression where it is not the last operation.
  fp32 arithmetic  (scale, shift, running statistics, eval_affine, the affine copy, reduce_partials with accumulate = 1):
                 (r + 1) U sum|terms of the final expression|, r the number of fp32 roundings of the kernel's formula,
                 listed next to each use (plain -O3, no fast-math: sqrt and divide are one rounding each).
  conditioning   the statistics against float64 of the DATA: the producers hand over fp32 partial sums, so
                 |var - var64| <= Bv = U (sum_g|p_sumsq,g| + 2 |mean| sum_g|p_sum,g|) / count, |mean - mean64| <= U sum_g|p_sum,g|
                 / count + U |mean|, and carried into rstd: relative 1/2 Bv / (var64 + eps) + U; a factor 2 on the whole for the
                 second-order terms.
  summation      relu_bwd_stats sums, conv_first, the chain's dz / dgamma / dbeta: convt_ref.close, the yardstick measured
                 on the same inputs."""
import functools
import hashlib
import os
import sys
import types

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bn_ref as R  # noqa: E402
import convt_ref as CR  # noqa: E402

U, D = 2.0 ** -24, 2.0 ** -50
SENT = 7.5
EPS = 1e-5
NAN = float("nan")
f64 = torch.float64


def _gen(*key):
    return torch.Generator().manual_seed(int(hashlib.sha1(repr(key).encode()).hexdigest()[:8], 16))


def _rn(g, *s):
    return torch.randn(*s, generator=g, dtype=torch.float32)


def _un(g, lo, hi, *s):
    return lo + (hi - lo) * torch.rand(*s, generator=g, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------- report and comparison
def report(line):
    """one line per case, through the writer the other per-kernel pins use: printed, and appended to parity_bn.txt in the
    directory TRUNET_PARITY_DIR names"""
    from convt_cases import report as write
    write(line, "parity_bn.txt")


class Judge:
    """collects every figure of a case BEFORE the first assertion fires; done() prints the line and asserts"""

    def __init__(self, tag, quiet=False):
        self.tag, self.figs, self.fails, self.quiet = tag, [], [], quiet

    def within(self, name, got, ref64, bnd):
        """element by element |got - ref64| <= bnd (a derived bound, tensor or number); every element finite"""
        got, ref64 = got.detach().cpu().double(), ref64.detach().cpu().double()
        bnd = torch.as_tensor(bnd, dtype=f64).expand_as(ref64)
        if got.shape != ref64.shape or not bool(torch.isfinite(got).all()):
            self.fails.append("%s %s: shape %s / not finite" % (self.tag, name, tuple(got.shape)))
            return
        err = (got - ref64).abs()
        worst = int((err / (bnd + 1e-300)).argmax()) if err.numel() else 0          # the element that uses most of its bound
        e, b = float(err.flatten()[worst]), float(bnd.flatten()[worst])
        self.figs.append("%s %.2e/-/%.2e" % (name, e, b))
        if not bool((err <= bnd).all()):
            self.fails.append("%s %s: error %.3e > bound %.3e at %d" % (self.tag, name, e, b, worst))

    def close(self, name, got, ref64, yard):
        """convt_ref.close: max error <= 4 e_y + 8 U max|ref|, relative L2 <= 4 rel_y + 1e-6"""
        got, ref64, yard = got.detach().cpu(), ref64.detach().cpu(), yard.detach().cpu()
        e_y, bnd = CR.bound(ref64, yard)[:2]
        err = float((got.double() - ref64).abs().max()) if bool(torch.isfinite(got).all()) else NAN
        self.figs.append("%s %.2e/%.2e/%.2e" % (name, err, e_y, bnd))
        try:
            CR.close(got, ref64, yard, "%s %s" % (self.tag, name))
        except AssertionError as e:
            self.fails.append(str(e))

    def exact(self, cond, msg):
        if not bool(cond):
            self.fails.append("%s: %s" % (self.tag, msg))

    def done(self):
        if not self.quiet:
            report("%s: kernel error / e_y / bound  %s" % (self.tag, "  ".join(self.figs)))
        assert not self.fails, "\n".join(self.fails)


def rejected(judge_fn, c, got):
    """the failure messages judge_fn raises for `got` ([] where it passes)"""
    try:
        judge_fn(c, got, quiet=True)
    except AssertionError as e:
        return str(e).split("\n")
    return []


def worse(ref64, a, b):
    """element by element the fp32 result further from the reference"""
    return torch.where((b.double() - ref64).abs() > (a.double() - ref64).abs(), b, a)


def is_pos_zero(t):
    return bool((t.contiguous().view(torch.int32) == 0).all())


# ---------------------------------------------------------------------------------------------- device buffers
class Sent:
    """device buffers with a sentinel row behind them"""

    def __init__(self):
        self.bufs = []

    def put(self, t, tail=None):
        """t (CPU fp32, any shape) -> device tensor of t's shape, a sentinel row (one slice along axis 0; `tail` elements
        for a flat tensor) right behind it in the same allocation"""
        t = t.contiguous()
        row = t[0].numel() if t.dim() > 1 else 1
        n_tail = tail if tail is not None else row
        flat = torch.cat([t.reshape(-1), torch.full((n_tail,), SENT)]).cuda()
        self.bufs.append((flat, t.numel()))
        return flat[:t.numel()].view(t.shape)

    def out(self, *shape, tail=None):
        return self.put(torch.full(shape, NAN), tail)

    def check(self, what):
        torch.cuda.synchronize()
        for flat, n in self.bufs:
            assert bool((flat[n:] == SENT).all()), "%s: a sentinel behind a %d-element buffer was overwritten" % (what, n)


def _lib():
    from tinyrecurrentunet_amd import _lib as Lb
    return Lb, Lb.lib()


# ============================================================================================== finalize_fwd / finalize_bwd
NPARTS = (1, 16, 255, 256, 257, 600)          # the kernels stride the part rows by 256
FIN_C = (1, 24, 192)
COUNTS = (13.0 * 130.0, 1.0, 2.0 ** 24 + 3.0)  # a non-power of two; 1 (torch refuses it); beyond fp32's integers (synthetic)
NBT0 = 41


# (running statistics, counter, momentum): NULL and non-NULL crossed in full; the momentum matters with running statistics only
FIN_FLAGS = ((False, False, 0.1), (False, True, 0.1), (True, False, 0.1), (True, False, 1.0), (True, True, 0.1), (True, True, 1.0))


def fin_cases():
    """(nparts, C, count, running, counter, momentum): nparts x C x count x FIN_FLAGS, the full cross -- running_var's
    unbiased branch (count > 1) and its count == 1 branch both run with every nparts and C, with and without the counter"""
    return [(nparts, Cn, count) + fl for nparts in NPARTS for Cn in FIN_C for count in COUNTS for fl in FIN_FLAGS]


FIN_CASES = fin_cases()
# trunet_bn_finalize_bwd has no such flags: one launch per (nparts, C, count)
FIN_BWD_CASES = [c for c in FIN_CASES if c[3:] == FIN_FLAGS[0]]


def fin_id(case):
    return "g%d-C%d-n%g-run%d-nbt%d-m%g" % case


@functools.lru_cache(maxsize=None)
def fin_inputs(case):
    """synthetic partial images.  fwd: part g holds count / nparts `elements` of mean mu_c + noise and second moment
    mu_c^2 + 1 + noise (variance about 1, channel 0 of C >= 24 offset to mean 3); bwd: sums of a cotangent"""
    nparts, Cn, count, running, counter, mom = case
    g = _gen("fin", case)
    c = types.SimpleNamespace(case=case, nparts=nparts, C=Cn, count=count, running=running, counter=counter, mom=mom)
    mu = 0.5 * _rn(g, Cn)
    if Cn >= 24:
        mu[0] = 3.0
    n_g = count / nparts
    c.pf = torch.stack([n_g * (mu + 0.3 * _rn(g, nparts, Cn)), n_g * (mu * mu + 1.0 + 0.3 * _un(g, 0, 1, nparts, Cn))], -1)
    c.gamma, c.beta = _un(g, 0.5, 1.5, Cn) * torch.where(_rn(g, Cn) < -0.5, -1.0, 1.0), 0.5 * _rn(g, Cn)
    c.rm, c.rv = 0.3 * _rn(g, Cn), _un(g, 0.5, 2.0, Cn)
    c.pb = torch.stack([n_g * 0.3 * _rn(g, nparts, Cn), n_g * 0.3 * _rn(g, nparts, Cn)], -1)
    c.mean, c.rstd = mu.clone(), _un(g, 0.5, 3.0, Cn)
    c.fwd64 = R.finalize_fwd(c.pf, count, c.gamma, c.beta, EPS, mom, c.rm, c.rv)
    c.bwd64 = R.finalize_bwd(c.pb, count, c.gamma, c.mean, c.rstd)
    return c


def fin_fwd_gpu(c):
    import ctypes
    Lb, lib = _lib()
    s = Sent()
    parts = s.put(c.pf)
    gam, bet = s.put(c.gamma), s.put(c.beta)
    rm, rv = (s.put(c.rm), s.put(c.rv)) if c.running else (None, None)
    o = {k: s.out(c.C) for k in ("scale", "shift", "mean", "rstd")}
    nbt = torch.tensor([NBT0, -5], dtype=torch.int64, device="cuda")
    Lb.check(lib.trunet_bn_finalize_fwd(Lb.ptr(parts), c.nparts, c.C, ctypes.c_double(c.count), Lb.ptr(gam), Lb.ptr(bet), EPS,
                                        c.mom, Lb.ptr(rm), Lb.ptr(rv), Lb.ptr(o["scale"]), Lb.ptr(o["shift"]),
                                        Lb.ptr(o["mean"]), Lb.ptr(o["rstd"]), nbt.data_ptr() if c.counter else None,
                                        Lb.stream()), "bn_finalize_fwd")
    s.check(fin_id(c.case))
    got = {k: v.cpu() for k, v in o.items()}
    got.update(parts=parts.cpu(), nbt=nbt.cpu().tolist(), running_mean=rm.cpu() if c.running else None,
               running_var=rv.cpu() if c.running else None)
    return got


def _round(d, keys):
    return {k: (d[k].float() if d[k] is not None else None) for k in keys}


def fin_fwd_emul(c, mut=None):
    """what a kernel that follows the contract returns: the double formula of the fp32 inputs, rounded once"""
    r = R.finalize_fwd(c.pf, c.count, c.gamma, c.beta, EPS, c.mom, c.rm, c.rv, mut=mut)
    got = _round(r, ("scale", "shift", "mean", "rstd", "running_mean", "running_var"))
    if not c.running:
        got["running_mean"] = got["running_var"] = None
    got.update(parts=torch.zeros_like(c.pf), nbt=[NBT0 + (1 if c.counter else 0), -5])
    return got


def judge_fin_fwd(c, got, quiet=False):
    j = Judge("BN-FIN-FWD " + fin_id(c.case), quiet)
    r, cnt, mom, eps = c.fwd64, c.count, R.f32(c.mom), R.f32(EPS)
    A0, A1 = c.pf[:, :, 0].double().abs().sum(0), c.pf[:, :, 1].double().abs().sum(0)
    g, b = c.gamma.double().abs(), c.beta.double().abs()
    mean, rstd, var = r["mean"].abs(), r["rstd"], r["var"]
    d_mean = D * A0 / cnt                                  # evaluation order of the double sums, per expression
    d_var = D * (A1 / cnt + mean * mean)
    d_rstd = 0.5 * rstd * d_var / (var + eps)
    j.exact(is_pos_zero(got["parts"]), "the consumed partial image is not exactly +0")
    j.exact(got["nbt"] == [NBT0 + (1 if c.counter else 0), -5], "counter %s" % (got["nbt"],))
    j.within("mean", got["mean"], r["mean"], 2 * U * mean + d_mean)                       # one rounding
    j.within("rstd", got["rstd"], rstd, 2 * U * rstd + d_rstd)                            # one rounding
    # scale = gamma * rstd32: r = 2 (rstd, product); term |gamma rstd|
    j.within("scale", got["scale"], r["scale"], 3 * U * g * rstd + g * d_rstd)
    # shift = beta - mean32 * scale32: r = 5 (rstd, scale, mean, product, difference); terms |beta|, |mean scale|
    j.within("shift", got["shift"], r["shift"], 6 * U * (b + mean * g * rstd) + mean * g * d_rstd + g * rstd * d_mean)
    if c.running:
        unb = var * cnt / (cnt - 1.0) if cnt > 1.0 else var
        # (1 - m) * rm + m * mean32: r = 5 (1 - m, product, mean, product, sum); terms |(1 - m) rm|, |m mean|
        j.within("run_mean", got["running_mean"], r["running_mean"],
                 6 * U * ((1 - mom) * c.rm.double().abs() + mom * mean) + mom * d_mean)
        # (1 - m) * rv + m * unb32: r = 5 (1 - m, product, unb, product, sum); terms |(1 - m) rv|, |m unb|
        j.within("run_var", got["running_var"], r["running_var"],
                 6 * U * ((1 - mom) * c.rv.double().abs() + mom * unb) + mom * d_var * (cnt / (cnt - 1.0) if cnt > 1 else 1.0))
    else:
        j.exact(got["running_mean"] is None and got["running_var"] is None, "running statistics without buffers")
    j.done()


def fin_bwd_gpu(c):
    import ctypes
    Lb, lib = _lib()
    s = Sent()
    parts = s.put(c.pb)
    gam, mean, rstd = s.put(c.gamma), s.put(c.mean), s.put(c.rstd)
    o = {k: s.out(c.C) for k in ("dgamma", "dbeta", "ca", "cb", "cc")}
    Lb.check(lib.trunet_bn_finalize_bwd(Lb.ptr(parts), c.nparts, c.C, ctypes.c_double(c.count), Lb.ptr(gam), Lb.ptr(mean),
                                        Lb.ptr(rstd), *[Lb.ptr(o[k]) for k in ("dgamma", "dbeta", "ca", "cb", "cc")],
                                        Lb.stream()), "bn_finalize_bwd")
    s.check(fin_id(c.case))
    got = {k: v.cpu() for k, v in o.items()}
    got["parts"] = parts.cpu()
    return got


def fin_bwd_emul(c, mut=None):
    got = _round(R.finalize_bwd(c.pb, c.count, c.gamma, c.mean, c.rstd, mut=mut), ("dgamma", "dbeta", "ca", "cb", "cc"))
    got["parts"] = torch.zeros_like(c.pb)
    return got


def bwd_bounds(ref, parts, count, gamma, mean, rstd):
    """one rounding each: 2 U |ref| + D sum|terms|"""
    A0, A1 = parts[:, :, 0].double().abs().sum(0), parts[:, :, 1].double().abs().sum(0)
    g, r, mu = gamma.double().abs(), rstd.double().abs(), mean.double().abs()
    terms = {"dgamma": r * A1, "dbeta": A0, "ca": g * r, "cb": g * r ** 3 * A1 / count,
             "cc": g * r * A0 / count + g * r ** 3 * mu * A1 / count}
    return {k: 2 * U * ref[k].abs() + D * terms[k] for k in terms}


def judge_fin_bwd(c, got, quiet=False):
    j = Judge("BN-FIN-BWD " + fin_id(c.case), quiet)
    j.exact(is_pos_zero(got["parts"]), "the consumed partial image is not exactly +0")
    bnd = bwd_bounds(c.bwd64, c.pb, c.count, c.gamma, c.mean, c.rstd)
    for k in ("dgamma", "dbeta", "ca", "cb", "cc"):
        j.within(k, got[k], c.bwd64[k], bnd[k])
    j.done()


# ============================================================================================== regimes of finalize_fwd
REG_CH = ("ordinary", "offset", "ill", "constant", "gamma_neg", "gamma_zero")
REG_RATIO = {"ordinary": 0.0, "offset": 5.0, "ill": 100.0, "constant": 0.0, "gamma_neg": 0.0, "gamma_zero": 0.0}
REG_CASES = ((13 * 130, 16), (16 * 255 * 8, 257))       # (count, nparts)
CONST_VALUE = 0.7


@functools.lru_cache(maxsize=None)
def reg_inputs(case):
    """one channel per regime: fp32 data x [6][count] of standard deviation about 1 (0.5 for the ill-conditioned channel)
    around |mean| / std = 0, 5, 100; the partials are the DOUBLE sums over nparts contiguous pieces, rounded to fp32 -- how
    the producing kernels hand them over"""
    count, nparts = case
    g = _gen("reg", case)
    c = types.SimpleNamespace(case=case, count=float(count), nparts=nparts, C=len(REG_CH))
    x = _rn(g, c.C, count)
    x[2] *= 0.5
    for i, k in enumerate(REG_CH):
        x[i] += REG_RATIO[k] * float(x[i].std()) * (-1.0 if i == 1 else 1.0)
    x[3] = CONST_VALUE
    c.x = x
    xd = x.double()
    edges = [(count * i) // nparts for i in range(nparts + 1)]
    c.pf = torch.stack([torch.stack([xd[:, a:b].sum(1), (xd[:, a:b] ** 2).sum(1)], -1) for a, b in zip(edges, edges[1:])]).float()
    c.gamma, c.beta = _un(g, 0.5, 1.5, c.C), 0.5 * _rn(g, c.C)
    c.gamma[4], c.gamma[5] = -c.gamma[4], 0.0
    c.mean64 = xd.mean(1)
    c.var64 = ((xd - c.mean64[:, None]) ** 2).mean(1)
    c.rstd64 = 1.0 / torch.sqrt(c.var64 + R.f32(EPS))
    A0, A1 = c.pf[:, :, 0].double().abs().sum(0), c.pf[:, :, 1].double().abs().sum(0)
    c.Bm = U * A0 / c.count + U * c.mean64.abs()
    c.Bv = U * (A1 + 2 * c.mean64.abs() * A0) / c.count
    c.Brel = 0.5 * c.Bv / (c.var64 + R.f32(EPS)) + U
    return c


def reg_gpu(c):
    import ctypes
    Lb, lib = _lib()
    s = Sent()
    parts, gam, bet = s.put(c.pf), s.put(c.gamma), s.put(c.beta)
    o = {k: s.out(c.C) for k in ("scale", "shift", "mean", "rstd")}
    Lb.check(lib.trunet_bn_finalize_fwd(Lb.ptr(parts), c.nparts, c.C, ctypes.c_double(c.count), Lb.ptr(gam), Lb.ptr(bet), EPS,
                                        0.1, None, None, *[Lb.ptr(o[k]) for k in ("scale", "shift", "mean", "rstd")], None,
                                        Lb.stream()), "bn_finalize_fwd")
    s.check("regimes %s" % (c.case,))
    return {k: v.cpu() for k, v in o.items()}


def reg_emul(c, mut=None):
    return _round(R.finalize_fwd(c.pf, c.count, c.gamma, c.beta, EPS, 0.1, mut=mut), ("scale", "shift", "mean", "rstd"))


def judge_reg(c, got, quiet=False):
    """the statistics against float64 of the DATA, every channel held to the conditioning bound (factor 2 on the whole);
    prints per channel the part of its bound rstd used"""
    j = Judge("BN-REGIMES n%d-g%d" % c.case, quiet)
    eps = R.f32(EPS)
    j.within("mean", got["mean"], c.mean64, 2 * c.Bm)
    j.within("rstd", got["rstd"], c.rstd64, 2 * c.Brel * c.rstd64)
    # scale = gamma * rstd32 (one more rounding), shift = beta - mean32 * scale32 (product and difference: two more, on
    # the terms |beta| + |mean scale|); the statistics' errors carried through
    sc64 = c.gamma.double() * c.rstd64
    b_sc = c.gamma.double().abs() * c.rstd64 * (2 * c.Brel + U)
    j.within("scale", got["scale"], sc64, b_sc)
    j.within("shift", got["shift"], c.beta.double() - c.mean64 * sc64,
             c.mean64.abs() * b_sc + sc64.abs() * 2 * c.Bm + 3 * U * (c.beta.double().abs() + (c.mean64 * sc64).abs()))
    if bool(torch.isfinite(got["rstd"]).all()):
        rs = got["rstd"].double()
        j.exact((rs > 0).all() and (rs <= (1.0 / eps ** 0.5) * (1 + 2 * U)).all(), "rstd above 1 / sqrt(eps): a negative variance")
        used = (rs - c.rstd64).abs() / (2 * c.Brel * c.rstd64)
        j.figs.append("rstd-used-of-bound " + " ".join("%s %.2f" % (k, float(u)) for k, u in zip(REG_CH, used)))
    j.exact(bool((got["scale"][5] == 0).all()) and bool(got["shift"][5] == c.beta[5]), "gamma = 0: scale != 0 or shift != beta")
    j.exact(bool(got["scale"][4] < 0), "gamma < 0: scale is not negative")
    j.done()


# ============================================================================================== eval_affine
EVAL_C = (1, 127, 128, 129, 192)


@functools.lru_cache(maxsize=None)
def eval_inputs(Cn):
    g = _gen("eval", Cn)
    c = types.SimpleNamespace(C=Cn, gamma=_un(g, 0.5, 1.5, Cn), beta=0.5 * _rn(g, Cn), rm=_rn(g, Cn), rv=_un(g, 1e-3, 2.0, Cn))
    c.rv[0] = 0.0                      # a running variance of 0
    c.gamma[Cn - 1] *= -1.0            # a negative weight
    c.ref64 = R.eval_affine(c.gamma, c.beta, c.rm, c.rv, EPS)
    return c


def eval_gpu(c):
    Lb, lib = _lib()
    s = Sent()
    i = [s.put(t) for t in (c.gamma, c.beta, c.rm, c.rv)]
    sc, sh = s.out(c.C), s.out(c.C)
    Lb.check(lib.trunet_bn_eval_affine(c.C, *[Lb.ptr(t) for t in i], EPS, Lb.ptr(sc), Lb.ptr(sh), Lb.stream()), "bn_eval_affine")
    s.check("eval_affine C %d" % c.C)
    return {"scale": sc.cpu(), "shift": sh.cpu()}


def eval_emul(c, mut=None):
    return _round(c.ref64, ("scale", "shift"))


def judge_eval(c, got, quiet=False):
    j = Judge("BN-EVAL C%d" % c.C, quiet)
    sc, sh = c.ref64["scale"], c.ref64["shift"]
    # scale = gamma / sqrtf(rv + eps): r = 3 (sum, sqrt, quotient); term |scale|
    j.within("scale", got["scale"], sc, 4 * U * sc.abs())
    # shift = beta - rm * scale32: r = 5 (the three of scale, product, difference); terms |beta|, |rm scale|
    j.within("shift", got["shift"], sh, 6 * U * (c.beta.double().abs() + (c.rm.double() * sc).abs()))
    j.exact(bool(got["scale"][c.C - 1] < 0), "negative gamma: scale is not negative")
    j.done()


# ============================================================================================== relu_bwd_stats
RELU_SHAPES = ((1, 1, 128, 1), (5, 1, 128, 127), (5, 13, 384, 130), (5, 13, 384, 257), (3, 43, 384, 384), (64, 16, 256, 255),
               (2, 257, 256, 131))           # (C, L, NP, N): L NP / 128 = 1, 1, 39, 39, 129, 32, 514 items against 16 x 8
RELU_CASES = [s + (m,) for s in RELU_SHAPES for m in ("plain", "bn")]
# channel roles: a negative scale; scale 0 with shift > 0 (all pass) and < 0 (all masked); shift 0 with z elements that are
# exactly 0 (pre = 0 in fp32 and fp64: masked by `>`)
ROLES = {1: {}, 2: {"on": 0, "zero": 1}, 3: {"zero": 0, "neg": 1, "off": 2}}
ROLES_5 = {"neg": 1, "on": 2, "off": 3, "zero": 4}


def relu_id(case):
    return "C%d-L%d-NP%d-N%d-%s" % case


def roles(Cn):
    return ROLES.get(Cn, ROLES_5)


@functools.lru_cache(maxsize=None)
def relu_inputs(case):
    Cn, L, NP, N, mode = case
    g = _gen("relu", case)
    c = types.SimpleNamespace(case=case, C=Cn, L=L, NP=NP, N=N, mode=mode, items=L * NP // 128)
    c.dy, c.z = _rn(g, Cn, L, NP), _rn(g, Cn, L, NP)
    c.sc, c.sh, c.mean = _un(g, 0.5, 1.5, Cn), 0.5 * _rn(g, Cn), 0.3 * _rn(g, Cn) + 0.1
    ro = roles(Cn)
    zeros = torch.zeros(Cn, L, NP, dtype=torch.bool)
    if "neg" in ro:
        c.sc[ro["neg"]] *= -1.0
    if "on" in ro:
        c.sc[ro["on"]], c.sh[ro["on"]] = 0.0, 0.7
    if "off" in ro:
        c.sc[ro["off"]], c.sh[ro["off"]] = 0.0, -0.7
    if "zero" in ro:
        c.sh[ro["zero"]] = 0.0
        zeros[ro["zero"], :, ::7] = True
    if Cn == 1:
        c.z[0, 0, 0], c.sh[0] = 0.8, 0.1               # the only live element of the smallest case passes the mask
    if mode == "plain":
        c.sc = c.sh = c.mean = None
    # nudge z away from mask flips (convt_cases._nudge), then plant the deliberate exact zeros
    sc = torch.ones(Cn, dtype=f64) if c.sc is None else c.sc.double()
    sh = torch.zeros(Cn, dtype=f64) if c.sh is None else c.sh.double()
    nz = (sc != 0)[:, None, None]
    safe = torch.where(nz, sc[:, None, None], torch.ones((), dtype=f64))
    for it in range(1, 12):
        pre = sc[:, None, None] * c.z.double() + sh[:, None, None]
        bad = nz & (pre.abs() < 2e-3)
        if not bool(bad.any()):
            break
        c.z = (c.z.double() + torch.where(bad, torch.where(pre >= 0, 1.0, -1.0) * (4e-3 * it) / safe, torch.zeros((), dtype=f64))).float()
    c.z[zeros] = 0.0
    pre = sc[:, None, None] * c.z.double() + sh[:, None, None]
    c.min_pre = float(torch.where(nz & ~zeros, pre.abs(), torch.full((), 1e30, dtype=f64)).min())
    assert c.min_pre >= 1e-3, (case, c.min_pre)
    c.n_zero = int((zeros[:, :, :N] & (pre[:, :, :N] == 0)).sum())
    c.dy[:, :, N:], c.z[:, :, N:] = NAN, NAN             # the header promises 0 beyond N whatever is there
    c.ref64 = R.relu_bwd_stats(c.dy, c.z, c.sc, c.sh, c.mean, N)
    c.blk = R.relu_bwd_stats(c.dy, c.z, c.sc, c.sh, c.mean, N, torch.float32, "blocked")
    c.seq = R.relu_bwd_stats(c.dy, c.z, c.sc, c.sh, c.mean, N, torch.float32, "seq")
    # fp32 and fp64 agree on every mask bit: no element is left out of any comparison
    assert torch.equal(c.ref64["dy"] != 0, c.blk["dy"] != 0) and torch.equal(c.ref64["dy"].float(), c.blk["dy"]), case
    c.yard = {k: worse(c.ref64[k], c.blk[k], c.seq[k]) for k in ("s1", "s2")}
    return c


def relu_gpu(c):
    Lb, lib = _lib()
    s = Sent()
    nparts = lib.trunet_relu_bwd_stats_nparts()
    assert nparts == R.RELU_PARTS
    dy, z = s.put(c.dy), s.put(c.z)
    bn = c.mode == "bn"
    sc, sh, mean = (s.put(c.sc), s.put(c.sh), s.put(c.mean)) if bn else (None, None, None)
    parts = s.out(nparts, c.C, 2) if bn else None
    Lb.check(lib.trunet_relu_bwd_stats(Lb.ptr(dy), Lb.ptr(z), Lb.ptr(sc), Lb.ptr(sh), Lb.ptr(mean), Lb.ptr(parts), c.C, c.L,
                                       c.NP, c.N, Lb.stream()), "relu_bwd_stats")
    s.check(relu_id(c.case))
    return {"dy": dy.cpu(), "parts": parts.cpu() if bn else None}


def relu_emul(c, mut=None):
    r = R.relu_bwd_stats(c.dy, c.z, c.sc, c.sh, c.mean, c.N, torch.float32, "blocked", mut)
    return {"dy": r["dy"], "parts": r["parts"] if c.mode == "bn" else None}


def judge_relu(c, got, quiet=False):
    j = Judge("RELU-BWD-STATS " + relu_id(c.case), quiet)
    want = c.ref64["dy"].float()
    j.exact(torch.equal(got["dy"].view(torch.int32), want.view(torch.int32)),
            "masked dy is not bit-exact (%d elements differ)" % int((got["dy"].view(torch.int32) != want.view(torch.int32)).sum()))
    j.exact(is_pos_zero(got["dy"][:, :, c.N:]), "dy is not exactly +0 for frames >= N")
    if c.mode == "bn":
        p = got["parts"]
        fin = bool(torch.isfinite(p).all())
        j.exact(fin, "partial rows are not finite")
        idle = torch.tensor([8 * gi >= c.items for gi in range(R.RELU_PARTS)])
        j.exact(bool((p[idle] == 0).all()), "rows of workgroups without an item are not exactly 0")
        if fin:
            j.close("sum_dy", p[:, :, 0].double().sum(0), c.ref64["s1"], c.yard["s1"])
            j.close("sum_dy_xc", p[:, :, 1].double().sum(0), c.ref64["s2"], c.yard["s2"])
    else:
        j.exact(got["parts"] is None, "plain ReLU with partials")
    j.done()


# ============================================================================================== from_frames_last_affine
FFL_SHAPES = ((300, 4, 257), (1, 8, 257), (77, 5, 13), (64, 8, 16), (130, 3, 33))       # (N, C, L)
FFL_CASES = [s + (r,) for s in FFL_SHAPES for r in (1, 0)]
FFL_TAIL = 64


def ffl_id(case):
    return "N%d-C%d-L%d-relu%d" % case


@functools.lru_cache(maxsize=None)
def ffl_inputs(case):
    N, Cn, L, relu = case
    g = _gen("ffl", case)
    NP = -(-N // 128) * 128
    c = types.SimpleNamespace(case=case, N=N, C=Cn, L=L, NP=NP, relu=relu)
    c.x = _rn(g, Cn, L, NP)
    c.x[:, :, N:] = NAN
    c.scale, c.shift = _un(g, 0.5, 1.5, Cn), 0.5 * _rn(g, Cn)
    c.scale[1], c.scale[2] = -c.scale[1], 0.0
    c.ref64 = R.from_frames_last_affine(c.x, N, c.scale, c.shift, relu)
    col = lambda v: v.double()[None, :, None]
    # y = max(fmaf(x, scale, shift), lo): r = 1; terms |scale x|, |shift| (max is 1-Lipschitz: the bound survives it)
    c.bnd = 2 * U * ((col(c.scale) * c.x[:, :, :N].double().permute(2, 0, 1)).abs() + col(c.shift).abs())
    return c


def ffl_gpu(c):
    Lb, lib = _lib()
    s = Sent()
    x, sc, sh = s.put(c.x), s.put(c.scale), s.put(c.shift)
    y = s.out(c.N * c.C * c.L, tail=FFL_TAIL)
    Lb.check(lib.trunet_from_frames_last_affine(Lb.ptr(x), Lb.ptr(y), c.N, c.C, c.L, c.NP, Lb.ptr(sc), Lb.ptr(sh), c.relu,
                                                Lb.stream()), "from_frames_last_affine")
    s.check(ffl_id(c.case))
    return {"y": y.cpu().view(c.N, c.C, c.L)}


def ffl_emul(c, mut=None):
    return {"y": R.from_frames_last_affine(c.x, c.N, c.scale, c.shift, c.relu, mut=mut).float()}


def judge_ffl(c, got, quiet=False):
    j = Judge("FROM-FRAMES-AFFINE " + ffl_id(c.case), quiet)
    j.within("y", got["y"], c.ref64, c.bnd)
    if c.relu:
        j.exact(bool((got["y"] >= 0).all()), "relu: a negative output")
    else:
        j.exact(bool((c.ref64 < -0.1).any()), "the case has no negative result")
    j.done()


# ============================================================================================== conv_first
CF_SL = ((2, 5), (2, 9), (2, 19), (2, 257), (1, 12))        # (S, Lin): Lout = 2, 4, 9 (the lo >= Lout tail), 128, 8
CF_CASES = [(Cin, Cout, S, Lin, NP) for S, Lin in CF_SL for Cin in (3, 4) for Cout in (5, 64) for NP in (128, 384)]
CF_TAIL = 512


def cf_id(case):
    return "Ci%d-Co%d-S%d-L%d-NP%d" % case


@functools.lru_cache(maxsize=None)
def cf_inputs(case):
    Cin, Cout, S, Lin, NP = case
    g = _gen("cf", case)
    c = types.SimpleNamespace(case=case, Cin=Cin, Cout=Cout, S=S, Lin=Lin, NP=NP, K=R.K_FIRST, Lout=R.lout_first(Lin, S))
    c.x, c.w, c.b = _rn(g, Cin, Lin, NP), 0.3 * _rn(g, Cout, Cin, c.K), 0.3 * _rn(g, Cout)
    c.ref64 = R.conv_first(c.x, c.w, c.b, S)
    c.blk = R.conv_first(c.x, c.w, c.b, S, torch.float32, "blocked")
    c.seq = R.conv_first(c.x, c.w, c.b, S, torch.float32, "seq")
    c.yard = worse(c.ref64, c.blk, c.seq)
    return c


def cf_gpu(c):
    Lb, lib = _lib()
    s = Sent()
    x, w, b = s.put(c.x), s.put(c.w, tail=16), s.put(c.b)
    y = s.out(c.Cout * c.Lout * c.NP, tail=CF_TAIL)
    Lb.check(lib.trunet_conv_first_fwd(Lb.ptr(x), Lb.ptr(w), Lb.ptr(b), Lb.ptr(y), c.Cin, c.Cout, c.K, c.S, c.Lin, c.Lout,
                                       c.NP, Lb.stream()), "conv_first_fwd")
    s.check(cf_id(c.case))
    return {"y": y.cpu().view(c.Cout, c.Lout, c.NP)}


def cf_emul(c, mut=None):
    return {"y": R.conv_first(c.x, c.w, c.b, c.S, torch.float32, "seq" if mut else "blocked", mut)}


def judge_cf(c, got, quiet=False):
    j = Judge("CONV-FIRST " + cf_id(c.case), quiet)
    j.close("y", got["y"], c.ref64, c.yard)
    j.done()


# ============================================================================================== reduce_partials
RP_NPARTS = (1, 3, 63, 64, 65, 600)
RP_NUMEL = (1, 15, 17, 100, 4096, 4097)       # numel <= 4096 with nparts >= 64 takes the 16-wide instance, the rest the 64-wide
RP_CASES = [(g, n, a) for g in RP_NPARTS for n in RP_NUMEL for a in (0, 1)]


def rp_id(case):
    return "g%d-n%d-acc%d" % case


def rp_inputs(case):
    nparts, numel, acc = case
    g = _gen("rp", case)
    c = types.SimpleNamespace(case=case, nparts=nparts, numel=numel, acc=acc)
    c.parts, c.out0 = _rn(g, nparts, numel), (_rn(g, numel) if acc else None)
    c.ref64 = R.reduce_partials(c.parts, c.out0)
    return c


def rp_gpu(c):
    Lb, lib = _lib()
    s = Sent()
    parts = s.put(c.parts)
    out = s.put(c.out0, tail=64) if c.acc else s.out(c.numel, tail=64)
    Lb.check(lib.trunet_reduce_partials(Lb.ptr(out), Lb.ptr(parts), c.nparts, c.numel, c.acc, Lb.stream()), "reduce_partials")
    s.check(rp_id(c.case))
    return {"out": out.cpu(), "parts": parts.cpu()}


def rp_emul(c, mut=None):
    return {"out": R.reduce_partials(c.parts, c.out0, mut=mut).float(), "parts": c.parts.clone()}


def judge_rp(c, got, quiet=False):
    j = Judge("REDUCE-PARTIALS " + rp_id(c.case), quiet)
    A = c.parts.double().abs().sum(0)
    t = c.parts.double().sum(0)
    if c.acc:
        # out + (float) t: r = 2 (t, sum); terms |out|, |t|
        j.within("out", got["out"], c.ref64, 3 * U * (c.out0.double().abs() + t.abs()) + D * A)
    else:
        j.within("out", got["out"], c.ref64, 2 * U * t.abs() + D * A)                 # one rounding
    j.exact(torch.equal(got["parts"], c.parts), "the partial image was modified")
    j.done()


# ============================================================================================== sumsq
SQ_N = (1, 3, 4, 1023, 1025, 4097)
SQ_CASES = [(n, off) for n in SQ_N for off in (0, 1)]      # off = 1: the pointer is one float past a 16-byte boundary


def sq_inputs(case):
    n, off = case
    c = types.SimpleNamespace(case=case, n=n, off=off, g=_rn(_gen("sq", case), n))
    c.ref64 = R.sumsq(c.g).reshape(1)
    return c


def sq_gpu(c):
    Lb, lib = _lib()
    s = Sent()
    buf = s.put(torch.cat([torch.full((c.off,), NAN), c.g]))
    g = buf[c.off:]
    assert g.data_ptr() % 16 == 4 * c.off
    out = s.out(1)
    Lb.check(lib.trunet_sumsq(Lb.ptr(g), c.n, Lb.ptr(out), Lb.stream()), "sumsq")
    s.check("sumsq %s" % (c.case,))
    return {"out": out.cpu()}


def sq_emul(c, mut=None):
    return {"out": c.ref64.float()}


def judge_sq(c, got, quiet=False):
    j = Judge("SUMSQ n%d-off%d" % c.case, quiet)
    j.within("out", got["out"], c.ref64, (2 * U + D) * c.ref64)                       # one rounding; every term >= 0
    j.done()


# ============================================================================================== the chain
CHAIN_SHAPES = ((5, 13, 384, 130), (64, 16, 256, 255))
CHAIN_CASES = [s + (r,) for s in CHAIN_SHAPES for r in ("ordinary", "offset")]
CHAIN_ILL = [s + ("ill",) for s in CHAIN_SHAPES]          # held to the conditioning bound, not to torch's fp32 autograd
CHAIN_RATIO = {"ordinary": 0.0, "offset": 5.0, "ill": 100.0}
CHAIN_PARTS = 24


def chain_id(case):
    return "C%d-L%d-NP%d-N%d-%s" % case


def bn_relu_autograd(z_ncl, gamma, beta, dy_ncl, dtype, steps=1, mom=0.1):
    """relu(F.batch_norm(z, training = True)) in `dtype`: (dz, dgamma, dbeta, running_mean, running_var after `steps`)"""
    z = z_ncl.to(dtype).clone().requires_grad_(True)
    g, b = gamma.to(dtype).clone().requires_grad_(True), beta.to(dtype).clone().requires_grad_(True)
    rm, rv = torch.zeros_like(g).detach(), torch.ones_like(g).detach()
    for _ in range(steps):
        y = torch.relu(F.batch_norm(z, rm, rv, g, b, True, R.f32(mom), R.f32(EPS)))
    (y * dy_ncl.to(dtype)).sum().backward()
    return z.grad, g.grad, b.grad, rm, rv


@functools.lru_cache(maxsize=None)
def chain_inputs(case):
    """z [C][L][NP] with per-channel |mean| / std = 0 (ordinary), 5 (offset) or 100 (ill), alternating sign; the live
    frames are the BatchNorm batch (count = L N); the partials are double sums over CHAIN_PARTS pieces rounded to fp32, how
    the producers hand them over.  z is nudged until every |pre| = |scale z + shift| of the float64 statistics is at least
    1e-3 AND above what the conditioning bound lets the kernel's fp32 scale and shift move it by (asserted), so that fp32,
    fp64 and the kernel agree on every ReLU mask bit; frames >= N hold NaN in dy and z."""
    Cn, L, NP, N, regime = case
    g = _gen("chain", case)
    c = types.SimpleNamespace(case=case, C=Cn, L=L, NP=NP, N=N, regime=regime, count=float(L * N))
    z = _rn(g, Cn, L, NP) * _un(g, 0.5, 2.0, Cn)[:, None, None]
    sign = torch.where(torch.arange(Cn) % 2 == 0, 1.0, -1.0)
    z = z + (CHAIN_RATIO[regime] * z[:, :, :N].std((1, 2)) * sign)[:, None, None]
    c.gamma, c.beta = _un(g, 0.5, 1.5, Cn), 0.5 * _rn(g, Cn)
    c.gamma[1] *= -1.0
    c.dy = _rn(g, Cn, L, NP)
    col = lambda v: v[:, None, None]
    eps = R.f32(EPS)
    margin = 2e-2 if regime == "ill" else 2e-3
    for it in range(1, 12):
        zl = z[:, :, :N].double()
        mean, var = zl.mean((1, 2)), zl.var((1, 2), unbiased=False)
        rstd = 1.0 / torch.sqrt(var + eps)
        sc = c.gamma.double() * rstd
        pre = col(sc) * (z.double() - col(mean)) + col(c.beta.double())
        bad = pre.abs() < margin
        bad[:, :, N:] = False
        if not bool(bad.any()):
            break                                     # zl, mean, var, rstd, sc, pre below are those of the final z
        z = (z.double() + torch.where(bad, torch.where(pre >= 0, 1.0, -1.0) * (2 * margin * it) / col(sc),
                                      torch.zeros((), dtype=f64))).float()
    else:
        raise AssertionError("%s: the nudge did not settle" % (case,))
    c.z = z.clone()
    c.z[:, :, N:], c.dy[:, :, N:] = NAN, NAN
    rows = zl.reshape(Cn, -1)
    edges = [(rows.shape[1] * i) // CHAIN_PARTS for i in range(CHAIN_PARTS + 1)]
    c.pf = torch.stack([torch.stack([rows[:, a:b].sum(1), (rows[:, a:b] ** 2).sum(1)], -1) for a, b in zip(edges, edges[1:])]).float()
    # the conditioning bound of these partials (module docstring)
    A0, A1 = c.pf[:, :, 0].double().abs().sum(0), c.pf[:, :, 1].double().abs().sum(0)
    c.mean64, c.var64, c.rstd64 = mean, var, rstd
    c.Bm = U * A0 / c.count + U * mean.abs()
    c.Bv = U * (A1 + 2 * mean.abs() * A0) / c.count
    c.Brel = 0.5 * c.Bv / (var + eps) + U
    xhat = col(rstd) * (zl - col(mean))
    pre = pre[:, :, :N]
    moved = 2 * (col(c.Brel) * (col(c.gamma.double()) * xhat).abs() + col(sc.abs() * c.Bm)) + 4 * U * (pre.abs() + col(c.beta.double().abs()))
    c.min_pre = float(pre.abs().min())
    assert c.min_pre >= 1e-3 and bool((pre.abs() > 2 * moved).all()), (case, c.min_pre)
    c.ratio = float((mean.abs() / var.sqrt()).min())
    ncl = lambda t: t[:, :, :N].permute(2, 0, 1).contiguous()
    back = lambda t: t.permute(1, 2, 0).contiguous()
    r64 = bn_relu_autograd(ncl(c.z), c.gamma, c.beta, ncl(c.dy), f64)
    r32 = bn_relu_autograd(ncl(c.z), c.gamma, c.beta, ncl(c.dy), torch.float32)
    c.ref64 = {"dz": back(r64[0]), "dgamma": r64[1], "dbeta": r64[2]}
    c.yard = {"dz": back(r32[0]), "dgamma": r32[1], "dbeta": r32[2]}
    # first-order effect of rstd (1 + e), mean + d on dz = gamma rstd (dy - m1 - xhat m2), xhat = rstd (z - mean),
    # m1 = mean(dy), m2 = mean(dy xhat) of the masked dy:  D xhat = e xhat - rstd d,  D m2 = e m2 - rstd d m1
    dym = torch.where(pre > 0, c.dy[:, :, :N].double(), torch.zeros((), dtype=f64))
    m1, m2 = dym.mean((1, 2)), (dym * xhat).mean((1, 2))
    e, d, gr = col(c.Brel), col(c.Bm * rstd), col(c.gamma.double().abs() * rstd)
    c.cond = {"dz": 2 * (e * c.ref64["dz"].abs() + gr * ((e * xhat.abs() + d) * col(m2.abs()) + xhat.abs() * (e * col(m2.abs()) + d * col(m1.abs())))),
              "dgamma": 2 * (c.Brel * c.ref64["dgamma"].abs() + rstd * c.Bm * c.ref64["dbeta"].abs()),
              "dbeta": torch.zeros(Cn, dtype=f64)}
    return c


def chain_steps(c, fwd, relu, bwd):
    """the three stages with the given implementations; dz = ca dy + cb z + cc formed in torch from the fp32 coefficients"""
    f = fwd(c)
    r = relu(c, f)
    b = bwd(c, f, r)
    col = lambda v: v.float()[:, None, None]
    dz = col(b["ca"]) * r["dy"][:, :, :c.N] + col(b["cb"]) * c.z[:, :, :c.N] + col(b["cc"])
    return {"dz": dz, "dgamma": b["dgamma"], "dbeta": b["dbeta"], "fwd": f, "relu": r, "bwd": b}


def chain_emul(c, mut=None):
    """the restatement's chain: double formulas on fp32 hand-overs, every stage's outputs rounded to fp32"""
    fwd = lambda c: _round(R.finalize_fwd(c.pf, c.count, c.gamma, c.beta, EPS, 0.1, mut=mut), ("scale", "shift", "mean", "rstd"))
    relu = lambda c, f: R.relu_bwd_stats(c.dy, c.z, f["scale"], f["shift"], f["mean"], c.N, torch.float32, "blocked", mut)
    bwd = lambda c, f, r: _round(R.finalize_bwd(r["parts"], c.count, c.gamma, f["mean"], f["rstd"], mut=mut),
                                 ("dgamma", "dbeta", "ca", "cb", "cc"))
    return chain_steps(c, fwd, relu, bwd)


def chain_gpu(c):
    import ctypes
    Lb, lib = _lib()

    def fwd(c):
        s = Sent()
        parts, gam, bet = s.put(c.pf), s.put(c.gamma), s.put(c.beta)
        o = {k: s.out(c.C) for k in ("scale", "shift", "mean", "rstd")}
        Lb.check(lib.trunet_bn_finalize_fwd(Lb.ptr(parts), CHAIN_PARTS, c.C, ctypes.c_double(c.count), Lb.ptr(gam), Lb.ptr(bet),
                                            EPS, 0.1, None, None, *[Lb.ptr(o[k]) for k in ("scale", "shift", "mean", "rstd")],
                                            None, Lb.stream()), "bn_finalize_fwd")
        s.check("chain fwd")
        return {k: v.cpu() for k, v in o.items()}

    def relu(c, f):
        s = Sent()
        dy, z = s.put(c.dy), s.put(c.z)
        sc, sh, mean = s.put(f["scale"]), s.put(f["shift"]), s.put(f["mean"])
        parts = s.out(R.RELU_PARTS, c.C, 2)
        Lb.check(lib.trunet_relu_bwd_stats(Lb.ptr(dy), Lb.ptr(z), Lb.ptr(sc), Lb.ptr(sh), Lb.ptr(mean), Lb.ptr(parts), c.C, c.L,
                                           c.NP, c.N, Lb.stream()), "relu_bwd_stats")
        s.check("chain relu")
        return {"dy": dy.cpu(), "parts": parts.cpu()}

    def bwd(c, f, r):
        s = Sent()
        parts = s.put(r["parts"])
        gam, mean, rstd = s.put(c.gamma), s.put(f["mean"]), s.put(f["rstd"])
        o = {k: s.out(c.C) for k in ("dgamma", "dbeta", "ca", "cb", "cc")}
        Lb.check(lib.trunet_bn_finalize_bwd(Lb.ptr(parts), R.RELU_PARTS, c.C, ctypes.c_double(c.count), Lb.ptr(gam),
                                            Lb.ptr(mean), Lb.ptr(rstd),
                                            *[Lb.ptr(o[k]) for k in ("dgamma", "dbeta", "ca", "cb", "cc")], Lb.stream()),
                 "bn_finalize_bwd")
        s.check("chain bwd")
        return {k: v.cpu() for k, v in o.items()}

    return chain_steps(c, fwd, relu, bwd)


def judge_chain(c, got, quiet=False):
    """dz, dgamma, dbeta against float64 autograd through relu(batch_norm(z)); yardstick: torch's fp32 autograd"""
    j = Judge("BN-CHAIN " + chain_id(c.case), quiet)
    for k in ("dz", "dgamma", "dbeta"):
        j.close(k, got[k], c.ref64[k], c.yard[k])
    j.exact(is_pos_zero(got["relu"]["dy"][:, :, c.N:]), "masked dy beyond N")
    j.done()


def judge_chain_ill(c, got, quiet=False):
    """|mean| / std = 100: the chain is held to the conditioning bound of its fp32 partial sums carried to first order into
    dz and dgamma (chain_inputs; factor 2 for the second order), ADDED to the allowance `close` gives any fp32 result;
    prints the error as a multiple of torch's own fp32 error -- the size of the sumsq / count - mean^2 design limit"""
    j = Judge("BN-CHAIN " + chain_id(c.case), quiet)
    for k in ("dz", "dgamma", "dbeta"):
        e_y, bnd = CR.bound(c.ref64[k], c.yard[k])[:2]
        j.within(k, got[k], c.ref64[k], c.cond[k] + bnd)
        j.figs.append("%s-error-over-torch-fp32 %.1f" % (k, float((got[k].double() - c.ref64[k]).abs().max()) / (e_y + 1e-300)))
    j.exact(torch.equal(got["relu"]["dy"].view(torch.int32), R.relu_bwd_stats(c.dy, c.z, got["fwd"]["scale"], got["fwd"]["shift"],
            None, c.N)["dy"].float().view(torch.int32)), "masked dy is not bit-exact")
    j.done()


def chain_same_bits(a, b):
    for st in ("fwd", "relu", "bwd"):
        for k in a[st]:
            assert torch.equal(a[st][k], b[st][k]), "second run: %s %s differs" % (st, k)
