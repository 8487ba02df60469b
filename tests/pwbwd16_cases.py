"""The fused bf16 pointwise backward (trunet_bf16_pw_bwd) and its unfused weight-gradient instances (trunet_bf16_wgrad)
through the C ABI against tests/pwbwd16_ref.py: layer signatures, input regimes, step geometry, launch helpers and the case
functions tests/test_pwbwd16_gpu.py calls.

A case is (signature, regime, NP, N, P).  Inputs come from seeded CPU generators keyed by the case; frames >= N hold live
random values (the kernels must ignore them in every sum and still store the data gradient there).

Step geometry: a step is (64 frames, position), position fastest; total = P NP / 64 steps are dealt to G workgroups,
workgroup b owning [b total / G, (b + 1) total / G).  The list is laid out for G = 256 (trunet_conv_wgrad_nparts(), asserted
by the GPU test):
    small   (64, 1), (64, 33), (192, 130) at P <= 3: total <= 9 < G -- all but a few workgroups own nothing, the others one
            step (the one-stage start of the depth-2 loop); N ends in the first / the second 32-frame half of a chunk, and
            chunk 2 of (192, 130) has 2 live frames;  (192, 64) adds a chunk wholly beyond N
    mid     NP = 8320: P = 3 -> 390 steps, workgroups own 1 or 2 (a full pair); P = 5 -> 650 steps, workgroups own 2 or 3 (the
            odd tail); neither total is a multiple of G / 2, so runs cross chunk boundaries (p wraps inside a run)
    big     NP = 16448, P = 3 -> 771 >= 3 G steps: 3 or 4 per workgroup"""
import ctypes
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

import pwbwd16_ref as R  # noqa: E402
from convt_cases import from_octets, report, to_octets  # noqa: E402

G = 256
NS = types.SimpleNamespace


def _src(nchan, dL=0, off=0, bn=False, mask=False, stats=False, accum=False, signed=False):
    return dict(nchan=nchan, dL=dL, off=off, bn=bn, mask=mask, stats=stats, accum=accum, signed=signed)


# M; sources (nchan, L - P, pos_off, kind) as engine_bf16.pw_bwd is handed them, then the contract shapes the network does
# not use.  A plain source next to a BN+ReLU one is a post-ReLU tensor (the launch applies ReLU to it: the header's rule);
# `signed`: a plain source of a launch without any BN source may hold negative values
SIGS = {
    "enc128": (128, [_src(128, bn=True, mask=True, stats=True, accum=True)]),
    "plain64": (128, [_src(64, mask=True, accum=True)]),
    "dec_pad": (64, [_src(64, dL=-1, off=-1, bn=True, mask=True, stats=True), _src(128)]),              # the F.pad shift
    "dec_crop": (64, [_src(64, dL=2, off=1, bn=True, mask=True, stats=True), _src(128)]),               # the crop
    "plain128": (64, [_src(128, signed=True)]),
    "bn64": (64, [_src(64, bn=True, mask=True, stats=True)]),
    "m16": (16, [_src(32, bn=True, mask=True, stats=True)]),          # one dz k-step, a row tile reading past M
    "m48": (48, [_src(32, bn=True, mask=True, stats=True, accum=True)]),   # odd octet count, odd number of dz k-steps
    "seg3": (64, [_src(32, bn=True, mask=True, stats=True), _src(32, mask=True, accum=True),
                  _src(32, dL=2, off=1, bn=True, mask=True, stats=True, accum=True)]),
}
# trunet_bf16_wgrad only (the fused entry point refuses them): 8 dz rows; a 4-channel source in a zero-padded octet
WGRAD_SIGS = {
    "thin8": (8, [_src(64, bn=True)]),
    "thin4": (64, [_src(4, signed=True)]),
}
# a shape both entry points' headers rule out for the fused kernel: 4 row tiles x 6 channel tiles of weight gradient
REFUSED_SIGS = {"m128k192": (128, [_src(64, bn=True, mask=True, stats=True), _src(128)])}
SMALL_NPN = ((64, 1), (64, 33), (192, 130))
BEYOND = (192, 64)
MID_NP, MID_N, BIG_NP, BIG_N = 8320, 8258, 16448, 16400
REGIMES = ("ordinary", "exact", "zero_cotangent")
ZERO_PRE_CH, ALWAYS_ON_CH, ALWAYS_OFF_CH = 10, 2, 6        # every regime: the BN channels with c0 = 0


def small_ps(sig):
    return (2, 3) if sig == "dec_pad" else (1, 3)          # the shifted source has L = P - 1 >= 1


ORDINARY_SMALL = [(s, "ordinary", NP, N, P) for s in SIGS for NP, N in SMALL_NPN for P in small_ps(s)]
ORDINARY_SMALL += [(s, "ordinary") + BEYOND + (2,) for s in ("enc128", "dec_pad")]
EXACT = [(s, "exact", NP, N, P) for s in SIGS for NP, N, P in ((192, 130, 2), (64, 33, 3))]
ZERO = [(s, "zero_cotangent", 192, 130, 2) for s in SIGS]
SMALL = ORDINARY_SMALL + EXACT + ZERO
MID = [("m16", "ordinary", MID_NP, MID_N, 3), ("m16", "ordinary", MID_NP, MID_N, 5), ("bn64", "ordinary", MID_NP, MID_N, 5)]
BIG = [(s, "ordinary", BIG_NP, BIG_N, 3) for s in ("enc128", "dec_pad")]
CASES = SMALL + MID + BIG
WGRAD_CASES = [(s, r, 192, 130, 3) for s in ("enc128", "dec_pad", "seg3", "thin8", "thin4") for r in ("ordinary", "exact")]
WGRAD_CASES += [("dec_crop", "ordinary", MID_NP, MID_N, 5)]


def case_id(case):
    return "%s-%s-NP%d-N%d-P%d" % case


def is_small(case):
    return case[2] <= 1024


def steps_owned(NP, P, grid=G):
    """[grid] number of steps of every workgroup"""
    total = P * (NP // R.STEP)
    return torch.tensor([((b + 1) * total) // grid - (b * total) // grid for b in range(grid)])


def crosses_chunk(NP, P, grid=G):
    """some workgroup's run holds the last position of one chunk and the first of the next"""
    total = P * (NP // R.STEP)
    for b in range(grid):
        s0, s1 = (b * total) // grid, ((b + 1) * total) // grid
        if s1 - s0 >= 2 and (s1 - 1) // P > s0 // P:
            return True
    return False


def _gen(*key):
    return torch.Generator().manual_seed(int(hashlib.sha1(repr(key).encode()).hexdigest()[:8], 16))


def inputs(case):
    sig, regime, NP, N, P = case
    M, srcs = SIGS.get(sig) or WGRAD_SIGS.get(sig) or REFUSED_SIGS[sig]
    g = _gen("pwbwd16", case)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    un = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g, dtype=torch.float32)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    pick = lambda vals, n: torch.tensor(vals, dtype=torch.float32)[torch.randint(0, len(vals), (n,), generator=g)]
    rb = R.bf16_round
    exact = regime == "exact"
    K = sum(s["nchan"] for s in srcs)
    c = NS(case=case, sig=sig, regime=regime, M=M, N=N, NP=NP, P=P, K=K)
    if exact:
        # dz = ca dy + cb z + cc lies on the 2^-8 grid with |dz| <= 5: up to 11 significant bits, so its bf16 rounding
        # happens (|dz| >= 1) and meets ties; W on the 1/4 grid, half of it zero; x, c1, mean on the 1/8 grid, c0 in
        # {1, -1, 1/2, 0}: pre = c0 x + c1 on the 1/16 grid, |pre| <= 2.5 (6 bits: the activation's rounding is the identity)
        c.dy, c.z = ri(-32, 32, M, P, NP) / 16, ri(-32, 32, M, P, NP) / 16
        c.ca, c.cb, c.cc = pick([1.0, 1.5, 0.5, -1.0], M), pick([0.25, -0.25, 0.5, 0.0], M), ri(-256, 256, M) / 256
        c.W = ri(-4, 4, M, K) / 4 * (torch.rand(M, K, generator=g) < 0.5).float()
    else:
        c.dy, c.z = rb(rn(M, P, NP)), rb(rn(M, P, NP))
        c.ca, c.cb, c.cc = un(0.5, 1.5, M), 0.2 * rn(M), 0.1 * rn(M)
        c.W = 0.1 * rn(M, K)
    if regime == "zero_cotangent":
        c.dy, c.cb, c.cc = torch.zeros_like(c.dy), torch.zeros_like(c.cb), torch.zeros_like(c.cc)
    c.segs, woff = [], 0
    mixed = any(s["bn"] for s in srcs)
    for sd in srcs:
        n, L = sd["nchan"], P + sd["dL"]
        s = NS(nchan=n, L=L, off=sd["off"], woff=woff, bn=sd["bn"], mask=sd["mask"], stats=sd["stats"], accum=sd["accum"])
        woff += n
        if exact:
            s.x, s.prev = ri(-12, 12, n, L, NP) / 8, ri(-16, 16, n, L, NP) / 8
            s.c0, s.c1, s.mean = pick([1.0, -1.0, 0.5, 0.0], n), ri(-8, 8, n) / 8, ri(-4, 4, n) / 8
        else:
            s.x, s.prev = rb(rn(n, L, NP)), rb(rn(n, L, NP))
            s.c0, s.c1, s.mean = un(0.5, 1.5, n), 0.5 * rn(n), 0.3 * rn(n)
            s.c0[1::4] *= -1                                   # every fourth channel: a negative BatchNorm weight
        if s.bn:
            for ch, sh in ((ALWAYS_ON_CH, 0.5), (ALWAYS_OFF_CH, -0.5), (ZERO_PRE_CH, 0.0)):
                s.c0[ch % n], s.c1[ch % n] = 0.0, sh           # pre = shift: always on, always off, exactly 0 (> against >=)
        else:
            s.c0, s.c1, s.mean = torch.ones(n), torch.zeros(n), torch.zeros(n)
            if mixed or not sd["signed"]:
                s.x = s.x.clamp_min(0)                         # a post-ReLU tensor: about half of it exactly 0
        c.segs.append(s)
    return c


def to_device(c, dev):
    """the case with every tensor on `dev` (the restatement runs where its inputs are)"""
    mv = lambda o: NS(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in vars(o).items() if k != "segs"})
    out = mv(c)
    out.segs = [mv(s) for s in c.segs]
    return out


def refs(c, seq=True, dev="cpu"):
    """ordinary / zero_cotangent: the float64 reference (no intermediate rounding) and the yardstick, the worse of the fp32
    emulation's orders, element by element (`blocked` alone with seq = False: the big cases).  exact: the float64 restatement
    with the kernel's roundings; it needs no yardstick."""
    cd = to_device(c, dev)
    cpu = lambda o: {k: v.cpu() for k, v in o.items()}
    if c.regime == "exact":
        c.ref64 = cpu(R.pw_bwd(cd, torch.float64, bf16=True))
        return c
    c.ref64 = cpu(R.pw_bwd(cd, torch.float64, bf16=False))
    c.blk = cpu(R.pw_bwd(cd, torch.float32, "blocked"))
    if seq:
        c.seq = cpu(R.pw_bwd(cd, torch.float32, "seq"))
        c.yard = R.yardstick(c.ref64, c.blk, c.seq)
    else:
        c.yard = c.blk
    return c


@functools.lru_cache(maxsize=None)
def small(case):
    """cached: the small cases are shared between tests and must be left unchanged"""
    assert is_small(case)
    return refs(inputs(case))


def wgrad_view(c, two):
    """the case as trunet_bf16_wgrad sees it: no data gradient; two = False: dz is dy as it is (TRUNET_PRO_NONE)"""
    w = to_device(c, "cpu")
    for s in w.segs:
        s.mask = s.stats = s.accum = False
    if not two:
        w.ca, w.cb, w.cc = torch.ones(c.M), torch.zeros(c.M), torch.zeros(c.M)
    w.two = two
    return w


# ---------------------------------------------------------------------------------------------- launches
SENT = 7.5                 # sentinel around the weight slot and the bias row, and the guard octets' value
W_OFF, W_TAIL = 96, 64     # the weight slot starts 96 floats into its image and ends 64 before the next
B_STRIDE, B_OFF = 160, 16
NAN = float("nan")


def _dev(t):
    return t.cuda().contiguous()


def _oct(t):
    """octet image of [C][L][NP]; C is padded to a multiple of 8 with zero channels"""
    Cn = t.shape[0]
    if Cn % 8:
        t = torch.cat([t, torch.zeros(8 - Cn % 8, *t.shape[1:])])
    return to_octets(t)


def _bseg(Lb, s, x16, keep, **over):
    sg = Lb.BSeg()
    sg.src0 = Lb.ptr16(x16)
    sg.nchan, sg.L, sg.pos_mul, sg.pos_off, sg.pos_div, sg.woff = s.nchan, s.L, 1, s.off, 1, s.woff
    sg.mode = Lb.PRO_BNRELU if s.bn else Lb.PRO_NONE
    if s.bn:
        c0, c1 = _dev(s.c0), _dev(s.c1)
        keep += [c0, c1]
        sg.c0, sg.c1 = Lb.ptr(c0), Lb.ptr(c1)
    for k, v in over.items():
        setattr(sg, k, v)
    return sg


def _wgrad_common(Lb, aw, c, keep, w_numel, wimg, bimg, bias, two=True):
    aw.NP, aw.N, aw.P, aw.p_begin, aw.M, aw.a_L, aw.a_pos_off = c.NP, c.N, c.P, 0, c.M, c.P, 0
    aw.a_mode = Lb.PRO_BNBWD if two else Lb.PRO_NONE
    aw.ldw_m, aw.ldw_c, aw.w_m_off, aw.nseg = c.K, 1, 0, len(c.segs)
    dy = _dev(_oct(c.dy))
    keep.append(dy)
    aw.a0 = Lb.ptr16(dy)
    if two:
        t = [_dev(_oct(c.z)), _dev(c.ca), _dev(c.cb), _dev(c.cc)]
        keep += t
        aw.a1, aw.ac0, aw.ac1, aw.ac2 = Lb.ptr16(t[0]), Lb.ptr(t[1]), Lb.ptr(t[2]), Lb.ptr(t[3])
    aw.w_numel, aw.b_stride, aw.b_off = w_numel, B_STRIDE, B_OFF
    aw.w_partials = Lb.ptr(wimg) + 4 * W_OFF
    aw.b_partials = Lb.ptr(bimg) if bias else None


def _out_buffers(c, grid):
    """weight images and bias rows: NaN where the kernel must write, sentinels everywhere else"""
    w_numel = W_OFF + c.M * c.K + W_TAIL
    wimg = torch.full((grid, w_numel), SENT, device="cuda", dtype=torch.float32)
    wimg[:, W_OFF:W_OFF + c.M * c.K] = NAN
    bimg = torch.full((grid, B_STRIDE), SENT, device="cuda", dtype=torch.float32)
    bimg[:, B_OFF:B_OFF + c.M] = NAN
    return w_numel, wimg, bimg


def pack_wT(Lb, c):
    """wfragT as engine_bf16.pw_bwd builds it: ONE image of all K source channels for K <= 128, else one image per source,
    back to back"""
    lib = Lb.lib()
    W = _dev(c.W)
    nks = (c.M // 8 + 1) // 2
    wf = torch.zeros((c.K // 32) * nks * 64 * 8, device="cuda", dtype=torch.bfloat16)
    one = lambda v: (ctypes.c_int32 * 1)(v)
    if c.K <= 128:
        got = lib.trunet_bf16_pack_weight(Lb.ptr(W), Lb.ptr16(wf), c.K, 1, c.K, 0, 1, one(c.M), one(0), Lb.stream())
        assert got == nks, got
    else:
        at = 0
        for s in c.segs:
            got = lib.trunet_bf16_pack_weight(Lb.ptr(W), Lb.ptr16(wf) + 2 * at, s.nchan, 1, c.K, s.woff, 1, one(c.M), one(0),
                                              Lb.stream())
            assert got == nks, got
            at += (s.nchan // 32) * nks * 64 * 8
    return wf


def pw_bwd_args(c, prezero=False, bias=True):
    """the argument block of trunet_bf16_pw_bwd for the case, every output prefilled: weight slot, bias row, statistics rows
    (zero with prezero, which the call is then told) and the visited positions of a never-accumulated out[s] with NaN; the
    other positions of out[s] with `prev`; one guard octet behind every out[s].  Returns (args, buffers)."""
    from tinyrecurrentunet_amd import _lib as Lb
    lib = Lb.lib()
    grid, nparts = lib.trunet_conv_wgrad_nparts(), lib.trunet_bf16_pw_bwd_nparts()
    assert grid == G and nparts == 2 * G, (grid, nparts)
    keep = []
    w_numel, wimg, bimg = _out_buffers(c, grid)
    a = Lb.BPwBwdArgs()
    _wgrad_common(Lb, a.w, c, keep, w_numel, wimg, bimg, bias)
    wf = pack_wT(Lb, c)
    a.dg.wfragT, a.dg.nrt_total = Lb.ptr16(wf), c.K // 32
    outs, parts = [], []
    for i, s in enumerate(c.segs):
        x16 = _dev(_oct(s.x))
        keep.append(x16)
        a.w.seg[i] = _bseg(Lb, s, x16, keep)
        pre = s.prev.clone()
        if not s.accum:
            p0, p1, off = R.p_range(s, c.P)
            pre[:, p0 + off:p1 + off] = NAN
        o = torch.cat([to_octets(pre).reshape(-1), torch.full((8,), SENT, dtype=torch.bfloat16)]).cuda()
        outs.append(o)
        a.dg.out[i] = Lb.ptr16(o)
        fl = Lb.DG_STORE | (Lb.DG_MASK if s.mask else 0) | (Lb.DG_ACCUM if s.accum else 0)
        part = None
        if s.stats:
            fl |= Lb.DG_STATS | (Lb.DG_PREZERO if prezero else 0)
            part = torch.full((nparts, s.nchan, 2), 0.0 if prezero else NAN, device="cuda", dtype=torch.float32)
            mean = _dev(s.mean)
            keep.append(mean)
            a.dg.mean[i], a.dg.partials[i] = Lb.ptr(mean), Lb.ptr(part)
        parts.append(part)
        a.dg.flags[i] = fl
    return a, NS(keep=keep, wf=wf, wimg=wimg, bimg=bimg if bias else None, outs=outs, parts=parts)


def _collect(c, b):
    n = lambda s: s.nchan * s.L * c.NP
    return NS(wimg=b.wimg.cpu(), bimg=None if b.bimg is None else b.bimg.cpu(),
              out16=[o.cpu()[:n(s)].view(s.nchan // 8, s.L, c.NP, 8) for o, s in zip(b.outs, c.segs)],
              guard=[o.cpu()[n(s):] for o, s in zip(b.outs, c.segs)],
              parts=[None if p is None else p.cpu() for p in b.parts], own=steps_owned(c.NP, c.P) > 0)


def gpu_pw_bwd(c, prezero=False, bias=True):
    """one launch of trunet_bf16_pw_bwd; returns CPU tensors: wimg [G][w_numel], bimg [G][B_STRIDE] (None with bias = False),
    out16[s] bf16 [nchan/8][L][NP][8], guard[s] bf16 [8], parts[s] [2 G][nchan][2] or None, own bool [G]"""
    from tinyrecurrentunet_amd import _lib as Lb
    a, b = pw_bwd_args(c, prezero, bias)
    Lb.check(Lb.lib().trunet_bf16_pw_bwd(a, Lb.stream()), "bf16_pw_bwd " + case_id(c.case))
    torch.cuda.synchronize()
    return _collect(c, b)


def gpu_wgrad(c, two, bias=True):
    """one launch of trunet_bf16_wgrad (bwgrad_kernel<two, *, false>) on NaN-prefilled partials"""
    from tinyrecurrentunet_amd import _lib as Lb
    lib = Lb.lib()
    grid = lib.trunet_conv_wgrad_nparts()
    assert grid == G
    keep = []
    w_numel, wimg, bimg = _out_buffers(c, grid)
    a = Lb.BWgradArgs()
    _wgrad_common(Lb, a, c, keep, w_numel, wimg, bimg, bias, two)
    for i, s in enumerate(c.segs):
        x16 = _dev(_oct(s.x))
        keep.append(x16)
        a.seg[i] = _bseg(Lb, s, x16, keep)
    Lb.check(lib.trunet_bf16_wgrad(a, Lb.stream()), "bf16_wgrad " + case_id(c.case))
    torch.cuda.synchronize()
    return NS(wimg=wimg.cpu(), bimg=bimg.cpu() if bias else None, own=steps_owned(c.NP, c.P) > 0)


# ---------------------------------------------------------------------------------------------- comparison and report
def sums(c, o):
    """the outputs of a launch under the restatement's names: partial images, bias rows and statistics rows summed in float64"""
    out = {"dW": o.wimg[:, W_OFF:W_OFF + c.M * c.K].double().sum(0).view(c.M, c.K)}
    if o.bimg is not None:
        out["db"] = o.bimg[:, B_OFF:B_OFF + c.M].double().sum(0)
    for i, s in enumerate(getattr(o, "out16", [])):
        out["g%d" % i] = from_octets(s)
        if o.parts[i] is not None:
            out["st0_%d" % i], out["st1_%d" % i] = o.parts[i][:, :, 0].double().sum(0), o.parts[i][:, :, 1].double().sum(0)
    return out


def compare(tag, c, got, names):
    """ordinary: every output through `close`; exact: equal bits (the sums' float64 value IS the fp32 value).  Every figure
    is printed BEFORE the first assertion fires; returns {name: (err, e_y, bound)}."""
    res, fails = {}, []
    for k in names:
        r64 = c.ref64[k]
        err = float((got[k].double() - r64).abs().max()) if r64.numel() else 0.0
        if c.regime == "exact":
            res[k] = (err, 0.0, 0.0)
            if not torch.equal(got[k].double(), r64):
                bad = got[k].double() != r64
                fails.append("%s %s: %d of %d elements differ from the exact value, max error %.3e" %
                             (tag, k, int(bad.sum()), bad.numel(), err))
        else:
            e_y, bnd = R.bound(r64, c.yard[k])[:2]
            res[k] = (err, e_y, bnd)
            try:
                R.close(got[k], r64, c.yard[k], "%s %s" % (tag, k))
            except AssertionError as e:
                fails.append(str(e))
    report("%s: kernel error / e_y / bound  " % tag + "  ".join("%s %.2e/%.2e/%.2e" % ((n,) + res[n]) for n in res),
           "parity_pwbwd16.txt")
    assert not fails, "\n".join(fails)
    return res


def mask64(s):
    """[nchan][L][NP] bool: where the data gradient passes (float64; tests/test_pwbwd16_ref_cpu.py shows that the kernel's fp32
    fma has the same sign everywhere)"""
    return (s.c0.double()[:, None, None] * s.x.double() + s.c1.double()[:, None, None]) > 0


def exactness(c, o, tag):
    """what must hold bit for bit in every regime: nothing left unwritten, nothing written outside the slots, untouched
    positions, exact zeros where the contract has zeros"""
    M, K, N = c.M, c.K, c.N
    slot = o.wimg[:, W_OFF:W_OFF + M * K]
    assert not bool(torch.isnan(slot).any()), "%s: weight images have unwritten (NaN) elements" % tag
    assert bool((o.wimg[:, :W_OFF] == SENT).all()) and bool((o.wimg[:, W_OFF + M * K:] == SENT).all()), \
        "%s: a write outside the weight slot" % tag
    assert bool((slot[~o.own] == 0).all()), "%s: weight images of workgroups without steps are not exactly 0" % tag
    if o.bimg is not None:
        row = o.bimg[:, B_OFF:B_OFF + M]
        assert not bool(torch.isnan(row).any()), "%s: bias rows have unwritten (NaN) elements" % tag
        assert bool((o.bimg[:, :B_OFF] == SENT).all()) and bool((o.bimg[:, B_OFF + M:] == SENT).all()), \
            "%s: a write outside the bias row" % tag
        assert bool((row[~o.own] == 0).all()), "%s: bias rows of workgroups without steps are not exactly 0" % tag
    zc = c.regime == "zero_cotangent"
    if zc:
        assert bool((slot == 0).all()) and (o.bimg is None or bool((o.bimg[:, B_OFF:B_OFF + M] == 0).all())), \
            "%s: zero cotangent, non-zero weight or bias gradient" % tag
    for i, s in enumerate(c.segs if hasattr(o, "out16") else []):
        g16, prev16 = o.out16[i], to_octets(s.prev)
        g = from_octets(g16)
        assert not bool(torch.isnan(g).any()), "%s: out[%d] has unwritten (NaN) elements" % (tag, i)
        assert bool((o.guard[i] == SENT).all()), "%s: a write behind out[%d]" % (tag, i)
        p0, p1, off = R.p_range(s, c.P)
        vis = torch.zeros(s.L, dtype=torch.bool)
        vis[p0 + off:p1 + off] = True
        assert torch.equal(g16[:, ~vis].view(torch.int16), prev16[:, ~vis].view(torch.int16)), \
            "%s: out[%d] changed at a position no p reaches" % (tag, i)
        keep = mask64(s) if s.mask else torch.ones_like(g, dtype=torch.bool)
        rest = torch.where(keep, s.prev, torch.zeros(())) if s.accum else torch.zeros_like(g)     # what dz = 0 leaves
        fr = slice(0, None) if zc else slice(N, None)
        assert torch.equal(g[:, vis, fr], rest[:, vis, fr]), \
            "%s: out[%d] is not mask(prev) / 0 %s" % (tag, i, "everywhere" if zc else "for frames >= N")
        if s.stats:
            pt = o.parts[i]
            assert not bool(torch.isnan(pt).any()), "%s: statistics rows %d have unwritten (NaN) elements" % (tag, i)
            assert bool((pt[(~o.own).repeat_interleave(2)] == 0).all()), \
                "%s: statistics rows %d of workgroups without steps are not exactly 0" % (tag, i)
            if zc and not s.accum:
                assert bool((pt == 0).all()), "%s: zero cotangent, non-zero statistics" % tag
            for ch in (ZERO_PRE_CH, ALWAYS_OFF_CH):
                assert bool((g[ch % s.nchan][vis] == 0).all()) and bool((pt[:, ch % s.nchan] == 0).all()), \
                    "%s: out[%d] channel %d (pre <= 0 everywhere) is not exactly 0" % (tag, i, ch)


def same_bits(o1, o2, what, skip=()):
    for k in ("wimg", "bimg"):
        if k not in skip:
            assert torch.equal(getattr(o1, k), getattr(o2, k)), "%s: %s differs" % (what, k)
    for i in range(len(o1.out16)):
        assert torch.equal(o1.out16[i].view(torch.int16), o2.out16[i].view(torch.int16)), "%s: out[%d] differs" % (what, i)
        if o1.parts[i] is not None:
            assert torch.equal(o1.parts[i], o2.parts[i]), "%s: statistics rows %d differ" % (what, i)


def check_case(c):
    """one launch of the fused entry point: every output against the restatement, then the exactness assertions"""
    o = gpu_pw_bwd(c)
    tag = "PWBWD16 " + case_id(c.case)
    res = compare(tag, c, sums(c, o), R.outputs(c))
    exactness(c, o, tag)
    return res, o


def check_wgrad(c, two):
    """one launch of an unfused instance on the same inputs: dW and db against the restatement of its view of the case"""
    w = wgrad_view(c, two)
    refs(w, seq=is_small(c.case))
    o = gpu_wgrad(w, two)
    tag = "BWGRAD16 %s %s" % ("bn-backward dz" if two else "plain dz", case_id(c.case))
    res = compare(tag, w, sums(w, o), ["dW", "db"])
    exactness(w, o, tag)
    return res
