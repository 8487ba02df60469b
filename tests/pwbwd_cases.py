"""The fp32 fused pointwise backward (trunet_pw_bwd: the six pw_bwd_kernel instances, each on the fp32 MFMA and on the
three-term bf16 split) and trunet_conv_wgrad on its own (both conv_wgrad_kernel instances and the four of wgrad_small.hip)
through the C ABI against tests/pwbwd_ref.py: layer signatures, input regimes, tile geometry, launch helpers and the case
functions tests/test_pwbwd_gpu.py calls.

A case is (signature, regime, NP, N, P).  Inputs come from seeded generators keyed by the case (CPU for the small cases,
which the CPU tests share; the device's for the others); frames >= N of dy, z, every source and every prev hold live random
values (the kernels must keep them out of every sum and still store the data gradient there).

Every launch runs as the engine launches it (engine.py, Fp32Kernels.pw_bwd / wgrad, the _wg_slot layout): the image stride
w_numel is larger than the weight and the weight slot starts W_OFF floats into its image; the bias row lies inside a longer
row at B_BASE + b_off; what the launch must write is prefilled with NaN (zero for conv_wgrad_kernel, whose contract is a
zero-filled image), everything around it with the sentinel SENT; statistics rows are prefilled with NaN unless the call is
told TRUNET_DG_PREZERO.

Signature table: instance pw_bwd_kernel<AK, SEC, KSPLIT, *> and ring depth NB (nb_of, restating the host code of pw_bwd.hip)

    enc128    128 <- 128 BN, accum, stats                               <64, false, false>   NB 3
    plain64   128 <- 64 plain post-ReLU, accum                          <64, false, true>    NB 3
    dec_pad   64 <- [64 BN pos_off -1, L = P - 1 | 128 raw]   (F.pad)    <32, true,  false>   NB 3
    dec_crop  64 <- [64 BN pos_off +1, L = P + 2 | 128 raw]   (crop)     <32, true,  false>   NB 3
    plain128  64 <- 128 raw signed                                      <32, false, false>   NB 4
    bn64      64 <- 64 BN                                               <32, false, true>    NB 4
    thin8     8 <- [64 BN | 64 plain post-ReLU]                         <16, false, false>   NB 4
    m96       96 <- 128 BN, accum      (contract shape, not sent)       <64, false, false>   NB 3   rows 96..127 padded
    m32       32 <- 128 BN             (contract shape, not sent)       <16, false, false>   NB 4
    m20       20 <- [64 BN | 64 raw]   (contract shape, not sent)       <16, false, false>   NB 4   rows 20..31 padded
    gru_a     rows 192..319 of 384 dz rows, weight rows 0..127 of 192, b_off 0, mask + accum          <64, false, false>
    gru_b     rows 320..383, weight rows 128..191, b_off 128, mask + accum + stats (the last block)   <32, false, false>
              (engine.py, _gru backward: blocks (d, r0, m) = (1, 0, 128) and (1, 128, 64), a_m_off = 3 H d + r0)

trunet_conv_wgrad on its own (WGRAD_SIGS; `two` = dz through the BatchNorm backward); instance reached:

    enc128 (the signature above)       two / plain   conv_wgrad_kernel<true> / <false>
    ct_taps   64 <- 5 taps of 64 BN, pos_div 2      two      conv_wgrad_kernel<true>
    m192      192 <- 128 BN                         plain    conv_wgrad_kernel<false>
    thin_pw   8 <- [64 BN | 64 plain]               two      conv_wgrad_kernel<true>  (64 channels: not a thin stream)
    first_taps 64 <- 5 taps of 4 plain, pos_mul 2   plain    NP % 256 == 0: wgrad_first_kernel<5>; NP = 384: wgrad_small_kernel<4,4,5>
    last_taps  8 <- 5 taps of 8 BN, pos_div 2       plain    NP % 256 == 0: wgrad_last_kernel<5>;  NP = 384: wgrad_small_kernel<8,8,1>
  The four wgrad_small.hip instances store every element of the slot and of the bias row from every block: NaN prefill.
  conv_wgrad_kernel relies on the caller's zero fill (header): its slot is prefilled with zeros.

Tile geometry (derived here, asserted by tests/test_pwbwd_ref_cpu.py): a tile is (position, 32 frames), position slowest;
total = P NP / 32 tiles are dealt to G = trunet_pw_bwd_nparts() / 2 = 256 workgroups, workgroup b owning
[b total / G, (b + 1) total / G); a run is the tiles of one position a workgroup owns; the ring of NB slots is refilled per
run.
    small   (128, 1), (128, 97), (384, 130), (384, 384), (384, 64) at P <= 3: total <= 36 < G, workgroups own 0 or 1 tile,
            most runs start mid-position; N ends in tile 0, 3 (97), 0 (130: chunk 2 holds 2 live frames), and with
            (384, 384) N = NP; (384, 64) has ten tiles wholly beyond N; NP = 384 is an odd multiple of 128
    tiles   (384, 50), (384, 75) join for enc128: with 97 and 130 N ends in each of the four tiles of a 128-frame chunk
    mid     NP = 8320 = 65 x 128: P = 3 -> 780 tiles, 3 or 4 per workgroup (NB and NB + 1 for NB = 3); P = 4 -> 1040, 4 or 5
            (NB and NB + 1 for NB = 4); runs start mid-position and cross into the next one
    big     NP = 16512 = 129 x 128, P = 5 -> 2580 tiles, 10 or 11 per workgroup (>= 2 NB + 1: the ring wraps twice)"""
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

import pwbwd_ref as R  # noqa: E402
from convt_cases import report  # noqa: E402

G = 256
NS = types.SimpleNamespace


def _src(nchan, dL=0, off=0, bn=False, mask=False, stats=False, accum=False, signed=False, mul=1, div=1, L=None, share=None):
    """L: function P -> positions of the source (default P + dL); share: key of the tensor the taps of one conv share"""
    return dict(nchan=nchan, L=L or (lambda P, d=dL: P + d), off=off, bn=bn, mask=mask, stats=stats, accum=accum, signed=signed,
                mul=mul, div=div, share=share)


def _sig(M, srcs, rows=None, a_m_off=0, wrows=None, w_m_off=0, b_off=0, taps=False):
    return dict(M=M, srcs=srcs, rows=rows or M, a_m_off=a_m_off, wrows=wrows or M, w_m_off=w_m_off, b_off=b_off, taps=taps)


_BN = dict(bn=True, mask=True, stats=True)
SIGS = {
    "enc128": _sig(128, [_src(128, accum=True, **_BN)]),
    "plain64": _sig(128, [_src(64, mask=True, accum=True)]),
    "dec_pad": _sig(64, [_src(64, dL=-1, off=-1, **_BN), _src(128)]),
    "dec_crop": _sig(64, [_src(64, dL=2, off=1, **_BN), _src(128)]),
    "plain128": _sig(64, [_src(128, signed=True)]),
    "bn64": _sig(64, [_src(64, **_BN)]),
    "thin8": _sig(8, [_src(64, **_BN), _src(64)]),
    "m96": _sig(96, [_src(128, accum=True, **_BN)]),
    "m32": _sig(32, [_src(128, **_BN)]),
    "m20": _sig(20, [_src(64, **_BN), _src(64)]),
    "gru_a": _sig(128, [_src(128, bn=True, mask=True, accum=True)], rows=384, a_m_off=192, wrows=192, w_m_off=0, b_off=0),
    "gru_b": _sig(64, [_src(128, accum=True, **_BN)], rows=384, a_m_off=320, wrows=192, w_m_off=128, b_off=128),
}
# pw_bwd_kernel<AK, SEC, KSPLIT>
INSTANCE = {"enc128": (64, False, False), "plain64": (64, False, True), "dec_pad": (32, True, False),
            "dec_crop": (32, True, False), "plain128": (32, False, False), "bn64": (32, False, True),
            "thin8": (16, False, False), "m96": (64, False, False), "m32": (16, False, False), "m20": (16, False, False),
            "gru_a": (64, False, False), "gru_b": (32, False, False)}
# trunet_conv_wgrad only: the taps of a stride-2 transposed conv (q = (p + 1 - k) / 2, P = 2 L + 1) and of the strided first
# conv (q = 2 p + k - 1, L = 2 P + 1) share one tensor; woff = tap; weight layouts as engine.py passes them: Conv1d (M, C, k):
# ldw_m = 5 C, ldw_c = 5 (taps = "conv"); ConvTranspose1d (C, M, k): ldw_m = 5, ldw_c = 5 M (taps = "convt")
WGRAD_SIGS = {
    "ct_taps": _sig(64, [_src(64, off=1 - k, div=2, bn=True, L=lambda P: (P - 1) // 2, share="a") for k in range(5)], taps="convt"),
    "first_taps": _sig(64, [_src(4, off=k - 1, mul=2, signed=True, L=lambda P: 2 * P + 1, share="x") for k in range(5)], taps="conv"),
    "last_taps": _sig(8, [_src(8, off=1 - k, div=2, bn=True, L=lambda P: (P - 1) // 2, share="a") for k in range(5)], taps="convt"),
    "m192": _sig(192, [_src(128, bn=True)]),
    "thin_pw": _sig(8, [_src(64, bn=True), _src(64)]),
}
# shapes trunet_pw_bwd refuses (tests/test_pwbwd_gpu.py): M = 160; 3, 5 and 8 source row tiles; M <= 32 without four row
# tiles; six row tiles under 128 rows; statistics on a segment that reaches row tile 4 or 5
REFUSED_SIGS = {
    "m160": _sig(160, [_src(128, **_BN)]),
    "k96": _sig(64, [_src(96, **_BN)]),
    "k160": _sig(64, [_src(32, **_BN), _src(128)]),
    "k256": _sig(64, [_src(128, **_BN), _src(128)]),
    "m8k64": _sig(8, [_src(64, **_BN)]),
    "m128k192": _sig(128, [_src(64, **_BN), _src(128)]),
    "stats_tile4": _sig(64, [_src(128), _src(64, **_BN)]),
}
ALL_SIGS = dict(SIGS, **WGRAD_SIGS, **REFUSED_SIGS)

SMALL_NPN = ((128, 1, 1), (128, 97, 3), (384, 130, 2), (384, 384, 1), (384, 64, 2))      # (NP, N, P)
TILE_NPN = ((384, 50, 2), (384, 75, 2))
MID_NP, MID_N, BIG_NP, BIG_N = 8320, 8290, 16512, 16450
REGIMES = ("ordinary", "exact", "zero_cotangent")
# BN channels every regime carries: c0 = 0 always on / always off / pre == 0 everywhere; c0 = 1/2, c1 = -1/4 with x = 1/2
# planted (pre == 0 at some elements: `>` against `>=`); |c1| > 65536 |c0| (always on; the statistics' slow path)
ON_CH, OFF_CH, ZERO_AT_CH, RATIO_CH, ZERO_CH = 2, 6, 10, 14, 18


def small_p(sig, P):
    return max(P, 2) if sig == "dec_pad" else P            # the shifted source has L = P - 1 >= 1


ORDINARY_SMALL = [(s, "ordinary", NP, N, small_p(s, P)) for s in SIGS for NP, N, P in SMALL_NPN]
ORDINARY_SMALL += [("enc128", "ordinary") + t for t in TILE_NPN]
EXACT = [(s, "exact", NP, N, small_p(s, P)) for s in SIGS for NP, N, P in ((384, 130, 2), (128, 97, 2))]
ZERO = [(s, "zero_cotangent", 384, 130, 2) for s in SIGS]
SMALL = ORDINARY_SMALL + EXACT + ZERO
MID = [("enc128", "ordinary", MID_NP, MID_N, 3), ("plain64", "ordinary", MID_NP, MID_N, 3),
       ("plain128", "ordinary", MID_NP, MID_N, 4), ("thin8", "ordinary", MID_NP, MID_N, 4)]
BIG = [("dec_crop", "ordinary", BIG_NP, BIG_N, 5), ("bn64", "ordinary", BIG_NP, BIG_N, 5)]
CASES = SMALL + MID + BIG
# (case, two): P = 5 for the transposed taps (L = 2), 3 for the strided ones (L = 7)
WGRAD_CASES = [(("enc128", r, 384, 130, 2), two) for r in ("ordinary", "exact") for two in (True, False)]
WGRAD_CASES += [(("enc128", "ordinary", MID_NP, MID_N, 3), True)]
WGRAD_CASES += [((s, r, NP, N, P), two) for s, two, P in (("ct_taps", True, 5), ("m192", False, 2), ("thin_pw", True, 2),
                                                          ("first_taps", False, 3), ("last_taps", False, 5))
                for r in ("ordinary", "exact") for NP, N in ((256, 200), (384, 300))]
WGRAD_NAN_PREFILL = ("first_taps", "last_taps")            # the wgrad_small.hip instances write every element themselves


def case_id(case):
    return "%s-%s-NP%d-N%d-P%d" % case


def is_small(case):
    return case[2] <= 1024


# ---------------------------------------------------------------------------------------------- geometry
def nb_of(sig):
    """ring depth trunet_pw_bwd picks (pw_bwd.hip, host code: rows, slot, fixed, NB)"""
    s = ALL_SIGS[sig]
    MA = R.padded_rows(s["M"])
    ntot = sum(x["nchan"] for x in s["srcs"])
    ksplit = sum(x["nchan"] // 32 for x in s["srcs"]) == 2
    rows = 2 * MA + ntot
    slot = rows * R.TILE * 4
    fixed = (MA + ntot) * 16 + ntot * 8 + (2 * 2 * 2 * 8 * 64 * 4 if ksplit else 0)
    return min(4, (160 * 1024 - fixed) // slot)


def tile_ranges(NP, P, grid=G):
    total = P * (NP // R.TILE)
    return [((b * total) // grid, ((b + 1) * total) // grid) for b in range(grid)]


def tiles_owned(NP, P, grid=G):
    return torch.tensor([t1 - t0 for t0, t1 in tile_ranges(NP, P, grid)])


def kinds(NP, P, NB, grid=G):
    """the kinds of workgroup a launch holds"""
    nfc = NP // R.TILE
    out = set()
    for t0, t1 in tile_ranges(NP, P, grid):
        n = t1 - t0
        for name, hit in (("0", n == 0), ("1", n == 1), ("NB", n == NB), ("NB+1", n == NB + 1), (">=2NB+1", n >= 2 * NB + 1),
                          ("mid_start", n > 0 and t0 % nfc != 0), ("crossing", n > 0 and (t1 - 1) // nfc > t0 // nfc)):
            if hit:
                out.add(name)
    return out


# ---------------------------------------------------------------------------------------------- inputs
W_TAIL = 64                # the image is this much longer than the weight


def _gen(dev, *key):
    return torch.Generator(device=dev).manual_seed(int(hashlib.sha1(repr(key).encode()).hexdigest()[:8], 16))


def inputs(case, dev="cpu"):
    sig, regime, NP, N, P = case
    sd = ALL_SIGS[sig]
    M, srcs, rows = sd["M"], sd["srcs"], sd["rows"]
    g = _gen(dev, "pwbwd", case)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32, device=dev)
    un = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g, dtype=torch.float32, device=dev)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g, device=dev).float()
    pick = lambda vals, n: torch.tensor(vals, dtype=torch.float32, device=dev)[torch.randint(0, len(vals), (n,), generator=g, device=dev)]
    exact = regime == "exact"
    taps = sd["taps"]
    K = srcs[0]["nchan"] * len(srcs) if taps else sum(s["nchan"] for s in srcs)
    c = NS(case=case, sig=sig, regime=regime, M=M, N=N, NP=NP, P=P, K=K, p_begin=0, a_L=P, a_pos_off=0, a_m_off=sd["a_m_off"],
           bnbwd=True, ldw_m=len(srcs) if taps == "convt" else K, ldw_c={"convt": M * len(srcs), "conv": len(srcs), False: 1}[taps],
           w_m_off=sd["w_m_off"], b_off=sd["b_off"],
           b_len=sd["b_off"] + M + 8, w_numel=sd["wrows"] * K + W_TAIL)
    assert not taps or sd["wrows"] == M
    if exact:
        # dz = ca dy + cb z + cc lies on the 2^-8 grid with |dz| <= 5 (11 bits), W on the 1/4 grid and three quarters of it
        # zero, x, c1, mean, prev on the 1/8 grid, c0 in {1, -1, 1/2}: pre = c0 x + c1 on the 1/16 grid, |pre| <= 2.5.  No
        # operand of a product has more than 16 significant bits: its three-term split has lo = 0, so the products the
        # split drops (mid lo, lo mid, lo lo) are zero and the six it keeps are exact
        c.dy, c.z = ri(-32, 32, rows, P, NP) / 16, ri(-32, 32, rows, P, NP) / 16
        c.ca, c.cb, c.cc = pick([1.0, 1.5, 0.5, -1.0], rows), pick([0.25, -0.25, 0.5, 0.0], rows), ri(-256, 256, rows) / 256
        c.W = ri(-4, 4, c.w_numel) / 4 * (torch.rand(c.w_numel, generator=g, device=dev) < 0.25).float()
    else:
        c.dy, c.z = rn(rows, P, NP), rn(rows, P, NP)
        c.ca, c.cb, c.cc = un(0.5, 1.5, rows), 0.2 * rn(rows), 0.1 * rn(rows)
        c.W = 0.1 * rn(c.w_numel)
    if regime == "zero_cotangent":
        c.dy, c.cb, c.cc = torch.zeros_like(c.dy), torch.zeros_like(c.cb), torch.zeros_like(c.cc)
    c.segs, woff, shared = [], 0, {}
    mixed = any(s["bn"] for s in srcs)
    for k, s_ in enumerate(srcs):
        n, L = s_["nchan"], s_["L"](P)
        s = NS(nchan=n, L=L, pos_mul=s_["mul"], pos_off=s_["off"], pos_div=s_["div"], woff=k if taps else woff, bn=s_["bn"],
               store=not taps and sig not in WGRAD_SIGS, mask=s_["mask"], stats=s_["stats"], accum=s_["accum"])
        woff += n
        if s_["share"] in shared:
            o = shared[s_["share"]]
            s.x, s.prev, s.c0, s.c1, s.mean = o.x, o.prev, o.c0, o.c1, o.mean
            c.segs.append(s)
            continue
        if exact:
            s.x, s.prev = ri(-12, 12, n, L, NP) / 8, ri(-16, 16, n, L, NP) / 8
            s.c0, s.c1, s.mean = pick([1.0, -1.0, 0.5], n), ri(-8, 8, n) / 8, ri(-4, 4, n) / 8
        else:
            s.x, s.prev = rn(n, L, NP), rn(n, L, NP)
            s.c0, s.c1, s.mean = un(0.5, 1.5, n), 0.5 * rn(n), 0.3 * rn(n)
            s.c0[1::4] *= -1                                   # every fourth channel: a negative BatchNorm weight
        if s.bn:
            for ch, k0, k1 in ((ON_CH, 0.0, 0.5), (OFF_CH, 0.0, -0.5), (ZERO_AT_CH, 0.5, -0.25), (RATIO_CH, 2.0 ** -17, 1.0),
                               (ZERO_CH, 0.0, 0.0)):
                if ch < n:
                    s.c0[ch], s.c1[ch] = k0, k1
            if ZERO_AT_CH < n:
                s.x[ZERO_AT_CH, :, ::7] = 0.5
            if RATIO_CH < n and exact:
                s.x[RATIO_CH] = 0.0           # c0 x would need 21 significant bits next to c1 = 1: this regime keeps pre = 1
        else:
            s.c0, s.c1, s.mean = torch.ones(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
            if mixed or not s_["signed"]:
                s.x = s.x.clamp_min(0)                         # a post-ReLU tensor: about half of it exactly 0
        if s_["share"] is not None:
            shared[s_["share"]] = s
        c.segs.append(s)
    return c


def to_device(c, dev):
    """the case with every tensor on `dev` (the restatement runs where its inputs are)"""
    mv = lambda o: NS(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in vars(o).items() if k != "segs"})
    out = mv(c)
    out.segs = [mv(s) for s in c.segs]
    return out


def refs(c, seq=True, dev="cpu"):
    """the float64 reference and the yardstick: element by element the worse of the fp32 orders `blocked` and `seq`
    (`blocked` alone with seq = False: the mid and big cases, the tighter choice)"""
    cd = to_device(c, dev)
    cpu = lambda o: {k: v.cpu() for k, v in o.items()}
    c.ref64 = cpu(R.pw_bwd(cd, torch.float64))
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
    """the case as trunet_conv_wgrad sees it: no data gradient; two = False: dz is dy as it is (TRUNET_PRO_NONE)"""
    w = to_device(c, c.dy.device)
    for s in w.segs:
        s.store = s.mask = s.stats = s.accum = False
    w.bnbwd = two
    return w


# ---------------------------------------------------------------------------------------------- launches
SENT = 7.5                 # sentinel around the weight slot and the bias row, and behind every out[s]
W_OFF = 96                 # the weight slot starts 96 floats into its image
B_BASE, B_TAIL = 16, 24
NAN = float("nan")
DEV = "cuda"


def _dev(t):
    return t.to(DEV).contiguous()


def written_cols(c):
    """sorted element indices of the image a launch must write"""
    return torch.unique(torch.cat([R.w_index(c, s).reshape(-1) for s in c.segs]))


def _seg(Lb, s, x, keep, **over):
    sg = Lb.Seg()
    sg.src0 = Lb.ptr(x)
    sg.nchan, sg.L, sg.pos_mul, sg.pos_off, sg.pos_div, sg.woff = s.nchan, s.L, s.pos_mul, s.pos_off, s.pos_div, s.woff
    sg.mode = Lb.PRO_BNRELU if s.bn else Lb.PRO_NONE
    if s.bn:
        k = keep[1].setdefault(id(s.c0), dict(c0=_dev(s.c0), c1=_dev(s.c1)))      # taps share their coefficient arrays
        sg.c0, sg.c1 = Lb.ptr(k["c0"]), Lb.ptr(k["c1"])
    for k, v in over.items():
        setattr(sg, k, v)
    return sg


def _wgrad_common(Lb, aw, c, keep, prefill, bias):
    """fills the trunet_wgrad_args half; returns (wimg [G][W_OFF + w_numel], bimg [G][B_BASE + b_len + B_TAIL])"""
    grid = G
    stride = W_OFF + c.w_numel
    aw.NP, aw.N, aw.P, aw.p_begin, aw.M, aw.a_L, aw.a_pos_off, aw.a_m_off = c.NP, c.N, c.P, c.p_begin, c.M, c.a_L, c.a_pos_off, c.a_m_off
    aw.a_mode = Lb.PRO_BNBWD if c.bnbwd else Lb.PRO_NONE
    aw.ldw_m, aw.ldw_c, aw.w_m_off, aw.nseg, aw.w_numel = c.ldw_m, c.ldw_c, c.w_m_off, len(c.segs), stride
    t = [_dev(c.dy), _dev(c.z), _dev(c.ca), _dev(c.cb), _dev(c.cc)]
    keep[0].extend(t)
    aw.a0 = Lb.ptr(t[0])
    if c.bnbwd:
        aw.a1, aw.ac0, aw.ac1, aw.ac2 = Lb.ptr(t[1]), Lb.ptr(t[2]), Lb.ptr(t[3]), Lb.ptr(t[4])
    wimg = torch.full((grid, stride), SENT, device=DEV, dtype=torch.float32)
    wimg[:, W_OFF + written_cols(c).to(DEV)] = prefill
    bimg = torch.full((grid, B_BASE + c.b_len + B_TAIL), SENT, device=DEV, dtype=torch.float32)
    bimg[:, B_BASE + c.b_off:B_BASE + c.b_off + c.M] = NAN
    aw.w_partials = Lb.ptr(wimg) + 4 * W_OFF
    aw.b_partials = Lb.ptr(bimg) + 4 * B_BASE if bias else None
    aw.b_stride, aw.b_off = bimg.shape[1], c.b_off
    return wimg, bimg


def pw_bwd_args(c, prezero=False, bias=True):
    """the argument block of trunet_pw_bwd for the case, every output prefilled: weight slot, bias row, statistics rows (zero
    with prezero, which the call is then told) and the visited positions of a never-accumulated out[s] with NaN; the other
    positions of out[s] with `prev`; 8 guard floats behind every out[s].  Returns (args, buffers)."""
    from tinyrecurrentunet_amd import _lib as Lb
    lib = Lb.lib()
    nparts = lib.trunet_pw_bwd_nparts()
    assert nparts == 2 * G and lib.trunet_conv_wgrad_nparts() == G, nparts
    keep = ([], {})
    a = Lb.PwBwdArgs()
    wimg, bimg = _wgrad_common(Lb, a.w, c, keep, NAN, bias)
    Wd = _dev(c.W)
    keep[0].append(Wd)
    a.W = Lb.ptr(Wd)
    outs, parts, xs = [], [], []
    for i, s in enumerate(c.segs):
        x = _dev(s.x)
        xs.append(x)
        a.w.seg[i] = _seg(Lb, s, x, keep)
        pre = s.prev.clone()
        if not s.accum:
            pre[:, R.positions(s, c)[1]] = NAN
        o = torch.cat([pre.reshape(-1), torch.full((8,), SENT, dtype=torch.float32, device=pre.device)]).to(DEV)
        outs.append(o)
        d = a.dg[i]
        d.out = Lb.ptr(o)
        fl = Lb.DG_STORE | (Lb.DG_MASK if s.mask else 0) | (Lb.DG_ACCUM if s.accum else 0)
        if s.mask:
            d.zmask = Lb.ptr(x)
        part = None
        if s.stats:
            fl |= Lb.DG_STATS | (Lb.DG_PREZERO if prezero else 0)
            part = torch.full((nparts, s.nchan, 2), 0.0 if prezero else NAN, device=DEV, dtype=torch.float32)
            mean = _dev(s.mean)
            keep[0].append(mean)
            d.e2, d.partials = Lb.ptr(mean), Lb.ptr(part)
        parts.append(part)
        d.flags = fl
    return a, NS(keep=keep, xs=xs, wimg=wimg, bimg=bimg if bias else None, outs=outs, parts=parts)


def _collect(c, b, own=None):
    n = lambda s: s.nchan * s.L * c.NP
    return NS(wimg=b.wimg.cpu(), bimg=None if b.bimg is None else b.bimg.cpu(),
              out=[o.cpu()[:n(s)].view(s.nchan, s.L, c.NP) for o, s in zip(getattr(b, "outs", []), c.segs)],
              guard=[o.cpu()[n(s):] for o, s in zip(getattr(b, "outs", []), c.segs)],
              parts=[None if p is None else p.cpu() for p in getattr(b, "parts", [])],
              own=tiles_owned(c.NP, c.P) > 0 if own is None else own)


def with_mfma(x3, fn):
    """fn() with the fused backward kernels on the three-term bf16 split (x3) or on the fp32 MFMA; the mode is restored"""
    from tinyrecurrentunet_amd import _lib as Lb
    lib = Lb.lib()
    prev = lib.trunet_gemm_x3_enable(Lb.X3_BWD if x3 else 0)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.trunet_gemm_x3_enable(prev)
    return out


def gpu_pw_bwd(c, x3=True, prezero=False, bias=True):
    """one launch of trunet_pw_bwd; returns CPU tensors: wimg [G][W_OFF + w_numel], bimg [G][..] (None with bias = False),
    out[s] [nchan][L][NP], guard[s] [8], parts[s] [2 G][nchan][2] or None, own bool [G]"""
    from tinyrecurrentunet_amd import _lib as Lb
    a, b = pw_bwd_args(c, prezero, bias)
    with_mfma(x3, lambda: Lb.check(Lb.lib().trunet_pw_bwd(a, Lb.stream()), "pw_bwd " + case_id(c.case)))
    return _collect(c, b)


def gpu_wgrad(c, bias=True):
    """one launch of trunet_conv_wgrad on the case's weight-gradient view"""
    from tinyrecurrentunet_amd import _lib as Lb
    lib = Lb.lib()
    assert lib.trunet_conv_wgrad_nparts() == G
    keep = ([], {})
    a = Lb.WgradArgs()
    wimg, bimg = _wgrad_common(Lb, a, c, keep, NAN if c.sig in WGRAD_NAN_PREFILL else 0.0, bias)
    shared = {}
    for i, s in enumerate(c.segs):
        if id(s.x) not in shared:
            shared[id(s.x)] = _dev(s.x)
        a.seg[i] = _seg(Lb, s, shared[id(s.x)], keep)
    Lb.check(lib.trunet_conv_wgrad(a, Lb.stream()), "conv_wgrad " + case_id(c.case))
    torch.cuda.synchronize()
    # (how trunet_conv_wgrad's kernels deal their work is not restated here: no image is expected to be all zero)
    return _collect(c, NS(wimg=wimg, bimg=bimg if bias else None), own=torch.ones(G, dtype=torch.bool))


# ---------------------------------------------------------------------------------------------- comparison and report
def sums(c, o):
    """the outputs of a launch under the restatement's names: partial images, bias rows and statistics rows summed in
    float64; what the launch must not write counts as zero here and is held to the sentinel by `exactness`"""
    cols = written_cols(c)
    dW = torch.zeros(c.w_numel, dtype=torch.float64)
    dW[cols] = o.wimg[:, W_OFF + cols].double().sum(0)
    out = {"dW": dW}
    if o.bimg is not None:
        db = torch.zeros(c.b_len, dtype=torch.float64)
        db[c.b_off:c.b_off + c.M] = o.bimg[:, B_BASE + c.b_off:B_BASE + c.b_off + c.M].double().sum(0)
        out["db"] = db
    for i, g in enumerate(o.out):
        out["g%d" % i] = g
        if o.parts[i] is not None:
            out["st0_%d" % i], out["st1_%d" % i] = o.parts[i][:, :, 0].double().sum(0), o.parts[i][:, :, 1].double().sum(0)
    return out


def compare(tag, c, got, names):
    """every output through `close`; exact: equal bits as well (the sums' float64 value IS the fp32 value).  Every figure
    is printed BEFORE the first assertion fires; returns {name: (err, e_y, bound, rel, rel_bound)}."""
    res, fails = {}, []
    for k in names:
        r64 = c.ref64[k]
        e_y, bnd, rel_y, rbnd = R.bound(r64, c.yard[k])
        d = got[k].double() - r64
        res[k] = (float(d.abs().max()), e_y, bnd, float(d.norm()) / (float(r64.norm()) + 1e-300), rbnd)
        try:
            R.close(got[k], r64, c.yard[k], "%s %s" % (tag, k))
        except AssertionError as e:
            fails.append(str(e))
        if c.regime == "exact" and not torch.equal(got[k].double(), r64):
            bad = got[k].double() != r64
            fails.append("%s %s: %d of %d elements differ from the exact value, max error %.3e" %
                         (tag, k, int(bad.sum()), bad.numel(), res[k][0]))
    report("%s: err / e_y / bound / rel / rel_bound  " % tag + "  ".join("%s %.2e/%.2e/%.2e/%.2e/%.2e" % ((n,) + res[n]) for n in res),
           "parity_pwbwd.txt")
    assert not fails, "\n".join(fails)
    return res


def mask64(s):
    """[nchan][L][NP] bool: where the data gradient passes.  c0 x is exact in float64 (24 x 24 bits) and the sum is rounded
    once: the sign is the exact value's, as the kernel's correctly rounded fmaf's is"""
    return (s.c0.double()[:, None, None] * s.x.double() + s.c1.double()[:, None, None]) > 0


def exactness(c, o, tag):
    """what must hold bit for bit in every regime: nothing left unwritten, nothing written outside the slots, untouched
    positions, exact zeros where the contract has zeros"""
    M, N = c.M, c.N
    cols = written_cols(c)
    img = o.wimg[:, W_OFF:]
    slot = img[:, cols]
    rest = torch.ones(img.shape[1], dtype=torch.bool)
    rest[cols] = False
    assert not bool(torch.isnan(slot).any()), "%s: weight images have unwritten (NaN) elements" % tag
    assert bool((o.wimg[:, :W_OFF] == SENT).all()) and bool((img[:, rest] == SENT).all()), \
        "%s: a write outside the weight elements of the launch" % tag
    assert bool((slot[~o.own] == 0).all()), "%s: weight images of workgroups without tiles are not exactly 0" % tag
    zc = c.regime == "zero_cotangent"
    if o.bimg is not None:
        b0 = B_BASE + c.b_off
        row = o.bimg[:, b0:b0 + M]
        assert not bool(torch.isnan(row).any()), "%s: bias rows have unwritten (NaN) elements" % tag
        assert bool((o.bimg[:, :b0] == SENT).all()) and bool((o.bimg[:, b0 + M:] == SENT).all()), \
            "%s: a write outside the bias row" % tag
        assert bool((row[~o.own] == 0).all()), "%s: bias rows of workgroups without tiles are not exactly 0" % tag
        assert not zc or bool((row == 0).all()), "%s: zero cotangent, non-zero bias gradient" % tag
    assert not zc or bool((slot == 0).all()), "%s: zero cotangent, non-zero weight gradient" % tag
    for i, s in enumerate(c.segs if o.out else []):
        g, prev = o.out[i], s.prev.cpu()
        assert not bool(torch.isnan(g).any()), "%s: out[%d] has unwritten (NaN) elements" % (tag, i)
        assert bool((o.guard[i] == SENT).all()), "%s: a write behind out[%d]" % (tag, i)
        vis = torch.zeros(s.L, dtype=torch.bool)
        vis[R.positions(s, c)[1]] = True
        assert torch.equal(g[:, ~vis].view(torch.int32), prev[:, ~vis].view(torch.int32)), \
            "%s: out[%d] changed at a position no p reaches" % (tag, i)
        keep = mask64(NS(c0=s.c0.cpu(), c1=s.c1.cpu(), x=s.x.cpu())) if s.mask else torch.ones_like(g, dtype=torch.bool)
        assert bool((g[:, vis][~keep[:, vis]] == 0).all()), "%s: out[%d]: a masked element is not exactly 0" % (tag, i)
        left = torch.where(keep, prev, torch.zeros(())) if s.accum else torch.zeros_like(g)      # what dz = 0 leaves
        fr = slice(0, None) if zc else slice(N, None)
        assert torch.equal(g[:, vis][:, :, fr], left[:, vis][:, :, fr]), \
            "%s: out[%d] is not mask(prev) / 0 %s" % (tag, i, "everywhere" if zc else "for frames >= N")
        if s.stats:
            pt = o.parts[i]
            assert not bool(torch.isnan(pt).any()), "%s: statistics rows %d have unwritten (NaN) elements" % (tag, i)
            assert bool((pt[(~o.own).repeat_interleave(2)] == 0).all()), \
                "%s: statistics rows %d of workgroups without tiles are not exactly 0" % (tag, i)
            if zc and not s.accum:
                assert bool((pt == 0).all()), "%s: zero cotangent, non-zero statistics" % tag
            for ch in (OFF_CH, ZERO_CH):
                if s.bn and ch < s.nchan:
                    assert bool((g[ch][vis] == 0).all()) and bool((pt[:, ch] == 0).all()), \
                        "%s: out[%d] channel %d (pre <= 0 everywhere) is not exactly 0" % (tag, i, ch)


def same_bits(o1, o2, what, skip=()):
    for k in ("wimg", "bimg"):
        if k not in skip:
            assert torch.equal(getattr(o1, k).view(torch.int32), getattr(o2, k).view(torch.int32)), "%s: %s differs" % (what, k)
    for i in range(len(o1.out)):
        assert torch.equal(o1.out[i].view(torch.int32), o2.out[i].view(torch.int32)), "%s: out[%d] differs" % (what, i)
        if o1.parts[i] is not None:
            assert torch.equal(o1.parts[i].view(torch.int32), o2.parts[i].view(torch.int32)), "%s: statistics rows %d differ" % (what, i)


def check_case(c, x3):
    """one launch of the fused entry point: every output against the restatement, then the exactness assertions"""
    o = gpu_pw_bwd(c, x3)
    ak, sec, ks = INSTANCE[c.sig]
    tag = "PWBWD <%d,%d,%d,%s> NB %d %s" % (ak, sec, ks, "x3" if x3 else "f32", nb_of(c.sig), case_id(c.case))
    res = compare(tag, c, sums(c, o), R.outputs(c))
    exactness(c, o, tag)
    return res, o


def check_wgrad(c, two):
    """one launch of trunet_conv_wgrad on the same inputs: dW and db against the restatement of its view of the case"""
    w = refs(wgrad_view(c, two), seq=is_small(c.case), dev=c.dy.device)
    o = gpu_wgrad(w)
    tag = "WGRAD %s %s" % ("bn-backward dz" if two else "plain dz", case_id(c.case))
    res = compare(tag, w, sums(w, o), ["dW", "db"])
    exactness(w, o, tag)
    return res
