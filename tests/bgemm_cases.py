"""The bf16 forward / data-gradient GEMM (trunet_bf16_gemm) through the C ABI against tests/bgemm_ref.py: layer signatures,
input regimes, tile geometry, launch helpers and the case functions tests/test_bgemm_gpu.py calls.

A case is (signature, regime, NP, N, P).  Inputs come from seeded CPU generators keyed by the case; frames >= N hold live
random values (the kernel must ignore them in the statistics and still store the rows there).

Tile geometry: a tile is (position, 64 frames), position fastest; total = P NP / 64 tiles.  BG_GRID = 512 workgroups of 4
waves; a tile is computed by one wave (tslots = 4 tile slots per workgroup) or, where two waves split more than 64 rows
(the instances with NRT = 2 at more than two row tiles), by two (tslots = 2).  Slot w of 512 tslots owns the tiles w,
w + 512 tslots, ...  The list is laid out for that grid (trunet_bf16_gemm_nparts() == 2048, asserted by the GPU test):
    small   (64, 1), (64, 32), (64, 33), (128, 128), (192, 130), (192, 64) at P in {1, 3}: at most 9 tiles; a last tile
            with 1 or 2 live frames, N on the 32-frame column-block edge, N = NP, a 64-frame chunk wholly beyond N
    wrap    total just above one sweep of the slots and no multiple of it: some slots own 2 tiles, most own 1 (the second
            trip of the tile loop, statistics accumulated over two tiles, the stride, the chunk / position wrap):
            NP = 44032, P = 3 (2064 > 2048) for an unsplit 64-row signature with statistics and for the one-wave 128-row
            forward; NP = 22016, P = 3 (1032 > 1024) for the split 128-row data gradient; NP = 26368, P = 5 (2060), where
            the position wrap and the chunk change fall inside one slot's stride"""
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

import bgemm_ref as R  # noqa: E402
from convt_cases import from_octets, report, to_octets  # noqa: E402
from pwbwd16_cases import to_device  # noqa: E402

NS = types.SimpleNamespace
GRID, NPARTS = 512, 2048
B, S, A, K, RL, F, PREZERO = 1, 2, 4, 8, 16, 32, 64          # TRUNET_EPI_*
NONE, BNRELU, BNBWD = R.NONE, R.BNRELU, R.BNBWD
PARITY = "parity_bgemm.txt"


def _sg(nchan, mode=NONE, L=lambda P: P, mul=1, off=0, div=1, woff=0, signed=False):
    return dict(nchan=nchan, mode=mode, L=L, mul=mul, off=off, div=div, woff=woff, signed=signed)


def _sig(M, segs, epi, inst, ldw_m=None, ldw_c=1, w_m_off=0, p_begin=0, dout=0, out_pos_off=0, chunks=(0,), min_P=1):
    """inst: the template instance (nrt, pro, epi, full) the launch must reach; out_L = P + dout"""
    Kc = sum(s["nchan"] for s in segs)
    return NS(M=M, segs=segs, epi=epi, inst=inst, ldw_m=Kc if ldw_m is None else ldw_m, ldw_c=ldw_c, w_m_off=w_m_off,
              p_begin=p_begin, dout=dout, out_pos_off=out_pos_off, chunks=chunks, min_P=min_P)


def _taps(nchan, Kt, S_, mode=BNRELU):
    """ConvTranspose1d(k = Kt, stride S_, padding S_ / 2) as tap segments: output position p reads source position
    (p + pad - k) / S_; weight [ci][co][k]"""
    return [_sg(nchan, mode, L=lambda P, S_=S_: (P + S_ - 1) // S_, off=S_ // 2 - k, div=S_, woff=k) for k in range(Kt)]


def _convt(M, nchan, Kt, S_, epi, inst):
    # the launch owns the P positions in the middle of an output of P + 2
    return _sig(M, _taps(nchan, Kt, S_), epi, inst, ldw_m=Kt, ldw_c=M * Kt, dout=2, out_pos_off=1)


def _dgrad(M, epi, inst, nchan=64, shifted=False):
    """data gradient of a pointwise layer: BatchNorm backward of (dy, z) [nchan] through the transposed weight
    W[nchan][64 + M]; shifted: the F.pad source -- positions 1 .. P of dy make positions 0 .. P - 1 of the gradient"""
    seg = [_sg(nchan, BNBWD, L=(lambda P: P + 1) if shifted else (lambda P: P))]
    if shifted:
        return _sig(M, seg, epi, inst, ldw_m=1, ldw_c=64 + M, w_m_off=0, p_begin=1, out_pos_off=-1)
    return _sig(M, seg, epi, inst, ldw_m=1, ldw_c=64 + M, w_m_off=64)


GEN1, GEN2 = (1, -1, -1, 0), (2, -1, -1, 0)
# the layers as engine_bf16.py launches them ...
SIGS = {
    "enc128": _sig(128, [_sg(128, BNRELU)], B | S, (4, BNRELU, B | S, 1)),
    "plain128": _sig(128, [_sg(64, signed=True)], B | S, (4, NONE, B | S, 1)),
    "pw64": _sig(64, [_sg(128, BNRELU)], B | S, (2, BNRELU, B | S, 1)),
    "plain64": _sig(64, [_sg(64, signed=True)], B | S, (2, NONE, B | S, 1)),
    "dec_pad": _sig(64, [_sg(64, BNRELU, L=lambda P: P - 1, off=-1), _sg(128, woff=64)], B | S, (2, BNRELU, B | S, 1), min_P=2),
    "dec_crop": _sig(64, [_sg(64, BNRELU, L=lambda P: P + 2, off=1), _sg(128, woff=64)], B | S, (2, BNRELU, B | S, 1)),
    "convt_k3s1": _convt(64, 64, 3, 1, B | S, (2, BNRELU, B | S, 1)),
    "convt_k5s2": _convt(64, 64, 5, 2, B | S, (2, BNRELU, B | S, 1)),
    "convt_k3s2": _convt(64, 64, 3, 2, B | S, (2, BNRELU, B | S, 1)),
    # first conv 64 <- 4 channels x 5 taps, stride 2: position p reads 2 p + k - 1; weight [co][ci][k]
    "first": _sig(64, [_sg(4, L=lambda P: 2 * P + 1, mul=2, off=k - 1, woff=k, signed=True) for k in range(5)], B | RL,
                  (2, NONE, B | RL, 0), ldw_m=20, ldw_c=5),
    "dec5_pw": _sig(8, [_sg(64, BNRELU), _sg(64, woff=64)], B | S, (1, BNRELU, B | S, 0)),
    "dec5_ct": _convt(8, 8, 5, 2, B, (1, BNRELU, B, 0)),
    # GRU input projection: three 128-row launches over one 384-row weight into one fp32 buffer
    "gru_proj": _sig(128, [_sg(128, BNRELU)], B | F, (4, BNRELU, B | F, 1), chunks=(0, 128, 256)),
    "dg128_KS": _dgrad(128, K | S, (2, BNBWD, K | S, 1)),
    "dg128_KSA": _dgrad(128, K | S | A, (2, BNBWD, K | S | A, 1)),
    "dg128_KA": _dgrad(128, K | A, (2, BNBWD, K | A, 1)),
    "dg128_0": _dgrad(128, 0, (2, BNBWD, 0, 1)),
    "dg64_KS": _dgrad(64, K | S, (2, BNBWD, K | S, 1), shifted=True),
    "dg64_KSA": _dgrad(64, K | S | A, (2, BNBWD, K | S | A, 1), shifted=True),
    "dg64_KA": _dgrad(64, K | A, (2, BNBWD, K | A, 1), shifted=True),
    "dg64_0": _dgrad(64, 0, (2, BNBWD, 0, 1), shifted=True),
    "plain_KS64": _sig(64, [_sg(64, signed=True)], K | S, (2, NONE, K | S, 1), ldw_m=1, ldw_c=64),
    "plain_KS8": _sig(8, [_sg(8, signed=True)], K | S, (1, NONE, K | S, 0), ldw_m=1, ldw_c=8),
    "dg8_KS": _dgrad(64, K | S, (2, BNBWD, K | S, 0), nchan=8),           # not FULL: 8 dz channels, half a k-step
    "dg8_0": _dgrad(64, 0, (2, BNBWD, 0, 0), nchan=8),
    # ... and contract shapes the network does not use
    "m16": _sig(16, [_sg(32, BNRELU)], B | S | RL, GEN1),
    "m40": _sig(40, [_sg(32, BNRELU)], B | S, GEN2),
    "m44": _sig(44, [_sg(32, signed=True)], B | A, GEN2),                 # M % 8 = 4: the last octet's padded rows, ACCUM
    "m44_KS": _sig(44, [_sg(32, BNBWD)], K | S, (2, BNBWD, K | S, 0), ldw_m=1, ldw_c=44),
    "m72": _sig(72, [_sg(64, BNBWD)], K | S | A, GEN2, ldw_m=1, ldw_c=72),   # 3 row tiles: the second wave of a tile owns one
    "seg24": _sig(64, [_sg(24, BNRELU), _sg(64, woff=24)], B | S, GEN2),     # odd octet count: 2 (ks0 + j) + h < noct
    "seg3x32": _sig(64, [_sg(32, BNRELU, woff=32 * i) for i in range(3)], B | S, (2, BNRELU, B | S, 1)),
    # 24 k-steps, the maximum, over the 5 segments an argument block holds: 4 x 64 + 128 channels
    "nks24": _sig(64, [_sg(64, BNRELU, woff=64 * i) for i in range(4)] + [_sg(128, woff=256)], B | S, (2, BNRELU, B | S, 1)),
    "eval_B": _sig(64, [_sg(64, BNRELU)], B, GEN2),
    "eval_BR": _sig(128, [_sg(64, BNRELU)], B | RL, GEN2),
    "m96_fwd": _sig(96, [_sg(64, BNRELU)], B | S, GEN2),
    "m96_bwd": _sig(96, [_sg(64, BNBWD)], K | S | A, GEN2, ldw_m=1, ldw_c=96),
}
M96 = ("m96_fwd", "m96_bwd")
# every instance of the dispatch in trunet_bf16_gemm
INSTANCES = {(4, BNRELU, B | S, 1), (4, NONE, B | S, 1), (4, BNRELU, B | F, 1), (2, BNRELU, B | S, 1), (2, NONE, B | S, 1),
             (2, NONE, K | S, 1), (2, BNBWD, K | S, 1), (2, BNBWD, K | S | A, 1), (2, BNBWD, K | A, 1), (2, BNBWD, 0, 1),
             (1, BNRELU, B | S, 0), (1, BNRELU, B, 0), (1, NONE, K | S, 0), (2, NONE, B | RL, 0), (2, BNBWD, K | S, 0),
             (2, BNBWD, 0, 0), GEN1, GEN2}

SMALL_NPN = ((64, 1), (64, 32), (64, 33), (128, 128), (192, 130), (192, 64))
REGIMES = ("ordinary", "exact", "zero")
ZERO_PRE_CH, ALWAYS_ON_CH, ALWAYS_OFF_CH, EDGE_CH = 10, 2, 6, 1    # channels (mod the count) with c0 / e0 = 0; `zero`: EDGE_CH


def small_ps(sig):
    return (2, 3) if SIGS[sig].min_P == 2 else (1, 3)


ORDINARY_SMALL = [(s, "ordinary", NP, N, P) for s in SIGS for NP, N in SMALL_NPN for P in small_ps(s)]
EXACT = [(s, "exact", NP, N, P) for s in SIGS for NP, N, P in ((192, 130, 2), (64, 33, 3))]
ZERO = [(s, "zero", 192, 130, 2) for s in SIGS]
SMALL = ORDINARY_SMALL + EXACT + ZERO
WRAP = [("pw64", "ordinary", 44032, 43990, 3), ("enc128", "ordinary", 44032, 43990, 3),
        ("dg128_KSA", "ordinary", 22016, 21990, 3), ("dec_crop", "ordinary", 26368, 26300, 5)]
CASES = SMALL + WRAP


def not_m96(cases):
    return [c for c in cases if c[0] not in M96]


def only_m96(cases):
    return [c for c in cases if c[0] in M96]


def case_id(case):
    return "%s-%s-NP%d-N%d-P%d" % case


def is_small(case):
    return case[2] <= 1024


def tslots(sig):
    s = SIGS[sig]
    return 2 if (s.inst[0] < 4 and (s.M + 31) // 32 > 2) else 4


def tiles_owned(sig, NP, P):
    """[GRID tslots] number of tiles of every slot"""
    total, n = P * (NP // 64), GRID * tslots(sig)
    return torch.tensor([(total - w + n - 1) // n if w < total else 0 for w in range(n)])


def _gen(*key):
    return torch.Generator().manual_seed(int(hashlib.sha1(repr(key).encode()).hexdigest()[:8], 16))


def inputs(case):
    sig, regime, NP, N, P = case
    sd = SIGS[sig]
    g = _gen("bgemm", case)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    un = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g, dtype=torch.float32)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    pick = lambda vals, n: torch.tensor(vals, dtype=torch.float32)[torch.randint(0, len(vals), (n,), generator=g)]
    rb = R.bf16_round
    exact = regime == "exact"
    M, epi = sd.M, sd.epi
    Mp = (M + 7) // 8 * 8
    c = NS(case=case, sig=sig, regime=regime, M=M, N=N, NP=NP, P=P, p_begin=sd.p_begin, out_L=P + sd.dout,
           out_pos_off=sd.out_pos_off, ldw_m=sd.ldw_m, ldw_c=sd.ldw_c, w_m_off=sd.w_m_off, chunks=sd.chunks, epi=epi,
           bias=bool(epi & B), stats=bool(epi & S), accum=bool(epi & A), mask=bool(epi & K), relu=bool(epi & RL),
           f32out=bool(epi & F), inst=sd.inst)

    def special(c0, c1, n):
        for ch, sh in ((ALWAYS_ON_CH, 0.5), (ALWAYS_OFF_CH, -0.5), (ZERO_PRE_CH, 0.0)):
            c0[ch % n], c1[ch % n] = 0.0, sh                   # pre = shift: always on, always off, exactly 0 (> against >=)
    c.segs, wmax = [], 0
    pro = BNBWD if any(s["mode"] == BNBWD for s in sd.segs) else (BNRELU if any(s["mode"] == BNRELU for s in sd.segs) else NONE)
    for s0 in sd.segs:
        n, L = s0["nchan"], s0["L"](P)
        assert L >= 1, (case, L)
        s = NS(nchan=n, L=L, pos_mul=s0["mul"], pos_off=s0["off"], pos_div=s0["div"], woff=s0["woff"], mode=s0["mode"])
        wmax = max(wmax, (M - 1 + sd.w_m_off + sd.chunks[-1]) * sd.ldw_m + (n - 1) * sd.ldw_c + s.woff)
        if s.mode == BNBWD:
            # exact: dz = ca dy + cb z + cc on the 2^-8 grid, |dz| <= 5: up to 11 significant bits, so its bf16 rounding
            # happens and meets ties
            if exact:
                s.x, s.z = ri(-32, 32, n, L, NP) / 16, ri(-32, 32, n, L, NP) / 16
                s.c0, s.c1, s.c2 = pick([1.0, 1.5, 0.5, -1.0], n), pick([0.25, -0.25, 0.5, 0.0], n), ri(-256, 256, n) / 256
            else:
                s.x, s.z = rb(rn(n, L, NP)), rb(rn(n, L, NP))
                s.c0, s.c1, s.c2 = un(0.5, 1.5, n), 0.2 * rn(n), 0.1 * rn(n)
        else:
            # exact: x, c1 on the 1/8 grid, c0 in {1, -1, 1/2, 0}: pre on the 1/16 grid, |pre| <= 2.5 (6 bits)
            s.x = ri(-12, 12, n, L, NP) / 8 if exact else rb(rn(n, L, NP))
            if s.mode == BNRELU:
                if exact:
                    s.c0, s.c1 = pick([1.0, -1.0, 0.5, 0.0], n), ri(-8, 8, n) / 8
                else:
                    s.c0, s.c1 = un(0.5, 1.5, n), 0.5 * rn(n)
                    s.c0[1::4] *= -1                               # every fourth channel: a negative BatchNorm weight
                special(s.c0, s.c1, n)
                if regime == "zero":                               # pre exactly 0 on every third frame of one channel
                    s.c0[EDGE_CH % n], s.c1[EDGE_CH % n] = 1.0, -0.5
                    s.x[EDGE_CH % n, :, ::3] = 0.5
            elif pro == BNRELU or not s0["signed"]:
                s.x = s.x.clamp_min(0)                             # a post-ReLU tensor: about half of it exactly 0
        c.segs.append(s)
    # W on the 1/4 grid, half of it zero; bias, old, zmask, e1, e2 on the 1/8 grid, e0 in {1, -1, 1/2, 0}
    nW = wmax + 1 + 4096
    # ordinary: a bf16-valued weight like every other operand (what the packer's rounding does to an fp32 master weight is
    # master_weight's and pack_image's business: here it would only add a systematic term to the yardstick)
    c.W = (ri(-4, 4, nW) / 4 * (torch.rand(nW, generator=g) < 0.5).float()) if exact else rb(0.1 * rn(nW))
    nb = M + sd.chunks[-1]
    c.b = ri(-8, 8, nb) / 8 if exact else 0.3 * rn(nb)
    rows = nb if c.f32out else Mp
    c.old = ri(-16, 16, rows, c.out_L, NP) / 8 if exact else rb(rn(rows, c.out_L, NP))
    c.zmask = ri(-12, 12, Mp, c.out_L, NP) / 8 if exact else rb(rn(Mp, c.out_L, NP))
    if exact:
        c.e0, c.e1, c.e2 = pick([1.0, -1.0, 0.5, 0.0], M), ri(-8, 8, M) / 8, ri(-4, 4, M) / 8
    else:
        c.e0, c.e1, c.e2 = un(0.5, 1.5, M), 0.5 * rn(M), 0.3 * rn(M)
        c.e0[1::4] *= -1
    special(c.e0, c.e1, M)
    if regime == "zero":
        c.e0[EDGE_CH % M], c.e1[EDGE_CH % M] = 1.0, -0.5
        c.zmask[EDGE_CH % M, :, ::3] = 0.5
    return c


def master_weight(c):
    """an fp32 weight in the case's layout that bf16 does NOT hold: what the packers must round"""
    return 0.1 * torch.randn(c.W.shape, generator=_gen("bgemm master weight", c.case), dtype=torch.float32)


def refs(c, seq=True, dev="cpu"):
    """ordinary / zero: the float64 reference (no intermediate rounding) and the yardstick, element by element the worst of
    the fp32 emulation's three orders (without `seq` where seq = False: the wrap cases).  exact: the float64 restatement
    with the kernel's roundings is the reference; the rows are compared bit for bit, the statistics too where the
    magnitudes' sum proves every partial sum exact (c.exact_stats), else by the ordinary rule against the fp32 orders."""
    cd = to_device(c, dev)
    cpu = lambda o: {k: v.cpu() for k, v in o.items()}
    exact = c.regime == "exact"
    c.ref64 = cpu(R.bgemm(cd, torch.float64, bf16=exact))
    orders = [cpu(R.bgemm(cd, torch.float32, o)) for o in R.ORDERS if seq or o != "seq"]
    c.yard = R.yardstick(c.ref64, *orders)
    c.exact_stats = {}
    if exact and c.stats:
        mags = cpu(R.bgemm(cd, torch.float64, bf16=True, absval=True))
        for k in ("st0", "st1"):
            c.exact_stats[k] = float(mags[k].max()) / stat_unit(c, k) < 2 ** 24
    return c


# units of the `exact` regime's grids: activations 2^-4 (BN+ReLU: 1/16; plain: 1/8), dz 2^-8, W 2^-2, bias / old 2^-3
def row_unit(c):
    return 2.0 ** -10 if R.launch_pro(c) == BNBWD else 2.0 ** -6


def stat_unit(c, k):
    u = row_unit(c)
    return u if k == "st0" else (u * 2.0 ** -3 if c.mask else u * u)


@functools.lru_cache(maxsize=None)
def small(case):
    """cached: the small cases are shared between tests and must be left unchanged"""
    assert is_small(case)
    return refs(inputs(case))


# ---------------------------------------------------------------------------------------------- launches
NAN = float("nan")
OCT, GUARD_OCT = 16, 2            # every octet tensor a launch writes or reads beside: 16 octets + 2 guard octets
F32_GUARD = 16                    # guard rows of the fp32 output of the GRU projection
PART_GUARD, SENT = 64, 7.5


def _dev(t):
    return t.cuda().contiguous()


def _oct(t):
    """octet image of [C][L][NP]; C is padded to a multiple of 8 with zero channels"""
    Cn = t.shape[0]
    if Cn % 8:
        t = torch.cat([t, torch.zeros(8 - Cn % 8, *t.shape[1:])])
    return to_octets(t)


def _framed(t, fill=NAN):
    """[rows][out_L][NP] inside [(OCT + GUARD_OCT) 8][out_L + 2][NP] of `fill`: the launch is told out_L + 2 positions and
    out_pos_off + 1, so that one position before and one behind, and every octet up to the 16th and two more, are memory
    the test owns"""
    rows, Ln, NP = t.shape
    big = torch.full(((OCT + GUARD_OCT) * 8, Ln + 2, NP), fill)
    big[:rows, 1:Ln + 1] = t
    return big


def seg_list(c):
    return [(s.nchan, s.woff) for s in c.segs]


def image_elems(c):
    return ((c.M + 31) // 32) * sum(R.ksteps(s.nchan) for s in c.segs) * 64 * 8


def pack_single(Lb, c, W, w_m_off):
    """trunet_bf16_pack_weight -> the bf16 image on the device (and its k-step count)"""
    ns = len(c.segs)
    img = torch.full((image_elems(c),), NAN, device="cuda", dtype=torch.bfloat16)
    arr = lambda v: (ctypes.c_int32 * ns)(*v)
    nks = Lb.lib().trunet_bf16_pack_weight(Lb.ptr(W), Lb.ptr16(img), c.M, c.ldw_m, c.ldw_c, w_m_off, ns,
                                           arr([s.nchan for s in c.segs]), arr([s.woff for s in c.segs]), Lb.stream())
    assert nks == sum(R.ksteps(s.nchan) for s in c.segs), nks
    return img, nks


def pack_batch(Lb, items):
    """ONE trunet_bf16_pack_weights_batch launch for items = [(c, W on the device, w_m_off)]; returns the images, each with
    a sentinel tail of PART_GUARD elements behind it"""
    imgs = [torch.full((image_elems(c) + PART_GUARD,), NAN, device="cuda", dtype=torch.bfloat16) for c, _, _ in items]
    for img in imgs:
        img[-PART_GUARD:] = SENT
    arr = (Lb.BPackDesc * len(items))()
    for d, (c, W, off), img in zip(arr, items, imgs):
        d.W, d.out = Lb.ptr(W), Lb.ptr16(img)
        d.M, d.ldw_m, d.ldw_c, d.w_m_off, d.nseg = c.M, c.ldw_m, c.ldw_c, off, len(c.segs)
        k0 = 0
        for i, s in enumerate(c.segs):
            d.nchan[i], d.woff[i], d.ks0[i] = s.nchan, s.woff, k0
            k0 += R.ksteps(s.nchan)
        d.nks_total = k0
    desc = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    max_elems = max(image_elems(c) // 8 for c, _, _ in items)
    Lb.check(Lb.lib().trunet_bf16_pack_weights_batch(desc.data_ptr(), len(items), max_elems, Lb.stream()), "pack_weights_batch")
    torch.cuda.synchronize()
    return imgs


def gemm_args(c, chunk=0, prezero=False, shared=None):
    """the argument block of trunet_bf16_gemm for the launch at row offset `chunk`, every buffer prefilled: `out` with NaN,
    or with the `old` values under ACCUM, inside its guard frame; zmask inside a NaN frame; the statistics partials with
    NaN (zero with prezero, which the call is then told) and a sentinel tail.  `shared`: the buffers of an earlier chunk's
    launch (the fp32 output the GRU projection's three launches share).  Returns (args, buffers)."""
    from tinyrecurrentunet_amd import _lib as Lb
    lib = Lb.lib()
    assert lib.trunet_bf16_gemm_nparts() == NPARTS, "the case list is laid out for %d partial rows (512 workgroups x 4 " \
        "waves); the library reports %d" % (NPARTS, lib.trunet_bf16_gemm_nparts())
    keep = []
    a = Lb.BGemmArgs()
    a.NP, a.N, a.P, a.p_begin, a.M = c.NP, c.N, c.P, c.p_begin, c.M
    a.out_L, a.out_pos_off, a.nseg, a.m_out_off = c.out_L + 2, c.out_pos_off + 1, len(c.segs), chunk
    W = _dev(c.W)
    wimg, nks = pack_single(Lb, c, W, c.w_m_off + chunk)
    a.wfrag, a.nks_total = Lb.ptr16(wimg), nks
    k0 = 0
    for i, s in enumerate(c.segs):
        sg = Lb.BSeg()
        x16 = _dev(_oct(s.x))
        keep.append(x16)
        sg.src0 = Lb.ptr16(x16)
        sg.nchan, sg.L, sg.pos_mul, sg.pos_off, sg.pos_div, sg.woff, sg.mode = s.nchan, s.L, s.pos_mul, s.pos_off, \
            s.pos_div, s.woff, s.mode
        sg.kstep0 = k0
        k0 += R.ksteps(s.nchan)
        if s.mode == BNBWD:
            z16 = _dev(_oct(s.z))
            keep.append(z16)
            sg.src1 = Lb.ptr16(z16)
        if s.mode != NONE:
            co = [_dev(v) for v in ((s.c0, s.c1, s.c2) if s.mode == BNBWD else (s.c0, s.c1))]
            keep += co
            sg.c0, sg.c1 = Lb.ptr(co[0]), Lb.ptr(co[1])
            if s.mode == BNBWD:
                sg.c2 = Lb.ptr(co[2])
        a.seg[i] = sg
    if shared is not None:
        out, pre = shared.out, shared.pre
    elif c.f32out:
        rows, Ln, NP = c.old.shape
        pre = torch.full((rows + F32_GUARD, Ln + 2, NP), NAN)
        out = _dev(pre)
    else:
        pre = _framed(c.old) if c.accum else _framed(torch.full_like(c.old, NAN))
        pre = to_octets(pre)
        out = _dev(pre)
    a.out = Lb.ptr(out) if c.f32out else Lb.ptr16(out)
    epi = c.epi
    if c.bias:
        b = _dev(c.b)
        keep.append(b)
        a.bias = Lb.ptr(b)
    if c.mask:
        t = [_dev(to_octets(_framed(c.zmask))), _dev(c.e0), _dev(c.e1), _dev(c.e2)]
        keep += t
        a.zmask, a.e0, a.e1, a.e2 = Lb.ptr16(t[0]), Lb.ptr(t[1]), Lb.ptr(t[2]), Lb.ptr(t[3])
    part = None
    if c.stats:
        part = torch.full((NPARTS * c.M * 2 + PART_GUARD,), 0.0 if prezero else NAN, device="cuda")
        part[NPARTS * c.M * 2:] = SENT
        a.partials, a.M_stat = Lb.ptr(part), c.M
        epi |= PREZERO if prezero else 0
    a.epi = epi
    return a, NS(keep=keep, W=W, wimg=wimg, out=out, pre=pre, part=part)


def plan(a):
    """(nrt, pro, epi, full) of trunet_bf16_gemm_plan"""
    from tinyrecurrentunet_amd import _lib as Lb
    v = [ctypes.c_int(-9) for _ in range(4)]
    Lb.check(Lb.lib().trunet_bf16_gemm_plan(a, *[ctypes.byref(x) for x in v]), "bf16_gemm_plan")
    return tuple(x.value for x in v)


def gpu_gemm(c, prezero=False):
    """the launches of the case (one per chunk); returns CPU tensors: out (the whole buffer, guard frame included, bf16
    octets or fp32 rows), pre (what it held before), part [NPARTS][M][2] and its sentinel tail, wimg of every chunk, and
    the instance the plan reports"""
    from tinyrecurrentunet_amd import _lib as Lb
    lib = Lb.lib()
    b, inst, wimgs = None, set(), []
    for chunk in c.chunks:
        a, b = gemm_args(c, chunk, prezero, shared=b)
        inst.add(plan(a))
        Lb.check(lib.trunet_bf16_gemm(a, Lb.stream()), "bf16_gemm " + case_id(c.case))
        torch.cuda.synchronize()
        wimgs.append(b.wimg.cpu())
    assert len(inst) == 1, inst
    part = None if b.part is None else b.part.cpu()
    return NS(out=b.out.cpu(), pre=b.pre, wimg=wimgs, inst=inst.pop(),
              part=None if part is None else part[:NPARTS * c.M * 2].view(NPARTS, c.M, 2),
              tail=None if part is None else part[NPARTS * c.M * 2:])


# ---------------------------------------------------------------------------------------------- comparison and report
def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def results(c, o, tag):
    """the outputs of a launch under the restatement's names, after the checks that need the whole buffers: nothing outside
    the rows and positions the launch owns has changed by a bit, nothing it owns is left unwritten.  The rows come back as
    [8 ceil(M/8)][out_L][NP] (fp32 output: every row) with the restatement's `old` values at the positions outside the
    window, which the first check has just shown untouched."""
    win = R.window(c)
    fwin = slice(win.start + 1, win.stop + 1)
    own = torch.zeros(o.out.shape, dtype=torch.bool)
    if c.f32out:
        rows = c.old.shape[0]
        own[:rows, fwin] = True
        full = o.out
    else:
        own[:(c.M + 7) // 8, fwin] = True
        rows = (c.M + 7) // 8 * 8
        full = from_octets(o.out)
    changed = (bits(o.out) != bits(o.pre)) & ~own
    assert not bool(changed.any()), "%s: %d elements outside the launch's rows and positions changed (first at %s)" % \
        (tag, int(changed.sum()), changed.nonzero()[0].tolist())
    got = c.old.clone()
    got[:, win] = full[:rows, fwin]
    assert not bool(torch.isnan(got[:, win]).any()), "%s: out has unwritten (NaN) elements" % tag
    res = {"out": got}
    if c.stats:
        assert bool((o.tail == SENT).all()), "%s: a write behind the statistics partials" % tag
        assert not bool(torch.isnan(o.part).any()), "%s: statistics partials have unwritten (NaN) elements" % tag
        res["st0"], res["st1"] = o.part[:, :, 0].double().sum(0), o.part[:, :, 1].double().sum(0)
    return res


def rejected(c, got):
    """the comparison of one case: `ordinary` and `zero` through `close` against the float64 reference with the measured
    yardstick, every element of every output; `exact`: the rows bit for bit, the statistics bit for bit where the magnitudes
    prove the sums exact and through `close` elsewhere; in every regime the positions outside the window bit for bit.
    Returns ({name: (err, e_y, bound)}, [failures])."""
    res, fails = {}, []
    win = R.window(c)
    outside = torch.ones(c.out_L, dtype=torch.bool)
    outside[win] = False
    for k in R.outputs(c):
        g, r64, y = got[k], c.ref64[k], c.yard[k]
        if k == "out":
            if not torch.equal(g[:, outside].double(), c.old[:, outside].double()):
                fails.append("out changed at a position outside the launch's window")
            g, r64, y = g[:, win], r64[:, win], y[:, win]
        err = float((g.double() - r64).abs().max())
        if c.regime == "exact" and (k == "out" or c.exact_stats[k]):
            res[k] = (err, 0.0, 0.0)
            if not torch.equal(g.double(), r64):
                bad = g.double() != r64
                fails.append("%s: %d of %d elements differ from the exact value, max error %.3e" %
                             (k, int(bad.sum()), bad.numel(), err))
        else:
            e_y, bnd = R.bound(r64, y)[:2]
            res[k] = (err, e_y, bnd)
            try:
                R.close(g, r64, y, k)
            except AssertionError as e:
                fails.append(str(e))
    return res, fails


def compare(tag, c, got):
    """every figure is printed BEFORE the first assertion fires"""
    res, fails = rejected(c, got)
    report("%s: kernel error / e_y / bound  " % tag + "  ".join("%s %.2e/%.2e/%.2e" % ((n,) + res[n]) for n in res), PARITY)
    assert not fails, tag + ":\n" + "\n".join(fails)
    return res


def zeros_hold(c, got, tag):
    """exact zeros of the contract: rows >= M of the last octet, masked rows whose mask can never pass"""
    if c.f32out:
        return
    win = R.window(c)
    assert bool((got["out"][c.M:, win] == 0).all()), "%s: rows >= M of the last octet are not zero" % tag
    if c.mask:
        for ch in (ZERO_PRE_CH, ALWAYS_OFF_CH):
            assert bool((got["out"][ch % c.M, win] == 0).all()), "%s: row %d (mask never passes) is not 0" % (tag, ch % c.M)
            if c.stats:
                assert got["st0"][ch % c.M] == 0 and got["st1"][ch % c.M] == 0, "%s: statistics of a masked row" % tag


def check_case(c):
    """the launches of one case: plan, packed image, every output against the restatement, the exact zeros"""
    o = gpu_gemm(c)
    tag = "BGEMM " + case_id(c.case)
    assert o.inst == c.inst, "%s: reaches bgemm_kernel<%s>, meant for <%s>" % (tag, o.inst, c.inst)
    for chunk, wimg in zip(c.chunks, o.wimg):
        want = R.pack_image(c.W, c.M, c.ldw_m, c.ldw_c, c.w_m_off + chunk, seg_list(c))
        assert torch.equal(bits(wimg), want.reshape(-1)), "%s: packed image differs from pack_image" % tag
    got = results(c, o, tag)
    res = compare(tag, c, got)
    zeros_hold(c, got, tag)
    return res, o


def same_bits(o1, o2, what):
    assert torch.equal(bits(o1.out), bits(o2.out)), "%s: out differs" % what
    if o1.part is not None:
        assert torch.equal(bits(o1.part), bits(o2.part)), "%s: statistics partials differ" % what
