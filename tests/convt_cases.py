"""The fused ConvTranspose backward kernels (trunet_convt_bwd on the fp32 MFMA and on the three-term bf16 split,
trunet_bf16_convt_bwd on octet tensors) through the C ABI against tests/convt_ref.py: input regimes, shapes, launch helpers
and the case functions tests/test_convt_bwd_gpu.py calls.

A case is (K, S, regime, Lin, NP, N).  Inputs come from seeded CPU generators keyed by the case; frames >= N hold random
values like the live ones (the kernels must ignore them).  After drawing, src is nudged so that no |pre| = |s_scale src +
s_shift| of a channel with s_scale != 0 is below 1e-3: fp32 and fp64 then agree on every mask bit and no comparison has to
leave an element out."""
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

import convt_ref as R  # noqa: E402

C = R.C
KS = ((3, 1), (3, 2), (5, 2))
# Lin 1, 2: the run-start special cases; 3: the first with the step-2 prefetch and no q + 3 issue; 4 fills the 4-slot source
# ring; 5 wraps it; 9 wraps every dz ring (K + 2 S = 5, 7, 9 deep for Lout = 11, 17, 19) at least twice
LINS = (1, 2, 3, 4, 5, 9)
# fp32 / split kernels: 32-frame chunks, NP % 128, 256 workgroups.  (128, *): 252 workgroups own no chunk; (128, 97) ends
# inside a chunk; (384, 257): one live frame in chunk 8, chunks 9-11 wholly beyond N; (8320, 8290): 260 chunks, four
# workgroups own two and reuse their rings
F32_NPN, F32_BIG, F32_MID = ((128, 1), (128, 128), (128, 97), (384, 257)), (8320, 8290), (384, 257)
# bf16 kernel: 64-frame chunks, NP % 64; (16512, 16450): 258 chunks, the pipelined next() crosses a chunk boundary
B16_NPN, B16_BIG, B16_MID = ((64, 1), (64, 33), (192, 130)), (16512, 16450), (192, 130)
BIG_LINS = (1, 3)
MID_LIN = 5
REGIMES = ("ordinary", "signed", "trained", "dead_tile", "zero_cotangent")
ZERO_PRE_CH, ALWAYS_ON_CH, ALWAYS_OFF_CH = 10, 2, 6        # `signed`: the channels with s_scale = 0


def _cases(npn, big, mid):
    out = [(K, S, "ordinary", Lin, NP, N) for K, S in KS for Lin in LINS for NP, N in npn]
    out += [(K, S, "ordinary", Lin) + big for K, S in KS for Lin in BIG_LINS]
    out += [(K, S, r, MID_LIN) + mid for K, S in KS for r in REGIMES if r != "ordinary"]
    return out


F32_CASES = _cases(F32_NPN, F32_BIG, F32_MID)
B16_CASES = _cases(B16_NPN, B16_BIG, B16_MID)


def case_id(case):
    return "k%ds%d-%s-L%d-NP%d-N%d" % case


def is_big(case):
    return case[4] > 1024


def _gen(*key):
    return torch.Generator().manual_seed(int(hashlib.sha1(repr(key).encode()).hexdigest()[:8], 16))


def _nudge(c, bf16):
    """move the src values whose pre lies within 2e-3 of zero away from it (further at every pass: rounding src to bf16
    moves pre again); asserts min|pre| >= 1e-3 over the channels with s_scale != 0"""
    sc, sh = c.s_scale.double()[:, None, None], c.s_shift.double()[:, None, None]
    nz = (c.s_scale != 0)[:, None, None]
    safe = torch.where(nz, sc, torch.ones((), dtype=torch.float64))
    for it in range(1, 12):
        pre = sc * c.src.double() + sh
        bad = nz & (pre.abs() < 2e-3)
        if not bool(bad.any()):
            break
        step = torch.where(pre >= 0, 1.0, -1.0) * (4e-3 * it) / safe
        src = (c.src.double() + torch.where(bad, step, torch.zeros((), dtype=torch.float64))).float()
        c.src = R.bf16_round(src) if bf16 else src
    pre = sc * c.src.double() + sh
    c.min_pre = float(torch.where(nz, pre.abs(), torch.full((), 1e30, dtype=torch.float64)).min())
    c.active = float((pre > 0).double().mean())
    assert c.min_pre >= 1e-3, (c.case, c.min_pre)


def inputs(case, bf16=False):
    K, S, regime, Lin, NP, N = case
    g = _gen("convt", case, bf16)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    un = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g, dtype=torch.float32)
    Lo = R.lout(Lin, K, S)
    c = types.SimpleNamespace(case=case, K=K, S=S, regime=regime, Lin=Lin, Lout=Lo, NP=NP, N=N, bf16=bf16)
    c.dy, c.z, c.src = rn(C, Lo, NP), rn(C, Lo, NP), rn(C, Lin, NP)
    c.s_scale, c.s_shift, c.s_mean = un(0.5, 1.5, C), 0.5 * rn(C), 0.3 * rn(C)
    c.ca, c.cb, c.cc = un(0.5, 1.5, C), 0.2 * rn(C), 0.1 * rn(C)
    c.W = 0.1 * rn(C, C, K)
    if regime == "signed":
        c.s_scale[1::4] *= -1                               # every fourth channel: a negative BatchNorm weight
        for ch, sh in ((ALWAYS_ON_CH, 0.7), (ALWAYS_OFF_CH, -0.7), (ZERO_PRE_CH, 0.0)):
            c.s_scale[ch], c.s_shift[ch] = 0.0, sh          # pre = shift: always on, always off, exactly 0 (> against >=)
    elif regime == "trained":
        c.ca = un(3.0, 30.0, C)                             # a small running variance
        c.cb, c.cc = 1e-3 * rn(C), 1e-3 * rn(C)
        c.W = 0.5 * rn(C, C, K)
    elif regime == "dead_tile":
        c.s_shift[32:] = -100.0                             # the second 32-channel source tile is masked off as a whole
    elif regime == "zero_cotangent":
        c.dy, c.z, c.cc = torch.zeros_like(c.dy), torch.zeros_like(c.z), torch.zeros_like(c.cc)
    else:
        assert regime == "ordinary", regime
    if bf16:
        c.dy, c.z, c.src, c.W = (R.bf16_round(t) for t in (c.dy, c.z, c.src, c.W))
    _nudge(c, bf16)
    return c


def refs(c):
    """fp64 reference and the yardstick (fp32 kernels: the worse of the two fp32 orders; bf16: the emulation), once per case"""
    c.ref64 = R.convt_bwd(c, torch.float64)
    if c.bf16:
        c.yard = R.convt_bwd(c, torch.float32, bf16=True)
    else:
        c.blk = R.convt_bwd(c, torch.float32, "blocked")
        c.seq = R.convt_bwd(c, torch.float32, "seq")
        c.perm = R.convt_bwd(c, torch.float32, "permuted")
        c.yard = R.yardstick(c.ref64, c.blk, c.seq)
    return c


def build(case, bf16=False):
    return refs(inputs(case, bf16))


@functools.lru_cache(maxsize=None)
def small(case, bf16=False):
    """cached: the small cases are shared between tests and must be left unchanged"""
    assert not is_big(case)
    return build(case, bf16)


# ---------------------------------------------------------------------------------------------- launches
SENT = 7.5                 # sentinel around the weight slot and the bias row
W_OFF, W_TAIL = 96, 64     # the weight slot starts 96 floats into its image and ends 64 before the next
B_STRIDE, B_OFF = 96, 16


def owners(NP, chunk, grid):
    """bool [grid]: workgroup g owns at least one chunk (chunks [g n / grid, (g + 1) n / grid) of the n = NP / chunk)"""
    n = NP // chunk
    return torch.tensor([(g * n) // grid < ((g + 1) * n) // grid for g in range(grid)])


def _dev(t):
    return t.cuda().contiguous()


def _common_args(a, c, w_numel):
    a.NP, a.N, a.Lin, a.Lout, a.K, a.S, a.pad, a.Ci, a.Co = c.NP, c.N, c.Lin, c.Lout, c.K, c.S, c.S // 2, C, C
    a.w_numel, a.b_stride, a.b_off = w_numel, B_STRIDE, B_OFF


def _out_buffers(c, grid):
    w_numel = W_OFF + C * C * c.K + W_TAIL
    wimg = torch.full((grid, w_numel), SENT, device="cuda", dtype=torch.float32)
    wimg[:, W_OFF:W_OFF + C * C * c.K] = 0.0            # the contract: zero inside the slot
    bimg = torch.full((grid, B_STRIDE), SENT, device="cuda", dtype=torch.float32)
    return w_numel, wimg, bimg


def gpu_convt_bwd(c, x3, bias=True):
    """trunet_convt_bwd on the fp32 MFMA (x3 = False) or the three-term bf16 split (x3 = True).  dsrc and the statistics
    rows are prefilled with NaN; the weight slot sits in the middle of a larger image, the bias row in the middle of a longer
    row, sentinels around both.  Returns CPU tensors: dsrc [64][Lin][NP], parts [grid][64][2], wimg [grid][w_numel],
    bimg [grid][B_STRIDE] (None with bias = False)."""
    from tinyrecurrentunet_amd import _lib as Lb
    lib = Lb.lib()
    grid = lib.trunet_convt_bwd_nparts()
    t = {k: _dev(getattr(c, k)) for k in ("dy", "z", "ca", "cb", "cc", "src", "s_scale", "s_shift", "s_mean", "W")}
    dsrc = torch.full((C, c.Lin, c.NP), float("nan"), device="cuda", dtype=torch.float32)
    parts = torch.full((grid, C, 2), float("nan"), device="cuda", dtype=torch.float32)
    w_numel, wimg, bimg = _out_buffers(c, grid)
    a = Lb.ConvtBwdArgs()
    _common_args(a, c, w_numel)
    for k, v in t.items():
        setattr(a, k, Lb.ptr(v))
    a.dsrc, a.partials = Lb.ptr(dsrc), Lb.ptr(parts)
    a.w_partials = Lb.ptr(wimg) + 4 * W_OFF
    a.b_partials = Lb.ptr(bimg) if bias else None
    prev = lib.trunet_gemm_x3_enable(Lb.X3_BWD if x3 else 0)
    try:
        Lb.check(lib.trunet_convt_bwd(a, Lb.stream()), "convt_bwd")
        torch.cuda.synchronize()
    finally:
        lib.trunet_gemm_x3_enable(prev)
    return types.SimpleNamespace(dsrc=dsrc.cpu(), parts=parts.cpu(), wimg=wimg.cpu(), bimg=bimg.cpu() if bias else None,
                                 own=owners(c.NP, 32, grid), rows_per_group=1)


def to_octets(t):
    """[C][L][NP] fp32 (C % 8 == 0) -> bf16 [C/8][L][NP][8]: element (c, l, n) at (((c/8) L + l) NP + n) 8 + c % 8"""
    Cn, Ln, NP = t.shape
    return t.view(Cn // 8, 8, Ln, NP).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)


def from_octets(t):
    o, Ln, NP, _ = t.shape
    return t.permute(0, 3, 1, 2).reshape(o * 8, Ln, NP).float()


def gpu_from_frames_last(t):
    """trunet_bf16_from_frames_last on a CPU fp32 tensor [C][L][NP] -> CPU bf16 octet tensor"""
    from tinyrecurrentunet_amd import _lib as Lb
    Cn, Ln, NP = t.shape
    src = _dev(t)
    out = torch.zeros(Cn // 8, Ln, NP, 8, device="cuda", dtype=torch.bfloat16)
    Lb.check(Lb.lib().trunet_bf16_from_frames_last(Lb.ptr(src), Lb.ptr16(out), Cn, Ln, NP, Lb.stream()), "bf16_from_frames_last")
    torch.cuda.synchronize()
    return out.cpu()


def gpu_bf16_convt_bwd(c, prezero=False, bias=True):
    """trunet_bf16_convt_bwd on the octet images of the case's (bf16-valued) tensors; wfragT from trunet_bf16_pack_weight as
    the header prescribes.  prezero = False: the statistics rows are prefilled with NaN (the call zero-fills them);
    True: they are zero and the call is told so.  Returns what gpu_convt_bwd returns, dsrc unpacked to fp32."""
    import ctypes
    from tinyrecurrentunet_amd import _lib as Lb
    lib = Lb.lib()
    grid = lib.trunet_conv_wgrad_nparts()
    nparts = lib.trunet_bf16_convt_bwd_nparts()
    assert nparts == 2 * grid
    K = c.K
    dy, z, src = (_dev(to_octets(getattr(c, k))) for k in ("dy", "z", "src"))
    t = {k: _dev(getattr(c, k)) for k in ("ca", "cb", "cc", "s_scale", "s_shift", "s_mean")}
    W = _dev(c.W)
    wfrag = torch.zeros(2 * 4 * K * 64 * 8, device="cuda", dtype=torch.bfloat16)      # [2 row tiles][4 K k-steps][64 lanes][8]
    nks = lib.trunet_bf16_pack_weight(Lb.ptr(W), Lb.ptr16(wfrag), C, C * K, K, 0, K, (ctypes.c_int32 * K)(*([C] * K)),
                                      (ctypes.c_int32 * K)(*range(K)), Lb.stream())
    assert nks == 4 * K, nks
    dsrc = torch.full((C // 8, c.Lin, c.NP, 8), float("nan"), device="cuda", dtype=torch.bfloat16)
    parts = torch.full((nparts, C, 2), 0.0 if prezero else float("nan"), device="cuda", dtype=torch.float32)
    w_numel, wimg, bimg = _out_buffers(c, grid)
    a = Lb.BConvtArgs()
    _common_args(a, c, w_numel)
    a.prezero = 1 if prezero else 0
    a.dy, a.z, a.src, a.wfragT, a.dsrc = (Lb.ptr16(v) for v in (dy, z, src, wfrag, dsrc))
    for k, v in t.items():
        setattr(a, k, Lb.ptr(v))
    a.partials = Lb.ptr(parts)
    a.w_partials = Lb.ptr(wimg) + 4 * W_OFF
    a.b_partials = Lb.ptr(bimg) if bias else None
    Lb.check(lib.trunet_bf16_convt_bwd(a, Lb.stream()), "bf16_convt_bwd")
    torch.cuda.synchronize()
    return types.SimpleNamespace(dsrc=from_octets(dsrc.cpu()), parts=parts.cpu(), wimg=wimg.cpu(),
                                 bimg=bimg.cpu() if bias else None, own=owners(c.NP, 64, grid), rows_per_group=2)


INSTANCES = ("fp32", "split", "bf16")


def launch(c, inst, **kw):
    assert inst in INSTANCES and c.bf16 == (inst == "bf16"), (inst, c.bf16)
    return gpu_bf16_convt_bwd(c, **kw) if inst == "bf16" else gpu_convt_bwd(c, inst == "split", **kw)


# ---------------------------------------------------------------------------------------------- comparison and report
def report(line, name="parity_convt.txt"):
    """one line per case and instance: printed, and appended to the file `name` in the directory TRUNET_PARITY_DIR names
    (relative to the repository root), where that is set and the directory exists.  The one writer of the parity files of
    the per-kernel pins (tests/gru_cases.py and tests/bn_cases.py call it with their file names)."""
    print(line)
    out_dir = os.environ.get("TRUNET_PARITY_DIR")
    out_dir = os.path.join(ROOT, out_dir) if out_dir else None
    if out_dir and os.path.isdir(out_dir):
        with open(os.path.join(out_dir, name), "a") as f:
            f.write(line + "\n")


def compare(tag, items):
    """items: (name, got, ref64, yardstick).  Every figure is printed BEFORE the first assertion fires; returns
    {name: (err, e_y, bound)}."""
    res, fails = {}, []
    for name, got, r64, yard in items:
        e_y, bnd = R.bound(r64, yard)[:2]
        res[name] = (float((got.double() - r64).abs().max()), e_y, bnd)
        try:
            R.close(got, r64, yard, "%s %s" % (tag, name))
        except AssertionError as e:
            fails.append(str(e))
    report("%s: kernel error / e_y / bound  " % tag + "  ".join("%s %.2e/%.2e/%.2e" % ((n,) + res[n]) for n in res))
    assert not fails, "\n".join(fails)
    return res


def sums(c, o):
    """the five outputs of a launch: partial images, bias rows and statistics rows summed in float64 on the host"""
    K = c.K
    out = {"dW": o.wimg[:, W_OFF:W_OFF + C * C * K].double().sum(0).view(C, C, K), "dsrc": o.dsrc,
           "st0": o.parts[:, :, 0].double().sum(0), "st1": o.parts[:, :, 1].double().sum(0)}
    if o.bimg is not None:
        out["db"] = o.bimg[:, B_OFF:B_OFF + C].double().sum(0)
    return out


def exactness(c, o, tag):
    """what must hold bit for bit: nothing left unwritten, nothing written outside the slots, exact zeros where the contract
    has zeros"""
    K, N = c.K, c.N
    slot = o.wimg[:, W_OFF:W_OFF + C * C * K]
    assert not bool(torch.isnan(o.dsrc).any()), "%s: dsrc has unwritten (NaN) elements" % tag
    assert not bool(torch.isnan(o.parts).any()), "%s: statistics rows have unwritten (NaN) elements" % tag
    assert bool((o.dsrc[:, :, N:] == 0).all()), "%s: dsrc is not exactly 0 for frames >= N" % tag
    assert bool((o.wimg[:, :W_OFF] == SENT).all()) and bool((o.wimg[:, W_OFF + C * C * K:] == SENT).all()), \
        "%s: a write outside the weight slot" % tag
    if o.bimg is not None:
        assert bool((o.bimg[:, :B_OFF] == SENT).all()) and bool((o.bimg[:, B_OFF + C:] == SENT).all()), \
            "%s: a write outside the bias row" % tag
        assert bool((o.bimg[~o.own, B_OFF:B_OFF + C] == 0).all()), "%s: bias rows of idle workgroups" % tag
    assert bool((slot[~o.own] == 0).all()), "%s: weight images of workgroups that own no chunk are not exactly 0" % tag
    idle_rows = (~o.own).repeat_interleave(o.rows_per_group)
    assert bool((o.parts[idle_rows] == 0).all()), "%s: statistics rows of workgroups that own no chunk are not exactly 0" % tag
    img = slot.view(-1, C, C, K)
    if c.regime == "dead_tile":
        assert bool((o.dsrc[32:] == 0).all()) and bool((o.parts[:, 32:] == 0).all()) and bool((img[:, 32:] == 0).all()), \
            "%s: the masked-off source tile is not exactly 0" % tag
    if c.regime == "signed":
        for ch in (ZERO_PRE_CH, ALWAYS_OFF_CH):
            assert bool((o.dsrc[ch] == 0).all()) and bool((o.parts[:, ch] == 0).all()) and bool((img[:, ch] == 0).all()), \
                "%s: channel %d (pre <= 0 everywhere) is not exactly 0" % (tag, ch)
        assert bool((o.dsrc[ALWAYS_ON_CH, :, :N] != 0).any())
    if c.regime == "zero_cotangent":
        assert bool((o.dsrc == 0).all()) and bool((o.parts == 0).all()) and bool((slot == 0).all()), \
            "%s: zero cotangent, non-zero output" % tag
        assert o.bimg is None or bool((o.bimg[:, B_OFF:B_OFF + C] == 0).all())


def same_bits(o1, o2, what, skip=()):
    for k in ("dsrc", "parts", "wimg", "bimg"):
        if k in skip:
            continue
        assert torch.equal(getattr(o1, k), getattr(o2, k)), "%s: %s differs" % (what, k)


def tag_of(c, inst):
    return "CONVT-BWD %s %s" % (inst, case_id(c.case))


def check_case(c, inst):
    """one launch of the case on the instance: the five outputs through `close`, then the exactness assertions"""
    o = launch(c, inst)
    got = sums(c, o)
    tag = tag_of(c, inst)
    res = compare(tag, [(k, got[k], c.ref64[k], c.yard[k]) for k in R.OUTPUTS])
    exactness(c, o, tag)
    return res, o
