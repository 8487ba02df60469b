"""GPU: the bf16 storage / bf16 MFMA family (BASELINE.json configs[2], a build extension -- SURVEY 8d: the reference has no
reduced-precision path, so the gate is against fp32 with a stated looser tolerance).

Unit level: every trunet_bf16_* kernel against a torch restatement of the SAME arithmetic (operands rounded to bf16
where the kernel rounds them, fp32/fp64 accumulation), so the bound is the final bf16 rounding of the stored value
(2^-8 relative) resp. fp32 accumulation error for the fp32 outputs.  Network level: forward within 1e-2 relative of the
fp32 HIP path, loss within 1 %, gradients close in relative L2."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _rb(x):
    return x.bfloat16().float()


def to_oct(x):
    """fp32 [C][L][NP] -> bf16 octets [C/8][L][NP][8] (channels zero-padded to a multiple of 8)"""
    C, Ln, NP = x.shape
    C8 = (C + 7) // 8 * 8
    if C8 != C:
        x = torch.cat([x, torch.zeros(C8 - C, Ln, NP, device=x.device)], 0)
    return x.view(C8 // 8, 8, Ln, NP).permute(0, 2, 3, 1).contiguous().bfloat16()


def from_oct(t, C):
    o, Ln, NP, _ = t.shape
    return t.float().permute(0, 3, 1, 2).reshape(o * 8, Ln, NP)[:C].contiguous()


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=g, device=DEV)


def _seg_q(p, mul, off, div, Ls):
    qn = p * mul + off
    if qn < 0 or qn % div or qn // div >= Ls:
        return None
    return qn // div


def _run_gemm(N, P, M, segs, W, ldw_m, ldw_c, w_m_off=0, bias=None, relu=False, mask=None, accum=None, stats=False,
              p_begin=0, out_L=None, out_pos_off=0):
    """segs: list of dict(x=fp32 [C][L][NP] (bf16-representable), x1=..., mode, c0, c1, c2, pos_mul, pos_off, pos_div, woff)
    returns (out fp32 [M][out_L][NP] as stored, stats or None) from the kernel and from the torch restatement."""
    from tinyrecurrentunet_amd import _lib as L
    from tinyrecurrentunet_amd._lib import (EPI_ACCUM, EPI_BIAS, EPI_MASK, EPI_RELU, EPI_STATS, PRO_BNBWD, PRO_BNRELU,
                                            BGemmArgs, check, ptr, ptr16)
    from tinyrecurrentunet_amd.engine_bf16 import bseg
    import ctypes as C
    lib, st = L.lib(), L.stream()
    NP = segs[0]["x"].shape[2]
    out_L = out_L or P
    keep = []
    bs = []
    for s in segs:
        t0 = to_oct(s["x"])
        t1 = to_oct(s["x1"]) if s.get("x1") is not None else None
        keep += [t0, t1]
        bs.append(bseg(t0, s["x"].shape[0], s["x"].shape[1], s.get("pos_mul", 1), s.get("pos_off", 0), s.get("pos_div", 1),
                       s.get("woff", 0), s.get("mode", 0), src1=t1, c0=s.get("c0"), c1=s.get("c1"), c2=s.get("c2")))
    nseg = len(bs)
    nks = sum(((b.nchan + 7) // 8 + 1) // 2 for b in bs)
    wfrag = torch.empty(((M + 31) // 32) * nks * 64 * 8, device=DEV, dtype=torch.bfloat16)
    rc = lib.trunet_bf16_pack_weight(ptr(W), ptr16(wfrag), M, ldw_m, ldw_c, w_m_off, nseg,
                                     (C.c_int32 * nseg)(*[b.nchan for b in bs]), (C.c_int32 * nseg)(*[b.woff for b in bs]), st)
    assert rc == nks
    a = BGemmArgs()
    a.NP, a.N, a.P, a.p_begin, a.M, a.out_L, a.out_pos_off, a.nseg, a.nks_total = NP, N, P, p_begin, M, out_L, out_pos_off, nseg, nks
    k0 = 0
    for i, b in enumerate(bs):
        b.kstep0 = k0
        k0 += ((b.nchan + 7) // 8 + 1) // 2
        a.seg[i] = b
    out0 = accum if accum is not None else torch.zeros(M, out_L, NP, device=DEV)
    out = to_oct(out0)
    a.out, a.wfrag = ptr16(out), ptr16(wfrag)
    epi = 0
    if bias is not None:
        epi |= EPI_BIAS
        a.bias = ptr(bias)
    if relu:
        epi |= EPI_RELU
    if accum is not None:
        epi |= EPI_ACCUM
    zm = None
    if mask is not None:
        epi |= EPI_MASK
        zm = to_oct(mask["z"])
        a.zmask, a.e0, a.e1, a.e2 = ptr16(zm), ptr(mask["e0"]), ptr(mask["e1"]), ptr(mask["e2"])
    part = None
    if stats:
        epi |= EPI_STATS
        nparts = lib.trunet_bf16_gemm_nparts()
        part = torch.empty(nparts * M * 2, device=DEV)
        a.partials, a.M_stat = ptr(part), M
    a.epi = epi
    check(lib.trunet_bf16_gemm(a, st), "bf16_gemm")
    torch.cuda.synchronize()
    got = from_oct(out, M)
    got_stats = part.view(-1, M, 2).double().sum(0) if stats else None

    # ---- torch restatement
    ref = torch.zeros(M, out_L, NP, device=DEV, dtype=torch.float64)
    if accum is not None:
        ref += _rb(accum).double()
    touched = torch.zeros(out_L, dtype=torch.bool)
    for p in range(p_begin, p_begin + P):
        acc = torch.zeros(M, NP, device=DEV, dtype=torch.float64)
        for s in segs:
            x = s["x"]
            Cs, Ls = x.shape[0], x.shape[1]
            q = _seg_q(p, s.get("pos_mul", 1), s.get("pos_off", 0), s.get("pos_div", 1), Ls)
            if q is None:
                continue
            v = x[:, q]
            mode = s.get("mode", 0)
            if mode == PRO_BNRELU:
                v = torch.relu(s["c0"][:, None] * v + s["c1"][:, None])
            elif mode == PRO_BNBWD:
                v = s["c0"][:, None] * v + s["c1"][:, None] * s["x1"][:, q] + s["c2"][:, None]
            v = _rb(v).double()
            idx = (torch.arange(M, device=DEV)[:, None] + w_m_off) * ldw_m + torch.arange(Cs, device=DEV)[None, :] * ldw_c \
                + s.get("woff", 0)
            A = _rb(W.reshape(-1)[idx]).double()
            acc += A @ v
        o = acc
        if bias is not None:
            o = o + bias[:, None].double()
        o = o + ref[:, p + out_pos_off]
        if mask is not None:
            zz = mask["z"][:, p + out_pos_off]
            o = torch.where((mask["e0"][:, None] * zz + mask["e1"][:, None]) > 0, o, torch.zeros_like(o))
        if relu:
            o = torch.relu(o)
        ref[:, p + out_pos_off] = o
        touched[p + out_pos_off] = True
    ref_stats = None
    if stats:
        r = _rb(ref.float()).double()[:, touched][:, :, :N]
        if mask is not None:
            zz = mask["z"][:, touched][:, :, :N].double() - mask["e2"][:, None, None].double()
            ref_stats = torch.stack([r.sum((1, 2)), (r * zz).sum((1, 2))], 1)
        else:
            ref_stats = torch.stack([r.sum((1, 2)), (r * r).sum((1, 2))], 1)
    return got, ref.float(), touched, got_stats, ref_stats


def _close_bf16(got, ref, what):
    err = (got - ref).abs()
    tol = 2.0 ** -7 * ref.abs() + 1e-2 * ref.abs().mean() + 1e-6
    bad = (err > tol).float().mean().item()
    assert bad < 1e-4, "%s: %.2e of the elements off by more than one bf16 ulp (max err %.3e)" % (what, bad, err.max().item())


def _stats_close(got, ref, n, what):
    # the kernel's statistics are those of ITS stored values; one ulp flips of individual elements move a sum by
    # ~2^-8 * |x| / sqrt(count)
    scale = ref.abs().max().item() + 1e-6
    assert (got - ref).abs().max().item() < 2e-3 * scale + 1e-3, "%s: %s vs %s" % (what, got[:4], ref[:4])


def test_bf16_gemm_pointwise_two_sources_stats():
    """decoder pointwise conv over [x1 (shifted by F.pad) | skip] with BN+ReLU prologues, bias, statistics"""
    rnd = _gen(1)
    N, NP, P, M = 300, 512, 9, 64
    x1, x2 = _rb(rnd(64, 8, NP)), _rb(rnd(128, 9, NP))
    W = rnd(M, 192, 1) * 0.1
    bias = rnd(M) * 0.1
    segs = [dict(x=x1, mode=1, c0=rnd(64) * 0.3 + 1, c1=rnd(64) * 0.2, pos_off=-1, woff=0),
            dict(x=x2, mode=1, c0=rnd(128) * 0.3 + 1, c1=rnd(128) * 0.2, woff=64)]
    got, ref, touched, gs, rs = _run_gemm(N, P, M, segs, W, 192, 1, bias=bias, stats=True)
    _close_bf16(got, ref, "pw two sources")
    _stats_close(gs, rs, N * P, "pw two sources statistics")


def test_bf16_gemm_transposed_conv_taps_m128_and_m8():
    rnd = _gen(2)
    N, NP = 200, 256
    # ConvTranspose1d(64 -> 64, k=5, s=2, pad=1): Lin 7 -> Lout 15
    x = _rb(rnd(64, 7, NP))
    W = rnd(64, 64, 5) * 0.1          # [ci][co][k]
    c0, c1 = rnd(64) * 0.3 + 1, rnd(64) * 0.2
    segs = [dict(x=x, mode=1, c0=c0, c1=c1, pos_off=1 - kk, pos_div=2, woff=kk) for kk in range(5)]
    got, ref, _, gs, rs = _run_gemm(N, 15, 64, segs, W, 5, 64 * 5, bias=rnd(64) * 0.1, stats=True)
    _close_bf16(got, ref, "convT k5 s2")
    _stats_close(gs, rs, N * 15, "convT statistics")
    # 128 rows (two waves share a tile), plain source, ReLU epilogue
    x = _rb(rnd(64, 6, NP))
    W = rnd(128, 64, 1) * 0.1
    got, ref, _, _, _ = _run_gemm(N, 6, 128, [dict(x=x)], W, 64, 1, bias=rnd(128) * 0.1, relu=True)
    _close_bf16(got, ref, "M=128 relu")
    # 8 rows (decoder.5): 128 -> 8 and the 8 -> 8 transposed conv
    x = _rb(rnd(128, 6, NP))
    W = rnd(8, 128, 1) * 0.1
    got, ref, _, _, _ = _run_gemm(N, 6, 8, [dict(x=x, mode=1, c0=rnd(128) * 0.3 + 1, c1=rnd(128) * 0.2)], W, 128, 1,
                                  bias=rnd(8) * 0.1)
    _close_bf16(got, ref, "M=8")
    # first conv: 4 channels (padded octet), k=5 s=2 pad=1: 257 -> 128 positions (take 21 -> 10)
    x = _rb(rnd(4, 21, NP))
    W = rnd(64, 4, 5) * 0.3
    segs = [dict(x=x, pos_mul=2, pos_off=kk - 1, woff=kk) for kk in range(5)]
    got, ref, _, _, _ = _run_gemm(N, 10, 64, segs, W, 20, 5, bias=rnd(64) * 0.1, relu=True)
    _close_bf16(got, ref, "first conv")


def test_bf16_gemm_data_gradient_bnbwd_mask_accum_stats():
    """data gradient of a pointwise conv: BatchNorm-backward prologue on (dy, z), transposed weight, output window
    shifted by the F.pad offset, ReLU mask of the source, accumulation onto the skip gradient, BN-backward statistics"""
    rnd = _gen(3)
    N, NP, P, M = 300, 512, 9, 64
    dy, z = _rb(rnd(M, P, NP)), _rb(rnd(M, P, NP))
    W = rnd(M, 192, 1) * 0.1
    seg = dict(x=dy, x1=z, mode=2, c0=rnd(M) * 0.5 + 1, c1=rnd(M) * 0.1, c2=rnd(M) * 0.01)
    zsrc = _rb(rnd(128, 9, NP))
    mask = dict(z=zsrc, e0=rnd(128) * 0.3 + 1, e1=rnd(128) * 0.2, e2=rnd(128) * 0.1)
    prev = _rb(rnd(128, 9, NP))
    got, ref, touched, gs, rs = _run_gemm(N, P, 128, [seg], W, 1, 192, w_m_off=64, mask=mask, accum=prev, stats=True)
    _close_bf16(got, ref, "dgrad skip")
    _stats_close(gs, rs, N * P, "dgrad statistics")
    # the x1 source: 8 positions, shifted by one (left = 1): p in [1, 9)
    zsrc = _rb(rnd(64, 8, NP))
    mask = dict(z=zsrc, e0=rnd(64) * 0.3 + 1, e1=rnd(64) * 0.2, e2=rnd(64) * 0.1)
    got, ref, touched, gs, rs = _run_gemm(N, 8, 64, [seg], W, 1, 192, w_m_off=0, mask=mask, stats=True, p_begin=1, out_L=8,
                                          out_pos_off=-1)
    assert touched.all()
    _close_bf16(got, ref, "dgrad x1")
    _stats_close(gs, rs, N * 8, "dgrad x1 statistics")


def _run_wgrad(N, P, M, dz, z, co, segs, Wshape, ldw_m, ldw_c):
    from tinyrecurrentunet_amd import _lib as L
    from tinyrecurrentunet_amd._lib import PRO_BNBWD, PRO_BNRELU, PRO_NONE, BWgradArgs, check, ptr, ptr16
    from tinyrecurrentunet_amd.engine_bf16 import bseg
    lib, st = L.lib(), L.stream()
    NP = dz.shape[2]
    numel = 1
    for d in Wshape:
        numel *= d
    npw = lib.trunet_conv_wgrad_nparts()
    a = BWgradArgs()
    a.NP, a.N, a.P, a.p_begin, a.M, a.a_L, a.a_pos_off = NP, N, P, 0, M, P, 0
    a.ldw_m, a.ldw_c, a.w_m_off, a.nseg, a.w_numel = ldw_m, ldw_c, 0, len(segs), numel
    keep = []
    for i, s in enumerate(segs):
        t0 = to_oct(s["x"])
        keep.append(t0)
        a.seg[i] = bseg(t0, s["x"].shape[0], s["x"].shape[1], s.get("pos_mul", 1), s.get("pos_off", 0), s.get("pos_div", 1),
                        s.get("woff", 0), s.get("mode", 0), c0=s.get("c0"), c1=s.get("c1"))
    d16 = to_oct(dz)
    a.a0 = ptr16(d16)
    if z is not None:
        z16 = to_oct(z)
        a.a_mode, a.a1, a.ac0, a.ac1, a.ac2 = PRO_BNBWD, ptr16(z16), ptr(co[0]), ptr(co[1]), ptr(co[2])
    else:
        a.a_mode = PRO_NONE
    wp = torch.full((npw * numel,), float("nan"), device=DEV)      # every image and bias row must be written by its workgroup
    bp = torch.full((npw * M,), float("nan"), device=DEV)
    a.w_partials, a.b_partials, a.b_stride, a.b_off = ptr(wp), ptr(bp), M, 0
    check(lib.trunet_bf16_wgrad(a, st), "bf16_wgrad")
    torch.cuda.synchronize()
    gw = wp.view(npw, numel).double().sum(0)
    gb = bp.view(npw, M).double().sum(0)
    # ---- restatement
    dzz = dz if z is None else co[0][:, None, None] * dz + co[1][:, None, None] * z + co[2][:, None, None]
    dzz = dzz.clone()
    dzz[:, :, N:] = 0
    rb_ = dzz.double().sum((1, 2))
    dzr = _rb(dzz).double()
    rw = torch.zeros(numel, device=DEV, dtype=torch.float64)
    for s in segs:
        x = s["x"]
        Cs, Ls = x.shape[0], x.shape[1]
        v = x
        if s.get("mode", 0) == PRO_BNRELU:
            v = torch.relu(s["c0"][:, None, None] * x + s["c1"][:, None, None])
        v = _rb(v).double()
        g = torch.zeros(M, Cs, device=DEV, dtype=torch.float64)
        for p in range(P):
            q = _seg_q(p, s.get("pos_mul", 1), s.get("pos_off", 0), s.get("pos_div", 1), Ls)
            if q is not None:
                g += dzr[:, p] @ v[:, q].T
        idx = torch.arange(M, device=DEV)[:, None] * ldw_m + torch.arange(Cs, device=DEV)[None, :] * ldw_c + s.get("woff", 0)
        rw[idx.reshape(-1)] += g.reshape(-1)
    return gw, rw, gb, rb_


def _l2(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def test_bf16_wgrad_shapes_of_the_backward():
    rnd = _gen(4)
    N, NP = 300, 512
    co = lambda M: (rnd(M) * 0.5 + 1, rnd(M) * 0.1, rnd(M) * 0.01)
    # encoder pointwise 128 <- 128 behind a BatchNorm
    M, P = 128, 6
    dz, z = _rb(rnd(M, P, NP)), _rb(rnd(M, P, NP))
    x = _rb(rnd(128, P, NP))
    gw, rw, gb, rb_ = _run_wgrad(N, P, M, dz, z, co(M), [dict(x=x, mode=1, c0=rnd(128) * 0.3 + 1, c1=rnd(128) * 0.2)],
                                 (M, 128, 1), 128, 1)
    assert _l2(gw, rw) < 3e-4 and _l2(gb, rb_) < 2e-5, (_l2(gw, rw), _l2(gb, rb_))
    # decoder pointwise 64 <- [64 shifted | 128]
    M, P = 64, 9
    dz, z = _rb(rnd(M, P, NP)), _rb(rnd(M, P, NP))
    segs = [dict(x=_rb(rnd(64, 8, NP)), mode=1, c0=rnd(64) * 0.3 + 1, c1=rnd(64) * 0.2, pos_off=-1, woff=0),
            dict(x=_rb(rnd(128, 9, NP)), mode=1, c0=rnd(128) * 0.3 + 1, c1=rnd(128) * 0.2, woff=64)]
    gw, rw, gb, rb_ = _run_wgrad(N, P, M, dz, z, co(M), segs, (M, 192, 1), 192, 1)
    assert _l2(gw, rw) < 3e-4 and _l2(gb, rb_) < 2e-5, (_l2(gw, rw), _l2(gb, rb_))
    # transposed conv 64 -> 64, k=5 s=2 pad=1: weight [ci][co][k], dz over 15 output positions, source 7 positions
    M, P = 64, 15
    dz, z = _rb(rnd(M, P, NP)), _rb(rnd(M, P, NP))
    x = _rb(rnd(64, 7, NP))
    c0, c1 = rnd(64) * 0.3 + 1, rnd(64) * 0.2
    segs = [dict(x=x, mode=1, c0=c0, c1=c1, pos_off=1 - kk, pos_div=2, woff=kk) for kk in range(5)]
    gw, rw, gb, rb_ = _run_wgrad(N, P, M, dz, z, co(M), segs, (64, 64, 5), 5, 64 * 5)
    assert _l2(gw, rw) < 3e-4 and _l2(gb, rb_) < 2e-5, (_l2(gw, rw), _l2(gb, rb_))
    # thin layers: 8 <- [64 | 64] (decoder.5 pointwise), 8 -> 8 transposed conv without BatchNorm, first conv 64 <- 4 x 5 taps
    M, P = 8, 6
    dz, z = _rb(rnd(M, P, NP)), _rb(rnd(M, P, NP))
    segs = [dict(x=_rb(rnd(64, 6, NP)), mode=1, c0=rnd(64) * 0.3 + 1, c1=rnd(64) * 0.2, woff=0),
            dict(x=_rb(torch.relu(rnd(64, 6, NP))), woff=64)]      # a plain source next to a BN+ReLU one is post-ReLU
    gw, rw, gb, rb_ = _run_wgrad(N, P, M, dz, z, co(M), segs, (M, 128, 1), 128, 1)
    assert _l2(gw, rw) < 3e-4 and _l2(gb, rb_) < 2e-5, (_l2(gw, rw), _l2(gb, rb_))
    M, P = 8, 15
    dz = _rb(rnd(M, P, NP))
    x = _rb(rnd(8, 7, NP))
    segs = [dict(x=x, mode=1, c0=rnd(8) * 0.3 + 1, c1=rnd(8) * 0.2, pos_off=1 - kk, pos_div=2, woff=kk) for kk in range(5)]
    for s in segs[1:]:
        s["c0"], s["c1"] = segs[0]["c0"], segs[0]["c1"]
    gw, rw, gb, rb_ = _run_wgrad(N, P, M, dz, None, None, segs, (8, 8, 5), 5, 8 * 5)
    assert _l2(gw, rw) < 3e-4 and _l2(gb, rb_) < 2e-5, (_l2(gw, rw), _l2(gb, rb_))
    M, P = 64, 10
    dz = _rb(rnd(M, P, NP))
    x = _rb(rnd(4, 21, NP))
    segs = [dict(x=x, pos_mul=2, pos_off=kk - 1, woff=kk) for kk in range(5)]
    gw, rw, gb, rb_ = _run_wgrad(N, P, M, dz, None, None, segs, (64, 4, 5), 20, 5)
    assert _l2(gw, rw) < 3e-4 and _l2(gb, rb_) < 2e-5, (_l2(gw, rw), _l2(gb, rb_))


@pytest.mark.parametrize("K,S,Lin", [(3, 1, 12), (5, 2, 21), (3, 2, 16), (5, 2, 64), (3, 1, 33)])
def test_bf16_depthwise_forward_backward(K, S, Lin):
    from tinyrecurrentunet_amd import _lib as L
    from tinyrecurrentunet_amd._lib import check, ptr, ptr16
    import torch.nn.functional as F
    lib, st = L.lib(), L.stream()
    rnd = _gen(10 * K + S)
    N, NP, Cn = 300, 512, 16
    Lout = (Lin + 2 * (K // 2) - K) // S + 1
    zin = _rb(rnd(Cn, Lin, NP))
    sc, sh, mean = rnd(Cn) * 0.3 + 1, rnd(Cn) * 0.2, rnd(Cn) * 0.1
    wgt, b = rnd(Cn, 1, K) * 0.5, rnd(Cn) * 0.1
    zin16 = to_oct(zin)
    zout16 = torch.empty((Cn // 8, Lout, NP, 8), device=DEV, dtype=torch.bfloat16)
    nparts = lib.trunet_bf16_dw_nparts(NP, Lout)
    part = torch.zeros(nparts * Cn * 2, device=DEV)
    check(lib.trunet_bf16_dwconv_fwd(ptr16(zin16), ptr(sc), ptr(sh), ptr(wgt), ptr(b), ptr16(zout16), ptr(part), Cn, K, S, Lin,
                                     Lout, NP, N, st), "fwd")
    torch.cuda.synchronize()
    act = torch.relu(sc[:, None, None] * zin + sh[:, None, None])                       # [C][L][NP]
    ref = F.conv1d(act.permute(2, 0, 1).double(), wgt.double(), b.double(), stride=S, padding=K // 2, groups=Cn)
    ref = ref.permute(1, 2, 0).float()                                                  # [C][Lout][NP]
    got = from_oct(zout16, Cn)
    _close_bf16(got, ref, "dw forward")
    r = _rb(ref)[:, :, :N].double()
    st_ref = torch.stack([r.sum((1, 2)), (r * r).sum((1, 2))], 1)
    _stats_close(part.view(nparts, Cn, 2).double().sum(0), st_ref, N * Lout, "dw statistics")

    # ---- backward
    dy, z = _rb(rnd(Cn, Lout, NP)), _rb(rnd(Cn, Lout, NP))
    ca, cb, cc = rnd(Cn) * 0.5 + 1, rnd(Cn) * 0.1, rnd(Cn) * 0.01
    dy16, z16 = to_oct(dy), to_oct(z)
    din16 = torch.empty((Cn // 8, Lin, NP, 8), device=DEV, dtype=torch.bfloat16)
    nparts = lib.trunet_bf16_dw_nparts(NP, Lin)
    part = torch.zeros(nparts * Cn * 2, device=DEV)
    wp = torch.zeros(nparts * Cn * K, device=DEV)
    bp = torch.zeros(nparts * Cn, device=DEV)
    check(lib.trunet_bf16_dwconv_bwd(ptr16(dy16), ptr16(z16), ptr(ca), ptr(cb), ptr(cc), ptr16(zin16), ptr(sc), ptr(sh),
                                     ptr(mean), ptr(wgt), ptr16(din16), ptr(part), ptr(wp), ptr(bp), Cn, K, S, Lin, Lout, NP,
                                     N, st), "bwd")
    torch.cuda.synchronize()
    dz = (ca[:, None, None] * dy + cb[:, None, None] * z + cc[:, None, None]).double()
    dz[:, :, N:] = 0
    dzn = dz.permute(2, 0, 1)                                                           # [NP][C][Lout]
    actn = act.permute(2, 0, 1).double().requires_grad_(True)
    wd = wgt.double().requires_grad_(True)
    bd = b.double().requires_grad_(True)
    y = F.conv1d(actn, wd, bd, stride=S, padding=K // 2, groups=Cn)
    y.backward(dzn)
    gin = (actn.grad.permute(1, 2, 0) * (act > 0)).float()
    got = from_oct(din16, Cn)
    _close_bf16(got, gin, "dw data gradient")
    assert _l2(wp.view(nparts, -1).double().sum(0), wd.grad.reshape(-1)) < 3e-4
    assert _l2(bp.view(nparts, -1).double().sum(0), bd.grad) < 2e-5
    r = _rb(gin)[:, :, :N].double()
    st_ref = torch.stack([r.sum((1, 2)), (r * (zin[:, :, :N].double() - mean[:, None, None].double())).sum((1, 2))], 1)
    _stats_close(part.view(nparts, Cn, 2).double().sum(0), st_ref, N * Lin, "dw backward statistics")


def test_bf16_layout_round_trip():
    from tinyrecurrentunet_amd import _lib as L
    from tinyrecurrentunet_amd._lib import check, ptr, ptr16
    lib, st = L.lib(), L.stream()
    rnd = _gen(7)
    for Cn in (4, 8, 128):
        x = rnd(Cn, 5, 256)
        y16 = torch.empty(((Cn + 7) // 8, 5, 256, 8), device=DEV, dtype=torch.bfloat16)
        check(lib.trunet_bf16_from_frames_last(ptr(x), ptr16(y16), Cn, 5, 256, st), "from")
        assert torch.equal(y16, to_oct(x))
        back = torch.empty_like(x)
        check(lib.trunet_bf16_to_frames_last(ptr16(y16), ptr(back), Cn, 5, 256, st), "to")
        assert torch.equal(back, _rb(x))
    # the module API layout (N, C, L) <-> one octet, directly
    for Cn, N, Ln, NP in ((4, 200, 257, 256), (8, 300, 70, 512), (3, 1, 33, 256)):
        xn = rnd(N, Cn, Ln)
        y16 = torch.full((1, Ln, NP, 8), float("nan"), device=DEV, dtype=torch.bfloat16)
        check(lib.trunet_bf16_from_ncl(ptr(xn), ptr16(y16), N, Cn, Ln, NP, st), "from_ncl")
        ref = torch.zeros(Cn, Ln, NP, device=DEV)
        ref[:, :, :N] = xn.permute(1, 2, 0)
        assert torch.equal(y16, to_oct(ref))
        back = torch.full((N, Cn, Ln), float("nan"), device=DEV)
        check(lib.trunet_bf16_to_ncl(ptr16(y16), ptr(back), N, Cn, Ln, NP, st), "to_ncl")
        assert torch.equal(back, _rb(xn))


def test_bf16_gru_kernels_match_the_fp32_recurrence_on_the_same_operands():
    """trunet_bf16_gru_fwd / _bwd (round 3: the bidirectional recurrence with octet tensors on both sides) against the fp32
    kernels trunet_gru_fwd / _bwd (pinned by block_gru_bi.npz and the fp64 oracle, and on their own against the fp64 recurrence by
    tests/test_gru_gpu.py) on the SAME bf16-representable operands:
    the arithmetic inside is the same fp32 arithmetic, so every stored value may differ by the final bf16 rounding only
    (one ulp = 2^-8 relative where the two fp32 values straddle a rounding boundary).  Ragged workgroup count (NP = 384)."""
    from tinyrecurrentunet_amd import _lib as L
    from tinyrecurrentunet_amd._lib import check, ptr, ptr16
    lib, st = L.lib(), L.stream()
    rnd = _gen(41)
    Hh, Lg, NP = 64, 16, 384
    whh = [rnd(3 * Hh, Hh) * 0.15 for _ in range(2)]
    bhh = [rnd(3 * Hh) * 0.1 for _ in range(2)]
    gi = _rb(rnd(6 * Hh, Lg, NP))
    gi16 = to_oct(gi)
    # forward
    hout = torch.empty(2 * Hh, Lg, NP, device=DEV)
    gates = torch.empty(2, 4, Hh, Lg, NP, device=DEV)
    check(lib.trunet_gru_fwd(ptr(gi), ptr(whh[0]), ptr(bhh[0]), ptr(whh[1]), ptr(bhh[1]), ptr(hout), ptr(gates), Hh, Lg, NP, st), "gru_fwd")
    hout16 = torch.full((2 * Hh // 8, Lg, NP, 8), float("nan"), device=DEV, dtype=torch.bfloat16)
    gates16 = torch.full((8 * Hh // 8, Lg, NP, 8), float("nan"), device=DEV, dtype=torch.bfloat16)
    check(lib.trunet_bf16_gru_fwd(ptr16(gi16), ptr(whh[0]), ptr(bhh[0]), ptr(whh[1]), ptr(bhh[1]), ptr16(hout16), ptr16(gates16),
                                  Hh, Lg, NP, st), "bf16_gru_fwd")
    torch.cuda.synchronize()

    def close(a16, ref, C, what):
        a = from_oct(a16, C)
        assert torch.isfinite(a).all(), what
        err = (a - ref).abs()
        tol = ref.abs() * 2.0 ** -7 + 1e-6          # one bf16 ulp (+ the fp32 difference in front of the rounding)
        assert bool((err <= tol).all()), (what, float((err - tol).max()))
        assert float(err.norm() / ref.norm()) < 3e-3, (what, float(err.norm() / ref.norm()))

    close(hout16, hout, 2 * Hh, "hout")
    close(gates16, gates.reshape(8 * Hh, Lg, NP), 8 * Hh, "gates")
    # eval: no gates
    hout16e = torch.full_like(hout16, float("nan"))
    check(lib.trunet_bf16_gru_fwd(ptr16(gi16), ptr(whh[0]), ptr(bhh[0]), ptr(whh[1]), ptr(bhh[1]), ptr16(hout16e), None,
                                  Hh, Lg, NP, st), "bf16_gru_fwd")
    assert torch.equal(hout16e, hout16)
    # backward on the state the bf16 forward saved (as fp32 for the fp32 kernel)
    dhout = _rb(rnd(2 * Hh, Lg, NP))
    h32 = from_oct(hout16, 2 * Hh)
    g32 = from_oct(gates16, 8 * Hh).reshape(2, 4, Hh, Lg, NP).contiguous()
    dgi = torch.empty(6 * Hh, Lg, NP, device=DEV)
    dghn = torch.empty(2 * Hh, Lg, NP, device=DEV)
    check(lib.trunet_gru_bwd(ptr(dhout), ptr(h32), ptr(g32), ptr(whh[0]), ptr(whh[1]), ptr(dgi), ptr(dghn), Hh, Lg, NP, NP, st), "gru_bwd")
    dgi16 = torch.full((6 * Hh // 8, Lg, NP, 8), float("nan"), device=DEV, dtype=torch.bfloat16)
    dghn16 = torch.full((2 * Hh // 8, Lg, NP, 8), float("nan"), device=DEV, dtype=torch.bfloat16)
    check(lib.trunet_bf16_gru_bwd(ptr16(to_oct(dhout)), ptr16(hout16), ptr16(gates16), ptr(whh[0]), ptr(whh[1]), ptr16(dgi16),
                                  ptr16(dghn16), Hh, Lg, NP, st), "bf16_gru_bwd")
    torch.cuda.synchronize()
    close(dgi16, dgi, 6 * Hh, "dgi")
    close(dghn16, dghn, 2 * Hh, "dghn")


def test_bf16_gru_backward_vs_the_exact_fp32_recurrence():
    """bgru_bwd_kernel takes h_{t-1} from the bf16-rounded recurrence output and r, z, n, gh from bf16 gate planes,
    while the forward carried h in fp32 -- so what it computes is not exactly the gradient of the forward that ran.  How far
    off is it?  The fp32 kernels (trunet_gru_fwd / _bwd, exact fp32 hout and gates, pinned by block_gru_bi.npz and the fp64
    oracle, and on their own by tests/test_gru_gpu.py) on the same bf16-representable gi and dhout are the yardstick: relative L2 of dgi, dghn and of the recurrent
    weight gradients dW_hh = sum_t dg_t h_{t-1}^T formed from either result (what trunet_bf16_wgrad computes from them).
    Measured (round 4, 1x MI355X, N = 384 x 16 steps): dgi 3.4e-3, dghn 3.8e-3, dW_hh 3.7e-3; bounds at ~3x.  TRUNET_BF16_GRU_IO=0 keeps
    the exact fp32 recurrence between conversion launches."""
    from tinyrecurrentunet_amd import _lib as L
    from tinyrecurrentunet_amd._lib import check, ptr, ptr16
    lib, st = L.lib(), L.stream()
    rnd = _gen(43)
    Hh, Lg, NP = 64, 16, 384
    whh = [rnd(3 * Hh, Hh) * 0.15 for _ in range(2)]
    bhh = [rnd(3 * Hh) * 0.1 for _ in range(2)]
    gi = _rb(rnd(6 * Hh, Lg, NP))
    dhout = _rb(rnd(2 * Hh, Lg, NP))
    # exact fp32 forward + backward
    hout = torch.empty(2 * Hh, Lg, NP, device=DEV)
    gates = torch.empty(2, 4, Hh, Lg, NP, device=DEV)
    check(lib.trunet_gru_fwd(ptr(gi), ptr(whh[0]), ptr(bhh[0]), ptr(whh[1]), ptr(bhh[1]), ptr(hout), ptr(gates), Hh, Lg, NP, st), "gru_fwd")
    dgi = torch.empty(6 * Hh, Lg, NP, device=DEV)
    dghn = torch.empty(2 * Hh, Lg, NP, device=DEV)
    check(lib.trunet_gru_bwd(ptr(dhout), ptr(hout), ptr(gates), ptr(whh[0]), ptr(whh[1]), ptr(dgi), ptr(dghn), Hh, Lg, NP, NP, st), "gru_bwd")
    # the bf16-I/O kernels
    gi16, dh16 = to_oct(gi), to_oct(dhout)
    hout16 = torch.empty((2 * Hh // 8, Lg, NP, 8), device=DEV, dtype=torch.bfloat16)
    gates16 = torch.empty((8 * Hh // 8, Lg, NP, 8), device=DEV, dtype=torch.bfloat16)
    check(lib.trunet_bf16_gru_fwd(ptr16(gi16), ptr(whh[0]), ptr(bhh[0]), ptr(whh[1]), ptr(bhh[1]), ptr16(hout16), ptr16(gates16),
                                  Hh, Lg, NP, st), "bf16_gru_fwd")
    dgi16 = torch.empty((6 * Hh // 8, Lg, NP, 8), device=DEV, dtype=torch.bfloat16)
    dghn16 = torch.empty((2 * Hh // 8, Lg, NP, 8), device=DEV, dtype=torch.bfloat16)
    check(lib.trunet_bf16_gru_bwd(ptr16(dh16), ptr16(hout16), ptr16(gates16), ptr(whh[0]), ptr(whh[1]), ptr16(dgi16), ptr16(dghn16),
                                  Hh, Lg, NP, st), "bf16_gru_bwd")
    torch.cuda.synchronize()
    a_dgi, a_dghn, a_h = from_oct(dgi16, 6 * Hh), from_oct(dghn16, 2 * Hh), from_oct(hout16, 2 * Hh)

    def dwhh(dgi_, dghn_, h_):
        """recurrent weight gradient per direction: rows (r, z) from dgi, rows n from dghn, against h of the previous step"""
        out = []
        for d in range(2):
            hd = h_[d * Hh:(d + 1) * Hh].double()
            prev = torch.zeros_like(hd)
            if d == 0:
                prev[:, 1:] = hd[:, :-1]
            else:
                prev[:, :-1] = hd[:, 1:]
            dg = torch.cat([dgi_[d * 3 * Hh:d * 3 * Hh + 2 * Hh], dghn_[d * Hh:(d + 1) * Hh]], 0).double()
            out.append(torch.einsum("mln,kln->mk", dg, prev))
        return torch.stack(out)

    e_dgi, e_dghn = _l2(a_dgi, dgi), _l2(a_dghn, dghn)
    e_w = _l2(dwhh(a_dgi, a_dghn, a_h).float(), dwhh(dgi, dghn, hout).float())
    msg = "bf16-I/O GRU backward vs the exact fp32 recurrence: dgi %.2e  dghn %.2e  dW_hh %.2e (relative L2)" % (e_dgi, e_dghn, e_w)
    print(msg)
    import os
    out_dir = os.path.join(os.path.dirname(os.path.dirname(__file__)), "gpurun_out")
    if os.path.isdir(out_dir):
        open(os.path.join(out_dir, "parity_bf16_gru.txt"), "a").write(msg + "\n")
    # one bf16 rounding of every stored value is 2^-9 = 2e-3 relative RMS; 16 recurrent steps compound it
    assert e_dgi < 1.2e-2 and e_dghn < 1.2e-2 and e_w < 1.2e-2, msg


def _pair(cin, seed=0):
    from tinyrecurrentunet_amd.network import TRUNet
    torch.manual_seed(seed)
    a = TRUNet(input_size=cin).cuda().train()
    b = TRUNet(input_size=cin, precision="bf16").cuda().train()
    b.load_state_dict(a.state_dict())
    return a, b


@pytest.mark.parametrize("N", [777, 32064])
def test_bf16_backward_matches_fp32_backward_on_the_same_forward_state(N):
    """(N = 32,064: the benchmarked size of BASELINE.json configs[2], round 4 -- every persistent workgroup, partial image and
    statistics row of the bf16 backward kernels in use.)  The whole-network gradient reacts chaotically to bf16-sized perturbations of the FORWARD (ReLU masks flip: see
    the next test), so the wiring of the bf16 backward is pinned where it is well conditioned: given the forward state,
    backward is a LINEAR map of the output cotangent.  The bf16 forward's saved tensors are converted to fp32 exactly and
    handed to the fp32 engine's backward (fused fp32 kernels, already pinned against the reference); the bf16 backward on
    the same state may differ only by the bf16 rounding of the activation gradients it stores and multiplies (2^-9 each,
    ~40 stages deep at the first layer: measured 1e-3 at decoder.5 growing to 3e-2 at encoder.0; gate 5e-2)."""
    from tinyrecurrentunet_amd import _lib as L
    from tinyrecurrentunet_amd._lib import check, ptr, ptr16
    from tinyrecurrentunet_amd.engine import Act, TRUNetEngine
    from tinyrecurrentunet_amd.engine_bf16 import Act16, TRUNetEngineBF16
    from tinyrecurrentunet_amd.network import TRUNet
    torch.manual_seed(3)
    net = TRUNet(input_size=4).cuda().train()
    g = torch.Generator(device=DEV)
    g.manual_seed(9)
    x = torch.randn(N, 4, 257, generator=g, device=DEV)
    gout = torch.randn(N, 8, 257, generator=g, device=DEV) / N
    e16 = TRUNetEngineBF16(net)
    _, ctx = e16.forward(x, True, record=True)
    acts, N_, NP, w, gen = ctx
    g16 = {p: t.clone() for p, t in e16.backward(ctx, gout).items()}
    # the same forward state as fp32 tensors
    lib, st = L.lib(), L.stream()
    acts32 = {}
    for k, a in acts.items():
        if isinstance(a, Act16):
            t = torch.empty((a.C, a.L, NP), device=DEV)
            check(lib.trunet_bf16_to_frames_last(ptr16(a.t), ptr(t), a.C, a.L, NP, st), "to_frames_last")
            acts32[k] = Act(t, a.C, a.L, a.bn)
        else:
            acts32[k] = a
    if "fgru.f32" in acts:                       # TRUNET_BF16_GRU_PROJ=0: the block ran in fp32 on fp32 copies
        acts32["fgru"], acts32["enc5"] = acts["fgru.f32"], acts["enc5.f32"]
    if "gates16" in w.t:                         # the recurrence saved its gates as octets: the fp32 backward reads them as fp32
        g16t = w.t["gates16"]
        gates32 = w.get("gates", (2, 4, g16t.shape[0], g16t.shape[1], NP))
        check(lib.trunet_bf16_to_frames_last(ptr16(g16t), ptr(gates32), g16t.shape[0] * 8, g16t.shape[1], NP, st), "to_frames_last")
    e32 = TRUNetEngine(net)
    # the saved depthwise outputs are the bf16 engine's ROUNDED tensors: the fp32 backward must read them, not recompute them
    # from the (also rounded) inputs, or its dz would not belong to the statistics of the forward state
    import tinyrecurrentunet_amd.engine as E32
    rz, E32.DW_RZ = E32.DW_RZ, False
    try:
        g32 = e32.backward((acts32, N, NP, w, gen), gout)
    finally:
        E32.DW_RZ = rz
    worst, errs = 0.0, []
    for n, p in net.named_parameters():
        if n.startswith("TGRU."):
            continue
        a, b = g16[p], g32[p]
        if b.norm().item() < 1e-5 * b.numel() ** 0.5:      # conv biases in front of a BatchNorm: analytically zero
            assert a.norm().item() < 2e-2, (n, a.norm().item())
            continue
        # a BatchNorm weight followed by ReLU -> conv -> BatchNorm has an analytically vanishing gradient while its bias
        # is 0 (the next BatchNorm removes the scale): measure it against the scale of its sibling bias gradient
        scale = b.norm().item()
        if n.endswith(".1.weight"):
            scale = max(scale, g32[dict(net.named_parameters())[n[:-6] + "bias"]].norm().item())
        e = (a - b).norm().item() / (scale + 1e-30)
        print("%-50s %.3e   |g| %.3e" % (n, e, b.norm().item()))
        worst = max(worst, e)
        errs.append((e, n))
    import numpy as np
    med = float(np.median([e for e, _ in errs]))
    msg = "N = %d: bf16 backward vs the fp32 backward of the same forward state: relative L2 median %.3e, worst %.3e (%s)" % (
        N, med, worst, max(errs)[1])
    print(msg)
    import os
    out_dir = os.path.join(os.path.dirname(os.path.dirname(__file__)), "gpurun_out")
    if os.path.isdir(out_dir):
        open(os.path.join(out_dir, "parity_bf16_same_state.txt"), "a").write(msg + "\n")
    # N = 777: 1e-3 at decoder.5 growing to 3e-2 at encoder.0 (gate 5e-2 per tensor).  N = 32,064 (random cotangent / N: the
    # per-channel sums cancel more strongly the longer they are): measured median 2.2e-2, most tensors 1.1e-2 .. 4.4e-2, the
    # two BatchNorm parameters of encoder.5 6.3e-2 / 1.06e-1 and the GRU input bias -- a plain sum of the bf16 dgi over all
    # 513,024 (frame, position) pairs -- 2.6e-1: gates median 3e-2, 90th percentile 8e-2, worst 4e-1
    es = sorted(e for e, _ in errs)
    if N < 10000:
        assert worst < 5e-2, msg
    else:
        assert es[int(0.9 * (len(es) - 1))] < 8e-2 and worst < 4e-1, msg
    assert med < 3e-2, msg


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_bf16_weight_images_follow_in_place_weight_updates(precision):
    """The bf16 engine packs every weight into MFMA A-fragment images, all of them in ONE launch at the start of a forward (from the
    second step on).  An image must be built from the weights of THIS step -- also for the GRU input projection, whose source is a
    workspace tensor (both directions' W_ih concatenated): until round 3 that concatenation happened AFTER the batched pack, so
    from the second step on the projection (forward GEMM and the W^T image of its data gradient) ran on the weights of the
    step before.  Here: forward / backward once (the plan fills), overwrite weights in place as an optimizer does, run again,
    and compare output and gradients bit for bit with a fresh network that holds the same weights."""
    from tinyrecurrentunet_amd.network import TRUNet
    from tinyrecurrentunet_amd import _lib
    torch.manual_seed(21)
    a = TRUNet(input_size=4, precision=precision).cuda().train()      # (fp32: no packed images; the same contract)
    g = torch.Generator(device=DEV)
    g.manual_seed(8)
    N = 140
    x = torch.randn(N, 4, 257, generator=g, device=DEV)
    gout = torch.randn(N, 8, 257, generator=g, device=DEV) / N
    for _ in range(2):          # two steps: the second one already runs on the batched pack
        for p in a.parameters():
            p.grad = None
        a(x).backward(gout)
    with torch.no_grad():
        for n, p in a.named_parameters():
            if p.dim() > 1 and not n.startswith("TGRU"):
                p.mul_(0.5).add_(0.01 * torch.randn(p.shape, generator=g, device=DEV))      # in place: same storage
    _lib.bump_mutation_epoch()
    for p in a.parameters():
        p.grad = None
    ya = a(x)
    ya.backward(gout)
    b = TRUNet(input_size=4, precision=precision).cuda().train()
    b.load_state_dict(a.state_dict())
    # BatchNorm running statistics were loaded AFTER a's third forward updated them; they do not enter a training forward
    yb = b(x)
    yb.backward(gout)
    assert torch.equal(ya, yb)
    pb = dict(b.named_parameters())
    for n, p in a.named_parameters():
        if n.startswith("TGRU"):
            continue
        assert torch.equal(p.grad, pb[n].grad), n


@pytest.mark.parametrize("cin,N", [(4, 501), (3, 130)])
def test_bf16_network_forward_and_gradients_vs_fp32(cin, N):
    """SURVEY 8d gate for configs[2].  The survey proposed "forward <= 1e-2 relative"; measured, the randomly initialised
    network turns ONE bf16 rounding per layer (the weights alone, fp32 everywhere else) into 1.7e-2 at the output and
    27-41 % in the deep layers' gradients -- every perturbation flips ReLU masks downstream -- so three roundings per layer
    (stored activation, MFMA operand, weight) give 3.0-3.3e-2.  The gate is therefore relative to that yardstick: forward
    <= 5e-2 and <= 2.5x the weights-only deviation; every gradient tensor within 2x the weights-only deviation (+ 0.1) and
    positively aligned with the fp32 gradient (cosine >= 0.6); the loss itself within 1 % (next test)."""
    from tinyrecurrentunet_amd.network import TRUNet
    f32, b16 = _pair(cin)
    f32w = TRUNet(input_size=cin).cuda().train()
    f32w.load_state_dict(f32.state_dict())
    with torch.no_grad():
        for p in f32w.parameters():
            if p.dim() > 1:
                p.copy_(_rb(p))
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    x = torch.randn(N, cin, 257, generator=g, device=DEV)
    gout = torch.randn(N, 8, 257, generator=g, device=DEV) / N
    ys = []
    for net in (f32, f32w, b16):
        y = net(x)
        y.backward(gout)
        ys.append(y.detach())
    rel, relw = _l2(ys[2], ys[0]), _l2(ys[1], ys[0])
    print("forward: bf16 vs fp32 %.3e, fp32 with bf16-rounded weights vs fp32 %.3e" % (rel, relw))
    assert rel < 5e-2 and rel < 2.5 * relw, (rel, relw)
    bad = []
    for (n, p), (_, pw), (_, q) in zip(f32.named_parameters(), f32w.named_parameters(), b16.named_parameters()):
        if n.startswith("TGRU."):
            continue
        assert q.grad is not None, n
        if p.grad.norm().item() < 1e-6 * p.grad.numel() ** 0.5:        # conv biases in front of a BatchNorm: ~0
            assert q.grad.norm().item() < 2e-2, n
            continue
        e, ew = _l2(q.grad, p.grad), _l2(pw.grad, p.grad)
        cos = (q.grad * p.grad).sum().item() / (q.grad.norm().item() * p.grad.norm().item() + 1e-30)
        sib = dict(f32.named_parameters())[n[:-6] + "bias"].grad.norm().item() if n.endswith(".1.weight") else 0.0
        if p.grad.norm().item() < 0.05 * sib:
            # analytically vanishing while the BatchNorm bias is 0 (its scale is removed by the next BatchNorm): only small
            if not (q.grad - p.grad).norm().item() < 0.5 * sib:
                bad.append((n, e, ew, cos, sib))
            continue
        if not (e < 2 * ew + 0.1 and cos > 0.6):
            bad.append((n, e, ew, cos))
    assert not bad, bad
    # BatchNorm running statistics updated like fp32
    for (n, p), (_, q) in zip(f32.named_buffers(), b16.named_buffers()):
        if n.startswith("TGRU.") or "num_batches" in n:
            continue
        assert _l2(q.float(), p.float()) < 3e-2, n


def test_bf16_loss_within_one_percent_and_repeatable():
    from tinyrecurrentunet_amd.stft_loss import MultiResolutionSTFTLoss
    from tinyrecurrentunet_amd.util import loss_fn
    f32, b16 = _pair(4)
    mr = MultiResolutionSTFTLoss(fft_sizes=[512, 1024, 2048], hop_sizes=[50, 120, 240], win_lengths=[240, 600, 1200],
                                 window="hann_window", sc_lambda=0.5, mag_lambda=0.5, band="full").cuda()
    g = torch.Generator(device=DEV)
    g.manual_seed(11)
    clean = 0.1 * torch.randn(4, 1, 16000, generator=g, device=DEV)
    noisy = clean + 0.05 * torch.randn(4, 1, 16000, generator=g, device=DEV)
    l32, d32 = loss_fn(f32, (clean, noisy), 1, 1.0, 1.0, mr)
    l16, d16 = loss_fn(b16, (clean, noisy), 1, 1.0, 1.0, mr)
    assert abs(l16.item() - l32.item()) < 1e-2 * abs(l32.item()), (l16.item(), l32.item())
    for k in d32:
        assert abs(d16[k].item() - d32[k].item()) < 2e-2 * abs(d32[k].item()) + 1e-5, (k, d16[k].item(), d32[k].item())
    l16.backward()
    g1 = [p.grad.clone() for n, p in b16.named_parameters() if p.grad is not None]
    b16.zero_grad(set_to_none=True)
    for m in b16.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.reset_running_stats()
    l16b, _ = loss_fn(b16, (clean, noisy), 1, 1.0, 1.0, mr)
    l16b.backward()
    g2 = [p.grad for n, p in b16.named_parameters() if p.grad is not None]
    assert l16b.item() == l16.item()
    assert all(torch.equal(a, b) for a, b in zip(g1, g2)), "bf16 step is not bitwise repeatable"


def test_bf16_eval_forward_through_the_layer_kernels():
    """eval() with the single-launch folded path switched off: the bf16 layer kernels with running statistics (bias-only
    epilogue: the run-time-flag instances) against the fp32 layer kernels; odd frame counts incl. one frame"""
    f32, b16 = _pair(4, seed=2)
    g = torch.Generator(device=DEV)
    g.manual_seed(21)
    x = torch.randn(700, 4, 257, generator=g, device=DEV)
    f32(x), b16(x)                                   # one training forward each: non-trivial running statistics
    f32.eval(), b16.eval()
    f32.fold_eval = b16.fold_eval = False
    with torch.no_grad():
        for N in (1, 63, 257, 700):
            y32, y16 = f32(x[:N]), b16(x[:N])
            assert y16.shape == (N, 8, 257) and torch.isfinite(y16).all()
            assert _l2(y16, y32) < 5e-2, (N, _l2(y16, y32))


def test_bf16_full_size_step_configs2_per_gpu_shape():
    """BASELINE.json configs[2] per-GPU shape (64 x 4 s pairs = 32,064 frames, C_in = 4), the size the bench runs at.
    (1) loss and its terms within 1 % of the fp32 HIP step (which test_configs_gpu pins against the fp32 oracle at this size,
    forward AND all 100 gradient tensors); the bf16 step bitwise repeatable.
    (2) round 4: EVERY one of the 100 bf16 gradient tensors against the fp32 HIP gradient of the same
    step -- relative L2 and cosine per tensor -- next to the same two figures for the yardstick "fp32 engine with
    bf16-rounded weights" (ONE rounding per layer instead of three).  At N <= 501 these deviations are 30-100 % (every
    perturbation flips ReLU masks and the sums are short); at 32,064 frames the sums are long and the figures below were
    measured (gpurun_out/parity_fullsize_bf16.txt, copied into DESIGN section 8); the bounds are ~3x the measured values.
    (3) the forward (training mode, batch statistics) at this size against fp32: relative L2 and the yardstick's."""
    import os
    import numpy as np
    from tinyrecurrentunet_amd import dataset as ds
    from tinyrecurrentunet_amd.network import TRUNet
    from tinyrecurrentunet_amd.stft_loss import MultiResolutionSTFTLoss
    from tinyrecurrentunet_amd.util import loss_fn
    f32, b16 = _pair(4, seed=4)
    mr = MultiResolutionSTFTLoss(fft_sizes=[512, 1024, 2048], hop_sizes=[50, 120, 240], win_lengths=[240, 600, 1200],
                                 window="hann_window", sc_lambda=0.5, mag_lambda=0.5, band="full").cuda()
    g = torch.Generator(device=DEV)
    g.manual_seed(31)
    clean = 0.1 * torch.randn(64, 1, 64000, generator=g, device=DEV)
    noisy = clean + 0.05 * torch.randn(64, 1, 64000, generator=g, device=DEV)
    feats = ds.stft_features(noisy[:, 0].contiguous(), pcen=True)

    def step(net):
        net.zero_grad(set_to_none=True)
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.reset_running_stats()
        loss, info = loss_fn(net, (clean, noisy), 1, 1.0, 1.0, mr)
        loss.backward()
        with torch.no_grad():
            y = net(feats)                       # training-mode forward (batch statistics) without recording
        return loss.item(), {k: v.item() for k, v in info.items()}, \
            {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}, y

    l32, d32, g32, y32 = step(f32)
    del f32
    torch.cuda.empty_cache()
    # yardstick: the fp32 engine on weights rounded to bf16 (matrices only, like the bf16 engine's packed images)
    f32w = TRUNet(input_size=4).cuda().train()
    f32w.load_state_dict(b16.state_dict())
    with torch.no_grad():
        for p in f32w.parameters():
            if p.dim() > 1:
                p.copy_(_rb(p))
    lw, dw, gw, yw = step(f32w)
    del f32w
    torch.cuda.empty_cache()
    runs = [step(b16) for _ in range(2)]
    l16, d16, g16, y16 = runs[0]
    assert abs(l16 - l32) < 1e-2 * abs(l32), (l16, l32)
    for k in d32:
        assert abs(d16[k] - d32[k]) < 2e-2 * abs(d32[k]) + 1e-5, (k, d16[k], d32[k])
    assert sum(t.numel() for t in g16.values()) == 298592 and len(g16) == 100
    assert all(torch.isfinite(t).all() for t in g16.values())
    assert runs[1][0] == l16 and all(torch.equal(g16[n], runs[1][2][n]) for n in g16)
    assert torch.equal(y16, runs[1][3])
    # ---- (3) forward at full size
    fwd16, fwdw = _l2(y16, y32), _l2(yw, y32)
    # ---- (2) all 100 gradient tensors
    real, zero, vanish = [], [], []
    for n, r in g32.items():
        def dev(t):
            cos = (t * r).sum().item() / (t.norm().item() * r.norm().item() + 1e-30)
            return (t - r).norm().item() / (r.norm().item() + 1e-30), cos
        sib = g32[n[:-6] + "bias"].norm().item() if n.endswith(".1.weight") else 0.0
        if r.norm().item() < 1e-6 * r.numel() ** 0.5:
            zero.append((n, g16[n].norm().item(), gw[n].norm().item()))      # conv bias in front of a BatchNorm: analytically 0
        elif r.norm().item() < 0.05 * sib:
            # BatchNorm weight whose gradient vanishes while its bias is 0 (the next BatchNorm removes the scale)
            vanish.append((n, (g16[n] - r).norm().item() / sib, (gw[n] - r).norm().item() / sib))
        else:
            real.append((n,) + dev(g16[n]) + dev(gw[n]))
    e16 = np.array([x[1] for x in real]); c16 = np.array([x[2] for x in real])
    ew = np.array([x[3] for x in real]); cw = np.array([x[4] for x in real])
    z16, v16 = max([x[1] for x in zero] + [0.0]), max([x[1] for x in vanish] + [0.0])
    lines = ["bf16 full-size step (N = 32,064) vs the fp32 HIP step; yardstick = fp32 engine with bf16-rounded weights",
             "forward (training mode) relative L2: bf16 %.3e   yardstick %.3e" % (fwd16, fwdw),
             "loss: fp32 %.6f  bf16 %.6f  yardstick %.6f" % (l32, l16, lw),
             "gradients, %d tensors with a non-vanishing fp32 gradient (of %d):" % (len(real), len(g32)),
             "  bf16      relative L2 median %.3e max %.3e   cosine median %.5f min %.5f" % (
                 np.median(e16), e16.max(), np.median(c16), c16.min()),
             "  yardstick relative L2 median %.3e max %.3e   cosine median %.5f min %.5f" % (
                 np.median(ew), ew.max(), np.median(cw), cw.min()),
             "  %d analytically zero gradients (conv biases in front of a BatchNorm): largest |g| bf16 %.3e yardstick %.3e" % (
                 len(zero), z16, max([x[2] for x in zero] + [0.0])),
             "  %d vanishing BatchNorm-weight gradients, deviation / |sibling bias gradient|: bf16 %.3e yardstick %.3e" % (
                 len(vanish), v16, max([x[2] for x in vanish] + [0.0]))]
    worst = sorted(real, key=lambda x: -x[1])[:8]
    lines += ["  %-46s bf16 %.3e (cos %.4f)   yardstick %.3e (cos %.4f)" % x for x in worst]
    msg = "\n".join(lines)
    print(msg)
    out_dir = os.path.join(os.path.dirname(os.path.dirname(__file__)), "gpurun_out")
    if os.path.isdir(out_dir):
        open(os.path.join(out_dir, "parity_fullsize_bf16.txt"), "a").write(msg + "\n\n")
    # Measured (round 4): the gradient of this randomly initialised network moves by 30-40 % in relative L2 under ANY
    # bf16-sized perturbation of the forward, also at 32,064 frames (yardstick: median 0.41, max 1.2, cosine min 0.52; bf16
    # path: median 0.30, max 0.82, cosine median 0.958, min 0.70) -- the loss runs through atan2 / sigmoid of the net output
    # and every perturbation flips ReLU masks.  So: no worse than the one-rounding-per-layer yardstick, absolute bounds at
    # ~1.5x the measured values, and the tight pin of the bf16 backward at this size is the linear-map test above
    # (test_bf16_backward_matches_fp32_backward_on_the_same_forward_state[32064], 5e-2 per tensor).
    assert fwd16 < 5e-2 and fwd16 < 2.5 * fwdw, msg
    assert np.median(e16) < 0.45 and np.median(e16) < 1.2 * np.median(ew), msg
    assert e16.max() < 1.2 and e16.max() < 1.2 * ew.max(), msg
    assert np.median(c16) > 0.93 and c16.min() > 0.55, msg
    assert z16 < 2e-2 and v16 < 0.5, msg


def test_bf16_200_step_loss_curve_at_8x1s():
    """200 FusedAdamW steps at B = 8 x 1 s from the same initial weights, fp32 HIP against bf16: both
    curves fall without diverging (every loss finite, never above 1.5x the start), and end within the stated percentage of
    each other (measured: see gpurun_out/parity_bf16_curve200.txt; the trajectories are chaotic step by step -- DESIGN
    section 10 -- so the gate is on where training arrives, over the mean of the last 20 steps)."""
    import os
    from tinyrecurrentunet_amd import network as hn, optim
    from tinyrecurrentunet_amd.stft_loss import MultiResolutionSTFTLoss
    from tinyrecurrentunet_amd.util import loss_fn
    mr = MultiResolutionSTFTLoss(fft_sizes=[512, 1024, 2048], hop_sizes=[50, 120, 240], win_lengths=[240, 600, 1200],
                                 window="hann_window", sc_lambda=0.5, mag_lambda=0.5, band="full").cuda()
    g = torch.Generator(device=DEV)
    g.manual_seed(77)
    B, Ls = 8, 16000
    c = 0.1 * torch.randn((B, 1, Ls + 1), generator=g, device=DEV)
    clean = (0.5 * (c[..., 1:] + c[..., :-1])).contiguous()
    noisy = (clean + 0.05 * torch.randn((B, 1, Ls), generator=g, device=DEV)).contiguous()
    curves = {}
    for prec in ("fp32", "bf16"):
        torch.manual_seed(5)
        net = hn.TRUNet(input_size=4, precision=prec).cuda().train()
        opt = optim.FusedAdamW(net.parameters(), lr=1e-3)
        ls = []
        for _ in range(200):
            opt.zero_grad()
            loss, _ = loss_fn(net, (clean, noisy), 1, 1.0, 1.0, mr)
            loss.backward()
            opt.step()
            ls.append(loss.detach())
        curves[prec] = [float(v) for v in torch.stack(ls).cpu()]
    f, b = curves["fp32"], curves["bf16"]
    tail_f, tail_b = sum(f[-20:]) / 20, sum(b[-20:]) / 20
    worst = max(abs(x - y) / x for x, y in zip(f, b))
    msg = ("200 steps at 8 x 1 s, lr 1e-3: fp32 %.4f -> %.4f (last-20 mean %.4f), bf16 %.4f -> %.4f (last-20 mean %.4f); "
           "largest per-step gap %.2f %%, gap of the last-20 means %.2f %%" % (
               f[0], f[-1], tail_f, b[0], b[-1], tail_b, 100 * worst, 100 * abs(tail_f - tail_b) / tail_f))
    print(msg)
    out_dir = os.path.join(os.path.dirname(os.path.dirname(__file__)), "gpurun_out")
    if os.path.isdir(out_dir):
        open(os.path.join(out_dir, "parity_bf16_curve200.txt"), "a").write(msg + "\n")
    for ls in (f, b):
        assert all(v == v and v < 1.5 * ls[0] for v in ls), msg          # finite, no divergence
        assert sum(ls[-20:]) / 20 < 0.6 * ls[0], msg                      # it trains
    assert abs(tail_f - tail_b) < 0.05 * tail_f, msg


def test_bf16_fused_pointwise_backward_matches_separate_launches():
    """trunet_bf16_pw_bwd (weight gradient + the data gradients of every source in one pass) against the launches it replaces
    (trunet_bf16_wgrad + one trunet_bf16_gemm per source).  Same bf16 operands and MFMA order: the first fused layer of the
    backward (decoder.4's pointwise conv; decoder.5's 8-row layer stays on the separate launches) reproduces the separate
    launches BIT FOR BIT -- all its weight / bias gradients and everything downstream of its data gradients up to the next
    BatchNorm.  From there on the two runs differ by the summation order of the fp32 BatchNorm-backward statistics (1e-7),
    which every following bf16 rounding amplifies towards the bf16 noise floor (measured 1e-7 -> 8e-6 -> 1e-4 -> ... -> 5e-3
    at encoder.0); gate 2e-2, with the conv biases in front of a BatchNorm and the BatchNorm weights whose gradient vanishes
    analytically (see above) measured against their sibling's scale."""
    from tinyrecurrentunet_amd import engine_bf16
    from tinyrecurrentunet_amd.network import TRUNet
    g = torch.Generator(device=DEV)
    g.manual_seed(17)
    N = 700
    x = torch.randn(N, 4, 257, generator=g, device=DEV)
    gout = torch.randn(N, 8, 257, generator=g, device=DEV) / N
    res = []
    old = engine_bf16.FUSED_PWBWD16
    try:
        for fused in (False, True):
            engine_bf16.FUSED_PWBWD16 = fused
            torch.manual_seed(7)
            net = TRUNet(input_size=4, precision="bf16").cuda().train()
            y = net(x)
            y.backward(gout)
            res.append((y.detach().clone(), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}))
    finally:
        engine_bf16.FUSED_PWBWD16 = old
    assert torch.equal(res[0][0], res[1][0])
    sep, fus = res[0][1], res[1][1]
    assert len(fus) == len(sep) and sum(t.numel() for t in fus.values()) == 298592
    bad = []
    for n, a in sep.items():
        b = fus[n]
        if n.startswith(("decoder.5.", "decoder.4.")):
            assert torch.equal(a, b), n
            continue
        sib = n[:-6] + "bias" if n.endswith(".1.weight") else (n[:-4] + "weight" if n.endswith("bias") else n)
        scale = max(a.norm().item(), sep[sib].norm().item() if sib in sep else 0.0)
        if (a - b).norm().item() > 2e-2 * scale:
            bad.append((n, (a - b).norm().item(), scale))
    assert not bad, bad


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_bf16_training_tracks_fp32(seed):
    """Whether the bf16 step is USABLE is a property of optimisation, not of one gradient: 40 FusedAdamW steps on one fixed
    synthetic batch from the same initial weights.  Measured (scripts/dbg/bf16_train_curve.py): e.g. 1.5765 -> 0.7379 in fp32,
    1.5749 -> 0.7408 in bf16 after 60 steps; over seeds 1-4 the curves stay within 0.6-1.0 % of each other at every step
    (2.5 % with the fp32 recurrence kernels between conversions that round 3 replaced by octet I/O: no worse).
    The trajectory itself is chaotic: on seed 0 two FP32 runs that differ only in the summation order of one kernel
    (TRUNET_PWB_KSPLIT=0: 1e-7 perturbations) are 2 % apart around step 22 and meet again, and the bf16 curve leaves the
    fp32 one by 2.5-11 % there depending on which benign variant is built -- so the gate runs on three other seeds and
    bounds every step by 6 %, the last one by 3 %."""
    from tinyrecurrentunet_amd import network as hn, optim
    from tinyrecurrentunet_amd.stft_loss import MultiResolutionSTFTLoss
    from tinyrecurrentunet_amd.util import loss_fn
    mr = MultiResolutionSTFTLoss(fft_sizes=[512, 1024, 2048], hop_sizes=[50, 120, 240], win_lengths=[240, 600, 1200],
                                 window="hann_window", sc_lambda=0.5, mag_lambda=0.5, band="full").cuda()
    g = torch.Generator(device=DEV)
    g.manual_seed(3 + seed)
    B, Ls = 8, 32000
    c = 0.1 * torch.randn((B, 1, Ls + 1), generator=g, device=DEV)
    clean = (0.5 * (c[..., 1:] + c[..., :-1])).contiguous()
    noisy = (clean + 0.05 * torch.randn((B, 1, Ls), generator=g, device=DEV)).contiguous()
    curves = {}
    for prec in ("fp32", "bf16"):
        torch.manual_seed(seed)
        net = hn.TRUNet(input_size=4, precision=prec).cuda().train()
        opt = optim.FusedAdamW(net.parameters(), lr=1e-3)
        ls = []
        for _ in range(40):
            opt.zero_grad()
            loss, _ = loss_fn(net, (clean, noisy), 1, 1.0, 1.0, mr)
            loss.backward()
            opt.step()
            ls.append(loss.item())
        curves[prec] = ls
    f, b = curves["fp32"], curves["bf16"]
    assert f[-1] < 0.7 * f[0] and b[-1] < 0.7 * b[0], (f[0], f[-1], b[0], b[-1])
    assert max(abs(x - y) / x for x, y in zip(f, b)) < 0.06, [round(abs(x - y) / x, 4) for x, y in zip(f, b)]
    assert abs(f[-1] - b[-1]) < 0.03 * f[-1], (f[-1], b[-1])


def test_bf16_fused_transposed_conv_backward_matches_separate_launches():
    """trunet_bf16_convt_bwd against trunet_bf16_wgrad + trunet_bf16_gemm over the tap segments, layer by layer: decoder.4 is
    the first transposed conv of the backward that takes the fused kernel, so its weight / bias / BatchNorm gradients must be
    reproduced (the weight-gradient MFMAs run in another order: 2e-5), and the whole gradient vector must stay within the
    bf16 noise floor of the separate launches (see the pointwise test)."""
    from tinyrecurrentunet_amd import engine_bf16
    from tinyrecurrentunet_amd.network import TRUNet
    g = torch.Generator(device=DEV)
    g.manual_seed(19)
    N = 700
    x = torch.randn(N, 4, 257, generator=g, device=DEV)
    gout = torch.randn(N, 8, 257, generator=g, device=DEV) / N
    res = []
    old = engine_bf16.FUSED_CONVT16
    try:
        for fused in (False, True):
            engine_bf16.FUSED_CONVT16 = fused
            torch.manual_seed(9)
            net = TRUNet(input_size=4, precision="bf16").cuda().train()
            y = net(x)
            y.backward(gout)
            res.append({n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None})
    finally:
        engine_bf16.FUSED_CONVT16 = old
    sep, fus = res
    assert sum(t.numel() for t in fus.values()) == 298592
    for n in ("decoder.5.LastTrCNN.0.weight", "decoder.5.LastTrCNN.3.weight", "decoder.5.LastTrCNN.1.weight"):
        assert torch.equal(sep[n], fus[n]), n                      # upstream of the first fused layer: untouched
    for n in ("decoder.4.TrCNN.3.weight", "decoder.4.TrCNN.3.bias", "decoder.4.TrCNN.4.weight", "decoder.4.TrCNN.4.bias"):
        e = _l2(fus[n], sep[n]) if sep[n].norm().item() > 1e-6 else (fus[n] - sep[n]).norm().item()
        assert e < 5e-5, (n, e)
    bad = []
    for n, a in sep.items():
        b = fus[n]
        sib = n[:-6] + "bias" if n.endswith(".1.weight") else (n[:-4] + "weight" if n.endswith("bias") else n)
        scale = max(a.norm().item(), sep[sib].norm().item() if sib in sep else 0.0)
        if (a - b).norm().item() > 2e-2 * scale:
            bad.append((n, (a - b).norm().item(), scale))
    assert not bad, bad
