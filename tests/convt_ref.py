"""Plain torch restatement of the fused ConvTranspose1d(64 -> 64, K, stride S, padding S/2) + BatchNorm backward
(trunet_convt_bwd_args in include/trunet_hip.h; convt_bwd.hip, bf16_convt.hip), in the kernels' [C][L][NP] layout with
explicit loops over (source position q, tap k):

    dz   = ca dy + (cb z + cc), zero for frames >= N
    pre  = s_scale src + s_shift,   a = max(pre, 0)
    dW[ci][co][k] = sum_{q, n < N} a[ci][q][n] dz[co][q S - pad + k][n]      over the taps with 0 <= p < Lout
    db[co]        = sum dz
    dsrc[ci][q][n] = [pre > 0] sum_{co, k} W[ci][co][k] dz[co][q S - pad + k][n]
    stats[ci]     = (sum_{n < N} dsrc, sum_{n < N} dsrc (src - s_mean))

dtype = float64 is the reference.  float32 is the yardstick `close` measures its tolerance with, in two plain orders:
`blocked` (torch's matmul) and `seq` (ONE strictly sequential fp32 chain over the K * 64 terms of a dsrc element and over
the q * frames terms of a dW element -- the worst plain fp32 order; the MFMA chains lie between the two).  `yardstick`
keeps, element by element, the one further from the reference.  A third order, `permuted` (the blocked one with the frames
and the co channels in a seeded random order), is no part of the yardstick: tests/test_convt_ref_cpu.py holds it and
`blocked` to each other through `close`, which is what checks c and f without a GPU.

bf16 = True emulates the octet contract of trunet_bf16_convt_bwd: dy, z, src and W are bf16 values already; dz and a are
rounded to bf16 before the products (the prologue itself is an fp32 fma, restated as the double expression rounded to
fp32); accumulation is fp32; db is summed from the fp32 dz as it enters the ring, before rounding; the mask comes from the
fp32 pre of the bf16 src; dsrc is rounded to bf16 and the statistics are taken from the rounded values.  For the bf16
kernel the float64 function on the same bf16 inputs is the reference and this emulation the yardstick.

`mut` names ONE deliberate error (tests/test_convt_ref_cpu.py passes such mutants through `close` in place of kernel
output to show that the comparison would catch a subtly wrong kernel); None everywhere else."""
import torch

MUTANTS = ("pad0", "drop_last_tap", "tap_flip", "w_transposed", "clip_last_row", "mask_ge", "mask_raw", "no_mean",
           "pad_frames_counted", "row_swap4")
OUTPUTS = ("dW", "db", "dsrc", "st0", "st1")
C = 64


def lout(Lin, K, S):
    return (Lin - 1) * S - 2 * (S // 2) + K


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def convt_bwd(c, dtype=torch.float64, order="blocked", mut=None, bf16=False):
    """c: namespace with K, S, N and the fp32 tensors dy, z [64][Lout][NP], ca, cb, cc [64], src [64][Lin][NP], s_scale,
    s_shift, s_mean [64], W [64][64][K] (Ci, Co, K).  Returns {dW [64][64][K], db [64], dsrc [64][Lin][NP], st0, st1 [64]}."""
    assert order in ("blocked", "seq", "permuted") and (mut is None or mut in MUTANTS)
    assert not bf16 or dtype == torch.float32
    K, S, N = c.K, c.S, c.N
    pad = 0 if mut == "pad0" else S // 2
    dy, z, src, W = c.dy.to(dtype), c.z.to(dtype), c.src.to(dtype), c.W.to(dtype)
    Lo, NP = dy.shape[1:]
    Lin = src.shape[1]
    assert Lo == lout(Lin, K, S) and dy.shape[0] == src.shape[0] == C
    col = lambda v: v.to(dtype)[:, None, None]
    live = (torch.arange(NP) < N)[None, None, :]
    zero = torch.zeros((), dtype=dtype)
    if bf16:
        d = torch.float64
        inner = (c.cb.to(d)[:, None, None] * c.z.to(d) + c.cc.to(d)[:, None, None]).float()
        dz = (c.ca.to(d)[:, None, None] * c.dy.to(d) + inner.to(d)).float()
        pre = (c.s_scale.to(d)[:, None, None] * c.src.to(d) + c.s_shift.to(d)[:, None, None]).float()
    else:
        dz = col(c.ca) * dy + (col(c.cb) * z + col(c.cc))
        pre = col(c.s_scale) * src + col(c.s_shift)
    if mut != "pad_frames_counted":
        dz = torch.where(live, dz, zero)
    if order == "permuted":
        g = torch.Generator().manual_seed(NP * 64 + Lin)
        pn, pc = torch.randperm(NP, generator=g), torch.randperm(C, generator=g)
    db = dz[:, :, pn].sum((1, 2)) if order == "permuted" else dz.sum((1, 2))
    a = pre.clamp_min(0)
    if bf16:
        dz, a = bf16_round(dz), bf16_round(a)
    mask = pre >= 0 if mut == "mask_ge" else (src > 0 if mut == "mask_raw" else pre > 0)
    p_end = Lo - 1 if mut == "clip_last_row" else Lo
    k_end = K - 1 if mut == "drop_last_tap" else K

    def tap(q, k):
        """row p = q S - pad + k of dz as [co][NP], or None where the tap does not exist"""
        p = q * S - pad + k
        return dz[:, p] if (0 <= p < p_end and k < k_end) else None

    def w_of(k):
        wk = W[:, :, K - 1 - k] if mut == "tap_flip" else W[:, :, k]
        return wk.t() if mut == "w_transposed" else wk

    dW = torch.zeros(C, C, K, dtype=dtype)
    dsrc = torch.zeros(C, Lin, NP, dtype=dtype)
    if order == "blocked":
        for q in range(Lin):
            for k in range(K):
                row = tap(q, k)
                if row is None:
                    continue
                dW[:, :, k] += a[:, q] @ row.t()
                dsrc[:, q] += w_of(k) @ row
    elif order == "permuted":
        for q in range(Lin):
            for k in range(K):
                row = tap(q, k)
                if row is None:
                    continue
                dW[:, :, k] += a[:, q][:, pn] @ row[:, pn].t()
                dsrc[:, q] += w_of(k)[:, pc] @ row[pc]
    else:
        none = torch.zeros(C, NP, dtype=dtype)       # a missing tap adds exact zeros to the chain
        win = torch.stack([torch.stack([none if tap(q, k) is None else tap(q, k) for k in range(K)]) for q in range(Lin)])
        # dsrc: one chain per element over (k, co)
        for k in range(K):
            wk, rows = w_of(k), win[:, k]            # [ci][co], [q][co][NP]
            for co in range(C):
                dsrc += wk[:, co, None, None] * rows[None, :, co]
        # dW: one chain per element over (frame, q)
        at = a.permute(2, 1, 0).contiguous()         # [NP][q][ci]
        wt = win.permute(3, 0, 2, 1).contiguous()    # [NP][q][co][k]
        for n in range(NP):
            for q in range(Lin):
                dW += at[n, q][:, None, None] * wt[n, q][None]
    dsrc = torch.where(mask, dsrc, zero)
    if bf16:
        dsrc = bf16_round(dsrc)
    x = torch.where(live, dsrc, zero)
    cen = src if mut == "no_mean" else src - col(c.s_mean)
    if order == "blocked":
        st0, st1 = x.sum((1, 2)), (x * cen).sum((1, 2))
    elif order == "permuted":
        st0, st1 = x[:, :, pn].sum((1, 2)), (x * cen)[:, :, pn].sum((1, 2))
    else:
        st0, st1 = torch.zeros(C, dtype=dtype), torch.zeros(C, dtype=dtype)
        for q in range(Lin):
            st0 += x[:, q].sum(1)
            st1 += (x[:, q] * cen[:, q]).sum(1)
    if mut == "row_swap4":
        # rows r <-> r + 4 inside every group of 8: in the MFMA C layout a lane's accumulator registers hold rows
        # r .. r + 3 and the other half-wave's lane the rows four further
        dW = dW.index_select(0, torch.arange(C) ^ 4)
    return {"dW": dW, "db": db, "dsrc": dsrc, "st0": st0, "st1": st1}


def yardstick(ref64, blocked, seq):
    """element by element the fp32 result that lies further from the reference"""
    out = {}
    for k in OUTPUTS:
        worse = (seq[k].double() - ref64[k]).abs() > (blocked[k].double() - ref64[k]).abs()
        out[k] = torch.where(worse, seq[k], blocked[k])
    return out


CLOSE_C = 4.0
CLOSE_F = 8 * 2.0 ** -24


def bound(ref64, yard, c=CLOSE_C, f=CLOSE_F):
    """(e_y, bound on the max error, rel_y, bound on the relative L2) of `close`"""
    d = yard.double() - ref64
    nrm = float(ref64.norm()) + 1e-300
    e_y, rel_y = float(d.abs().max()), float(d.norm()) / nrm
    return e_y, c * e_y + f * float(ref64.abs().max()), rel_y, c * rel_y + 1e-6


def close(got, ref64, yard, what):
    """The one comparison of the ConvTranspose backward tests.  The tolerance is measured on the same inputs, against the
    reference and never against the kernel: e_y = max|yardstick - fp64|, rel_y = relative L2 of the same difference.
    Required: every value finite, max|got - fp64| <= c e_y + f max|fp64|, relative L2 <= c rel_y + 1e-6; no element is
    left out.  Returns (err, e_y, bound, rel, rel_bound).

    c = 4: another summation order in the MFMA (gru_ref.close's constant).

    f = 8 * 2^-24 = 4.8e-7 is the floor for results whose yardstick error happens to vanish (a single product that is
    exact in fp32, a sum of one term); units of 2^-24 relative to the result, for a result that is one K-step of the MFMA:
      1   the fp32 rounding of the stored result (round to nearest: 2^-24);
      1   the operand truncation of the three-term split: x3_common.hpp drops the products a1 b2, a2 b1, a2 b2 and the
          residue of lo, together below 2^-24 |a b| (the fp32-MFMA and bf16 instances have no such term);
      6   the split instance adds its six partial products into the fp32 accumulator one MFMA after the other: six
          accumulator roundings where the yardstick's chain has one (the fp32 MFMA rounds once per product).
    Everything that grows with the number of terms -- the product and accumulator roundings along the chains, the
    roundings of the dz and pre prologues (the kernels use fma, the restatement a multiply and an add) -- is what e_y
    measures on the same inputs, and c covers the order."""
    got, ref64, yard = got.detach().cpu(), ref64.detach().cpu(), yard.detach().cpu()
    assert ref64.dtype == torch.float64 and got.shape == ref64.shape == yard.shape, (what, got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), "%s: not finite" % what
    assert bool(torch.isfinite(ref64).all()) and bool(torch.isfinite(yard).all()), "%s: reference not finite" % what
    e_y, bnd, rel_y, rbound = bound(ref64, yard)
    d = got.double() - ref64
    err, rel = float(d.abs().max()), float(d.norm()) / (float(ref64.norm()) + 1e-300)
    assert err <= bnd, "%s: max error %.3e > bound %.3e (e_y %.3e)" % (what, err, bnd, e_y)
    assert rel <= rbound, "%s: relative L2 %.3e > bound %.3e (rel_y %.3e)" % (what, rel, rbound, rel_y)
    return err, e_y, bnd, rel, rbound
