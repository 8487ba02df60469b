"""Plain torch restatement of the bf16 implicit GEMM (trunet_bf16_gemm in include/trunet_hip.h; bgemm_kernel in csrc/bf16.hip)
and of the weight packer (trunet_bf16_pack_weight, pack_weight_kernel), on fp32 tensors in the kernels' [C][L][NP] layout:

    v_s  = x_s                                   TRUNET_PRO_NONE: the raw operand
           bf16(relu(fma(c0, x_s, c1)))          TRUNET_PRO_BNRELU
           bf16(fma(ca, x_s, fma(cb, z_s, cc)))  TRUNET_PRO_BNBWD
    a segment contributes at position p only where qn = p pos_mul + pos_off is >= 0, is divisible by pos_div and
    q = qn / pos_div < L_s
    acc[m][p][n] = sum_s sum_ch bf16(W[(m + w_m_off) ldw_m + ch ldw_c + woff_s]) v_s[ch][q_s(p)][n]
    val = acc + bias[m]  (+ old[m][p + out_pos_off][n] with ACCUM: a bf16 value);  MASK: 0 unless fma(e0, zmask, e1) > 0;
          RELU: max(., 0);  rows m >= M of the last octet: 0
    out[m][p + out_pos_off][n] = r = bf16(val), stored for EVERY frame;  F32OUT: fp32 row m_out_off + m holds val itself and
          the bias is bias[m + m_out_off]
    st0[m] = sum_{p, n < N} r,   st1[m] = sum r^2, or sum r (zmask - e2) with MASK       from the STORED, rounded values
    positions of `out` outside [p_begin, p_begin + P) + out_pos_off keep their old contents

A plain segment next to a BN+ReLU one gets identity coefficients in the compile-time BN+ReLU instances, relu(1 x + 0): the
host contract makes it a post-ReLU source (x >= 0), for which that is x.

A case `c` is a namespace with NP, N, P, p_begin, M, out_L, out_pos_off, w_m_off, ldw_m, ldw_c, the flags bias, stats,
accum, mask, relu, f32out, chunks (row offsets of the launches that share `out`: (0,) but for the GRU input projection, whose
launch at offset o has m_out_off = o and w_m_off + o), the fp32 tensors W (flat), b, old and zmask [8 ceil(M/8)][out_L][NP],
e0, e1, e2 [M], and c.segs: namespaces with nchan, L, pos_mul, pos_off, pos_div, woff, mode, x (, z) [nchan][L][NP] and the
coefficients c0, c1 (, c2).

dtype / order / bf16 / absval / mut as tests/pwbwd16_ref.pw_bwd: float64 with bf16 = False is the reference of the
`ordinary` comparisons; float32 with bf16 = True is the kernel's emulation and the yardstick, with the K axis summed in the
`order` asked for -- `blocked` (one fp32 product per 16-channel k-step, in the kernel's segment order), `seq` (one strictly
sequential chain over the channels) and `permuted` (blocked over the channels of all segments in a seeded random order);
float64 with bf16 = True is the reference of the `exact` regime.  absval = True sums magnitudes (the unit budget of the
exact regime).  `mut` names ONE deliberate error; tests/test_bgemm_ref_cpu.py shows that each is rejected."""
import torch

from convt_ref import CLOSE_C, CLOSE_F, bf16_round, bound, close  # noqa: F401  (the one comparison, shared)
from pwbwd16_ref import yardstick  # noqa: F401

MUTANTS = ("mask_ge", "mask_after_relu_swapped", "accum_dropped", "stats_from_unrounded", "pad_frames_counted",
           "st1_no_center", "pos_off_sign", "pos_div_ignored", "seg_woff_swapped", "w_m_off_dropped",
           "bias_m_out_off_dropped", "unvisited_zeroed", "tail_rows_not_zeroed", "prologue_unrounded", "rne_as_truncate",
           "plain_in_bnrelu_not_identity")
ORDERS = ("blocked", "seq", "permuted")
NONE, BNRELU, BNBWD = 0, 1, 2              # TRUNET_PRO_*
KSTEP = 16                                 # channels of a k-step


def bf16_truncate(t):
    """round toward zero to 8 significant bits (the mutant of the round-to-nearest-even store)"""
    f = t.float()
    assert torch.equal(f.to(t.dtype), t)
    return (f.view(torch.int32) & -65536).view(torch.float32).to(t.dtype)


def ksteps(nchan):
    return ((nchan + 7) // 8 + 1) // 2


def seg_q(s, p, mut=None):
    """source position of output position p, or None where the segment does not contribute"""
    qn = p * s.pos_mul + (-s.pos_off if mut == "pos_off_sign" else s.pos_off)
    if qn < 0 or (qn % s.pos_div and mut != "pos_div_ignored") or qn // s.pos_div >= s.L:
        return None
    return qn // s.pos_div


def launch_pro(c):
    """prologue class of the launch, as the dispatch takes it"""
    modes = [s.mode for s in c.segs]
    return BNBWD if BNBWD in modes else (BNRELU if BNRELU in modes else NONE)


def outputs(c):
    return ["out"] + (["st0", "st1"] if c.stats else [])


def window(c):
    """the positions of `out` the launch owns"""
    return slice(c.p_begin + c.out_pos_off, c.p_begin + c.P + c.out_pos_off)


def weight(c, s, w_m_off, woff, D, rb, Mp):
    """[Mp][nchan]: bf16(W[(m + w_m_off) ldw_m + ch ldw_c + woff]), zero rows for m >= M"""
    m, ch = torch.arange(c.M)[:, None], torch.arange(s.nchan)[None, :]
    A = torch.zeros(Mp, s.nchan, dtype=D, device=c.W.device)
    A[:c.M] = rb(c.W.reshape(-1)[((m + w_m_off) * c.ldw_m + ch * c.ldw_c + woff).to(c.W.device)].to(D))
    return A


def bgemm(c, dtype=torch.float64, order="blocked", mut=None, bf16=True, absval=False, raw=False):
    """{"out": [8 ceil(M/8)][out_L][NP] (F32OUT: [rows of c.old][out_L][NP]), "st0", "st1": [M]} in `dtype`; raw = True adds
    "raw": the rows as they stand before the store's rounding"""
    assert order in ORDERS and (mut is None or mut in MUTANTS)
    D, d = dtype, torch.float64
    dev = c.W.device
    M, N, NP = c.M, c.N, c.NP
    Mp = (M + 7) // 8 * 8
    fma = (lambda t: t.float().to(D)) if D == torch.float32 else (lambda t: t)     # the rounding of one fp32 fma
    rnd = bf16_truncate if mut == "rne_as_truncate" else bf16_round
    rb = rnd if bf16 else (lambda t: t)
    rbw = bf16_round if bf16 else (lambda t: t)                                     # the packer's rounding
    col = lambda v, T=d: v.to(T)[:, None, None]
    zero = torch.zeros((), dtype=D, device=dev)
    live = (torch.arange(NP, device=dev) < N)[None, :]
    K = sum(s.nchan for s in c.segs)
    g = torch.Generator().manual_seed(1000 * NP + 10 * c.P + M)
    pk, pn = torch.randperm(K, generator=g).to(dev), torch.randperm(NP, generator=g).to(dev)
    pro = launch_pro(c)
    true = bgemm(c, dtype, order, mut, bf16) if absval else None        # the statistics' terms are the STORED values

    # ---- prologue of every segment, once for all positions
    vs = []
    for s in c.segs:
        x = s.x.to(d)
        if s.mode == BNRELU:
            v = fma(col(s.c0) * x + col(s.c1)).to(D).clamp_min(0)
            v = v if mut == "prologue_unrounded" else rb(v)
        elif s.mode == BNBWD:
            v = fma(col(s.c0) * x + fma(col(s.c1) * s.z.to(d) + col(s.c2)).to(d)).to(D)
            v = v if mut == "prologue_unrounded" else rb(v)
        else:
            v = x.to(D)
            if pro == BNRELU and mut == "plain_in_bnrelu_not_identity":
                v = torch.zeros_like(v)                       # coefficients left at zero: relu(0 x + 0)
        vs.append(v.abs() if absval else v)
    woffs = [s.woff for s in c.segs]
    if mut == "seg_woff_swapped":
        woffs = woffs[::-1]

    F32 = c.f32out
    old = c.old.to(D)
    out = torch.zeros_like(old) if mut == "unvisited_zeroed" else old.clone()
    unrounded = out.clone() if raw else None
    st0, st1 = torch.zeros(M, dtype=D, device=dev), torch.zeros(M, dtype=D, device=dev)
    for off in c.chunks:
        w_m_off = 0 if mut == "w_m_off_dropped" else c.w_m_off + off
        As = [weight(c, s, w_m_off, wo, D, rbw, Mp) for s, wo in zip(c.segs, woffs)]
        if absval:
            As = [A.abs() for A in As]
        bias = torch.zeros(Mp, dtype=D, device=dev)
        if c.bias:
            b0 = 0 if (mut == "bias_m_out_off_dropped" or not F32) else off
            bias[:M] = c.b[b0:b0 + M].to(D)
        rows = slice(off, off + M) if F32 else slice(0, Mp)
        for p in range(c.p_begin, c.p_begin + c.P):
            po = p + c.out_pos_off
            acc = torch.zeros(Mp, NP, dtype=D, device=dev)
            terms = [(A, v[:, q]) for A, v, s in zip(As, vs, c.segs) for q in [seg_q(s, p, mut)] if q is not None]
            if terms and order == "permuted":
                A, v = torch.cat([t[0] for t in terms], 1), torch.cat([t[1] for t in terms], 0)
                k = pk[pk < A.shape[1]]
                terms = [(A[:, k], v[k])]
            for A, v in terms:
                if order == "seq":
                    for ch in range(A.shape[1]):
                        acc += A[:, ch, None] * v[ch][None, :]
                else:
                    for k0 in range(0, A.shape[1], KSTEP):
                        acc += A[:, k0:k0 + KSTEP] @ v[k0:k0 + KSTEP]
            val = acc + (bias.abs() if absval else bias)[:, None]
            if F32:
                out[rows, po] = val[:M]
                continue
            prev = old[:, po].abs() if absval else old[:, po]
            keep = None
            if c.mask:
                e = lambda v: torch.cat([v.to(d), torch.zeros(Mp - M, dtype=d, device=dev)])[:, None]
                pre = fma(e(c.e0) * c.zmask[:, po].to(d) + e(c.e1)).to(D)
                keep = (pre >= 0) if mut == "mask_ge" else (pre > 0)
            if c.accum and mut == "mask_after_relu_swapped":
                val = (torch.where(keep, val, zero) if c.mask else val) + prev
            else:
                if c.accum and mut != "accum_dropped":
                    val = val + prev
                if c.mask:
                    val = torch.where(keep, val, zero)
            if c.relu:
                val = val.clamp_min(0)
            if mut != "tail_rows_not_zeroed":
                val[M:] = 0
            r = rb(val)
            out[:, po] = r
            if raw:
                unrounded[:, po] = val
            if c.stats:
                xs = val if mut == "stats_from_unrounded" else r
                if absval:
                    xs = true["out"][:, po].to(D)
                if mut != "pad_frames_counted":
                    xs = torch.where(live, xs, zero)
                if c.mask:
                    cen = (c.zmask[:M, po].to(D) - (0 if mut == "st1_no_center" else c.e2.to(D)[:, None]))
                else:
                    cen = xs[:M]
                xs = xs[:M]
                if absval:
                    xs, cen = xs.abs(), cen.abs()
                t0, t1 = xs, xs * cen
                if order == "permuted":
                    t0, t1 = t0[:, pn], t1[:, pn]
                st0 += t0.sum(1)
                st1 += t1.sum(1)
    res = {"out": out}
    if raw:
        res["raw"] = unrounded
    if c.stats:
        res["st0"], res["st1"] = st0, st1
    return res


def pack_image(W, M, ldw_m, ldw_c, w_m_off, segs):
    """the int16 image of pack_weight_kernel, [ceil(M/32)][nks_total][64 lanes][8]: element (rt, ks, lane, j) holds
    bf16(W[(m + w_m_off) ldw_m + ch ldw_c + woff_s]) for m = 32 rt + lane % 32, ch = 16 (ks - ks0_s) + 8 (lane / 32) + j of the
    segment s that owns k-step ks; zero for m >= M or ch >= nchan_s.  segs: (nchan, woff) pairs."""
    Wf = W.reshape(-1).float().cpu()
    nks = sum(ksteps(n) for n, _ in segs)
    nrt = (M + 31) // 32
    img = torch.zeros(nrt, nks, 64, 8, dtype=torch.bfloat16)
    rt, lane, j = torch.arange(nrt)[:, None, None, None], torch.arange(64)[None, None, :, None], torch.arange(8)
    m = 32 * rt + lane % 32                                                 # [nrt][1][64][1]
    ks0 = 0
    for nchan, woff in segs:
        n = ksteps(nchan)
        ch = 16 * torch.arange(n)[None, :, None, None] + 8 * (lane // 32) + j    # [1][n][64][8]
        ok = (m < M) & (ch < nchan)
        idx = ((m + w_m_off) * ldw_m + ch * ldw_c + woff) * ok                  # 0 where the element is padding
        img[:, ks0:ks0 + n] = torch.where(ok, Wf[idx], torch.zeros(())).to(torch.bfloat16)
        ks0 += n
    return img.view(torch.int16)
