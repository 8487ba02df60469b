"""Plain torch restatement of the fused backward of a Conv1d(k = 1) + BatchNorm layer on bf16 octet tensors
(trunet_bf16_pw_bwd and trunet_bf16_wgrad in include/trunet_hip.h; bwgrad_kernel in csrc/bf16.hip), on fp32 tensors in the
kernels' [C][L][NP] layout:

    dz   = ca dy + (cb z + cc), zero for frames >= N;  db = sum dz (from the UNROUNDED dz);  dz -> bf16 for both GEMMs
    act_s = bf16(relu(c0 x_s + c1)) for a BN+ReLU source, x_s for a plain one
    dW[m][woff_s + c] = sum_{p, n < N} dz[m][p][n] act_s[c][p + off_s][n]            over 0 <= p + off_s < L_s
    g_s[c][p + off_s][n] = sum_m bf16(W)[m][woff_s + c] dz[m][p][n]  (+ prev with ACCUM), zero where the mask fails
                          (MASK: c0 x + c1 <= 0 for a BN source, x <= 0 for a plain one), rounded to bf16 and stored for
                          EVERY frame (dz = 0 for n >= N); positions no p reaches keep what out[s] held
    st0_s[c] = sum_{n < N} g_s,  st1_s[c] = sum_{n < N} g_s (x_s - mean_s)         from the STORED, rounded g_s

A case `c` is a namespace with M, N, NP, P, the fp32 tensors dy, z [M][P][NP], ca, cb, cc [M], W [M][K], and
c.segs: namespaces with nchan, L, off, woff, bn, mask, stats, accum, x / prev [nchan][L][NP], c0, c1, mean [nchan].

dtype = float64 with bf16 = False is the reference of the `ordinary` comparisons (the same bf16-valued inputs, no rounding
of any intermediate); float32 with bf16 = True emulates the kernel and is the yardstick convt_ref.close measures its
tolerance with: the prologues are fp32 fmas, restated as the double expression rounded to fp32 (dy, z, x are 8-bit values:
the double product is exact), accumulation is fp32 in the `order` asked for -- `blocked` (one fp32 matmul per (position, 64
frames) step, the kernel's own grouping), `seq` (one strictly sequential chain over the frames of a dW element, over the m
of a g element) and `permuted` (blocked with the frames and the dz channels in a seeded random order).  float64 with
bf16 = True is the reference of the `exact` regime, where every sum holds its exact value and only the 8-bit roundings
remain: all dtypes and orders then agree bit for bit.  absval = True sums the magnitudes of the terms of every output
instead (the largest partial sum any order can meet: the unit budget of the exact regime).

`mut` names ONE deliberate error, a plausible kernel mistake; tests/test_pwbwd16_ref_cpu.py shows that each is rejected."""
import torch

from convt_ref import CLOSE_C, CLOSE_F, bf16_round, bound, close  # noqa: F401  (the one comparison, shared)

MUTANTS = ("mask_ge", "mask_from_activated", "no_mean", "pad_frames_counted", "shift_sign", "seg_woff_swapped",
           "w_not_transposed", "accum_dropped", "accum_after_mask", "dz_unrounded", "db_from_rounded_dz",
           "stats_from_unrounded", "unvisited_zeroed")
ORDERS = ("blocked", "seq", "permuted")
STEP = 64                                  # frames of a kernel step


def outputs(c):
    """names of the outputs of a case, in report order"""
    out = ["dW", "db"]
    for i, s in enumerate(c.segs):
        out.append("g%d" % i)
        if s.stats:
            out += ["st0_%d" % i, "st1_%d" % i]
    return out


def p_range(s, P, mut=None):
    """[p0, p1): the positions p with 0 <= p + off < L, and the shift actually applied"""
    off = -s.off if mut == "shift_sign" else s.off
    return max(0, -off), min(P, s.L - off), off


def pw_bwd(c, dtype=torch.float64, order="blocked", mut=None, bf16=True, absval=False):
    assert order in ORDERS and (mut is None or mut in MUTANTS)
    D, d = dtype, torch.float64
    dev = c.dy.device
    M, N, NP, P = c.M, c.N, c.NP, c.P
    fma = (lambda t: t.float().to(D)) if D == torch.float32 else (lambda t: t)     # the rounding of one fp32 fma
    rb = bf16_round if bf16 else (lambda t: t)
    col = lambda v, T=d: v.to(T)[:, None, None]
    zero = torch.zeros((), dtype=D, device=dev)
    live = (torch.arange(NP, device=dev) < N)[None, None, :]
    g = torch.Generator().manual_seed(1000 * NP + 10 * P + M)
    pn, pm = torch.randperm(NP, generator=g).to(dev), torch.randperm(M, generator=g).to(dev)

    dz = fma(col(c.ca) * c.dy.to(d) + fma(col(c.cb) * c.z.to(d) + col(c.cc)).to(d)).to(D)
    if mut != "pad_frames_counted":
        dz = torch.where(live, dz, zero)
    dzr = dz if mut == "dz_unrounded" else rb(dz)
    dzb = dzr if mut == "db_from_rounded_dz" else dz
    if absval:
        dzr, dzb = dzr.abs(), dzb.abs()

    def fsum(t):
        """sum over (position, frame) of t [C][p][NP] in the order asked for"""
        if order == "seq":
            acc = torch.zeros(t.shape[0], dtype=D, device=dev)
            for p in range(t.shape[1]):
                for n in range(NP):
                    acc += t[:, p, n]
            return acc
        return (t[:, :, pn] if order == "permuted" else t).sum((1, 2))

    out = {"db": fsum(dzb)}
    true = pw_bwd(c, dtype, order, mut, bf16) if absval else None      # the statistics' terms are the STORED gradients
    W = rb(c.W.to(D))
    if absval:
        W = W.abs()
    dW = torch.zeros(M, W.shape[1], dtype=D, device=dev)
    woffs = [s.woff for s in c.segs]
    if mut == "seg_woff_swapped":
        woffs = woffs[::-1]
    for i, s in enumerate(c.segs):
        x = s.x.to(D)
        if s.bn:
            pre = fma(col(s.c0) * s.x.to(d) + col(s.c1)).to(D)
            act = rb(pre.clamp_min(0))
        else:
            pre, act = x, x
        if mut == "mask_from_activated":
            pre = fma(col(s.c0) * act.to(d) + col(s.c1)).to(D) if s.bn else act
        mask = (pre >= 0) if mut == "mask_ge" else (pre > 0)
        if absval:
            act = act.abs()
        p0, p1, off = p_range(s, P, mut)
        woff = woffs[i]
        Ws = W[:, woff:woff + s.nchan]                       # [M][nchan]
        if mut == "w_not_transposed":
            Ws = Ws.reshape(s.nchan, M).t()
        prev = s.prev.to(D)
        gs = torch.zeros_like(prev) if mut == "unvisited_zeroed" else prev.clone()
        if p1 > p0:
            Z, A = dzr[:, p0:p1], act[:, p0 + off:p1 + off]        # [M][np][NP], [nchan][np][NP]
            dWs = torch.zeros(M, s.nchan, dtype=D, device=dev)
            if order == "seq":
                for p in range(p1 - p0):
                    for n in range(NP):
                        dWs.addmm_(Z[:, p, n:n + 1], A[:, p, n:n + 1].t())
                gv = torch.zeros(s.nchan, p1 - p0, NP, dtype=D, device=dev)
                for m in range(M):
                    gv += Ws[m][:, None, None] * Z[m][None]
            else:
                if order == "permuted":
                    Z, A = Z[:, :, pn], A[:, :, pn]
                for p in range(p1 - p0):
                    for n0 in range(0, NP, STEP):
                        dWs.addmm_(Z[:, p, n0:n0 + STEP], A[:, p, n0:n0 + STEP].t())
                if order == "permuted":
                    gv = torch.einsum("mc,mpn->cpn", Ws[pm], dzr[pm, p0:p1])
                else:
                    gv = torch.einsum("mc,mpn->cpn", Ws, dzr[:, p0:p1])
            dW[:, woff:woff + s.nchan] = dWs
            pv, mk = prev[:, p0 + off:p1 + off], mask[:, p0 + off:p1 + off]
            if absval:
                pv = pv.abs()
            if s.accum and mut == "accum_after_mask":
                gv = (torch.where(mk, gv, zero) if s.mask else gv) + pv
            else:
                if s.accum and mut != "accum_dropped":
                    gv = gv + pv
                if s.mask:
                    gv = torch.where(mk, gv, zero)
            gr = rb(gv)
            gs[:, p0 + off:p1 + off] = gr
            if s.stats:
                xs = gv if mut == "stats_from_unrounded" else gr
                if absval:
                    xs = true["g%d" % i][:, p0 + off:p1 + off]
                if mut != "pad_frames_counted":
                    xs = torch.where(live, xs, zero)
                cen = x[:, p0 + off:p1 + off] - (0 if mut == "no_mean" else col(s.mean, D))
                if absval:
                    xs, cen = xs.abs(), cen.abs()
                out["st0_%d" % i], out["st1_%d" % i] = fsum(xs), fsum(xs * cen)
        elif s.stats:
            out["st0_%d" % i] = out["st1_%d" % i] = torch.zeros(s.nchan, dtype=D, device=dev)
        out["g%d" % i] = gs
    out["dW"] = dW
    return out


def yardstick(ref64, *orders):
    """element by element the fp32 result that lies furthest from the reference (convt_ref.yardstick for dict outputs of
    any names)"""
    out = {}
    for k in ref64:
        best = orders[0][k]
        for o in orders[1:]:
            worse = (o[k].double() - ref64[k]).abs() > (best.double() - ref64[k]).abs()
            best = torch.where(worse, o[k], best)
        out[k] = best
    return out
