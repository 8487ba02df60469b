"""Plain torch restatement of the fp32 weight gradient and fused pointwise backward (trunet_wgrad_args, trunet_pwbwd_args
in include/trunet_hip.h; conv_wgrad_kernel in csrc/gemm_conv.hip, csrc/wgrad_small.hip, pw_bwd_kernel in csrc/pw_bwd.hip), in
the kernels' [C][L][NP] layout, for general segments:

    dz[m][p][n] = ac0 a0 + (ac1 a1 + ac2) at row m + a_m_off, position p + a_pos_off (a_mode BNBWD; a0 itself for NONE),
                  zero for frames >= N;  p = p_begin .. p_begin + P - 1
    q_s(p)      = (p pos_mul + pos_off) / pos_div; the segment takes no part at p where that is negative, fractional or >= L
    act_s       = max(c0 x_s + c1, 0) for a BN+ReLU segment, x_s for a plain one
    dW[(m + w_m_off) ldw_m + c ldw_c + woff_s] = sum_{p, n < N} dz[m][p][n] act_s[c][q_s(p)][n]
                  as a full image of w_numel elements: what no (m, c, s) addresses is zero and part of the comparison
    db[b_off + m] = sum_{p, n} dz[m][p][n]                                            a row of b_len elements, zero elsewhere
    g_s[c][q_s(p)][n] = sum_m W[(m + w_m_off) ldw_m + c ldw_c + woff_s] dz[m][p][n]  (+ prev with ACCUM, added BEFORE the
                  mask), zero where MASK fails (c0 x + c1 <= 0; x <= 0 for a plain segment).  Stored for EVERY frame of a
                  visited position: dz = 0 for n >= N, so the padding columns hold 0, or mask(prev) with ACCUM.  Positions no
                  p reaches keep what out[s] held.
    st0_s[c] = sum_{n < N} g_s,  st1_s[c] = sum_{n < N} g_s (x_s - mean_s)

A case `c` is a namespace with N, NP, P, p_begin, M, a_L, a_pos_off, a_m_off, bnbwd, the tensors dy, z [rows][a_L][NP] and ca,
cb, cc [rows] (rows >= a_m_off + M: the row block of a wider layer), ldw_m, ldw_c, w_m_off, w_numel, W [w_numel] (the weight,
addressed like the image), b_len, b_off and c.segs: namespaces with nchan, L, pos_mul, pos_off, pos_div, woff, bn, store,
mask, stats, accum, x / prev [nchan][L][NP], c0, c1, mean [nchan].

dtype = float64 is the reference.  float32 is the yardstick convt_ref.close measures its tolerance with, in the orders
`blocked` (one torch matmul over all (position, frame) terms), `seq` (one strictly sequential fp32 chain over the frames of a
dW element and over the m of a g element) and `permuted` (blocked with frames and dz rows in a seeded random order; no part
of the yardstick).  The two prologues are single fmas in the kernels, restated in every dtype as the double expression
rounded to the dtype: a correctly rounded fma has the sign of the exact value, so float64 and the kernels agree on every
mask bit and no comparison leaves an element out.

The second statistics column: float64 uses x_s - mean.  The kernel does not read x_s again; where the mask passes it
recovers x - mean = a / c0 - (c1 / c0 + mean) from the staged activation a (pw_bwd.hip, CZ), except for channels with
|c0| < 1e-30 or |c1| > 65536 |c0|, where it loads x.  The float32 orders restate exactly that, so the rounding of a carried
through 1 / c0 is part of the yardstick's own error and `close` needs no extra term for it.

absval = True sums the magnitudes of the terms of every output (the largest partial sum any order can meet).
`mut` names ONE deliberate error, a plausible kernel mistake; tests/test_pwbwd_ref_cpu.py shows that each is rejected."""
import torch

from convt_ref import CLOSE_C, CLOSE_F, bound, close  # noqa: F401  (the one comparison, shared)
from pwbwd16_ref import yardstick  # noqa: F401  (convt_ref.yardstick for dict outputs of any names)

MUTANTS = ("pad_frames_counted", "last_tile_dropped", "cc_dropped", "mask_ge", "mask_raw", "accum_after_mask", "no_mean",
           "shift_off_by_one", "woff_ignored", "w_transposed", "row_swap4", "clamped_row_counted", "a_m_off_ignored",
           "b_off_ignored")
ORDERS = ("blocked", "seq", "permuted")
TILE = 32                                  # frames of a tile


def outputs(c):
    """names of the outputs of a case, in report order"""
    out = ["dW", "db"]
    for i, s in enumerate(c.segs):
        if s.store:
            out.append("g%d" % i)
            if s.stats:
                out += ["st0_%d" % i, "st1_%d" % i]
    return out


def positions(s, c, mut=None):
    """(ps, qs): the positions p - p_begin in [0, P) at which the segment takes part, and its own position q there"""
    off = s.pos_off + (1 if mut == "shift_off_by_one" else 0)
    ps, qs = [], []
    for i in range(c.P):
        num = (c.p_begin + i) * s.pos_mul + off
        if num >= 0 and num % s.pos_div == 0 and num // s.pos_div < s.L:
            ps.append(i)
            qs.append(num // s.pos_div)
    return ps, qs


def w_index(c, s, mut=None):
    """[M][nchan] element index of A(m, c) in the weight / in a partial image"""
    m = torch.arange(c.M)[:, None] + c.w_m_off
    ch = torch.arange(s.nchan)[None, :]
    return m * c.ldw_m + ch * c.ldw_c + (0 if mut == "woff_ignored" else s.woff)


def padded_rows(M):
    """rows of the dz block trunet_pw_bwd stages for M rows (pw_bwd.hip: MA)"""
    return 32 if M <= 32 else (64 if M <= 64 else 128)


def slow_stat_channel(c0, c1):
    """pw_bwd.hip: the channels whose z of the statistics is loaded, not recovered from the activation"""
    return (c0.abs() < 1e-30) | (c1.abs() > 65536.0 * c0.abs())


def pw_bwd(c, dtype=torch.float64, order="blocked", mut=None, absval=False):
    assert order in ORDERS and (mut is None or mut in MUTANTS)
    D, d = dtype, torch.float64
    dev = c.dy.device
    M, N, NP = c.M, c.N, c.NP
    rnd = lambda t: t.to(D)                                        # the rounding of one fma
    col = lambda v, T=d: v.to(T)[:, None, None]
    zero = torch.zeros((), dtype=D, device=dev)
    live = (torch.arange(NP, device=dev) < N)[None, None, :]
    g = torch.Generator().manual_seed(1000 * NP + 10 * c.P + M)
    pn, pm = torch.randperm(NP, generator=g).to(dev), torch.randperm(M, generator=g).to(dev)

    r0 = 0 if mut == "a_m_off_ignored" else c.a_m_off
    rows = slice(r0, r0 + M)
    pos = slice(c.p_begin + c.a_pos_off, c.p_begin + c.a_pos_off + c.P)
    dy = c.dy[rows, pos]
    if c.bnbwd:
        cc = torch.zeros_like(c.cc[rows]) if mut == "cc_dropped" else c.cc[rows]
        inner = rnd(col(c.cb[rows]) * c.z[rows, pos].to(d) + col(cc))
        dz = rnd(col(c.ca[rows]) * dy.to(d) + inner.to(d))
    else:
        dz = dy.to(D)
    if mut != "pad_frames_counted":
        dz = torch.where(live, dz, zero)
    dzs = dz                                                       # what the sums over frames see
    if mut == "last_tile_dropped":
        t_last = (N - 1) // TILE * TILE
        dzs = torch.where((torch.arange(NP, device=dev) >= t_last)[None, None, :], zero, dz)
    if absval:
        dz, dzs = dz.abs(), dzs.abs()

    def fsum(t):
        """sum over (position, frame) of t [C][p][NP] in the order asked for"""
        if order == "seq":
            acc = torch.zeros(t.shape[0], dtype=D, device=dev)
            for p in range(t.shape[1]):
                for n in range(NP):
                    acc += t[:, p, n]
            return acc
        return (t[:, :, pn] if order == "permuted" else t).sum((1, 2))

    db = torch.zeros(c.b_len, dtype=D, device=dev)
    b0 = 0 if mut == "b_off_ignored" else c.b_off
    dbm = fsum(dzs)
    npad = padded_rows(M) - M                                      # dz rows the MFMA tile holds beyond M
    if mut == "clamped_row_counted":
        dbm[M - 1] = dbm[M - 1] * (1 + npad)
    db[b0:b0 + M] = dbm
    out = {"db": db}
    true = pw_bwd(c, dtype, order, mut) if absval else None        # the statistics' terms are the STORED gradients
    Wf = c.W.to(D)
    if absval:
        Wf = Wf.abs()
    dW = torch.zeros(c.w_numel, dtype=D, device=dev)
    for i, s in enumerate(c.segs):
        x = s.x.to(D)
        if s.bn:
            pre = rnd(col(s.c0) * s.x.to(d) + col(s.c1))
            act = pre.clamp_min(0)
        else:
            pre, act = x, x
        mask = (pre >= 0) if mut == "mask_ge" else ((x > 0) if mut == "mask_raw" else (pre > 0))
        if absval:
            act = act.abs()
        ps, qs = positions(s, c, mut)
        idx = w_index(c, s, mut).to(dev)
        Ws = Wf[idx]                                               # [M][nchan]
        if mut == "w_transposed" and M == s.nchan:
            Ws = Ws.t()
        elif mut == "w_transposed":
            Ws = Ws.reshape(s.nchan, M).t()
        prev = s.prev.to(D) if s.store else None
        gs = prev.clone() if s.store else None
        if ps:
            Z, Zs, A = dz[:, ps], dzs[:, ps], act[:, qs]          # [M][np][NP], [nchan][np][NP]
            dWs = torch.zeros(M, s.nchan, dtype=D, device=dev)
            if order == "seq":
                for p in range(len(ps)):
                    for n in range(NP):
                        dWs.addmm_(Zs[:, p, n:n + 1], A[:, p, n:n + 1].t())
            else:
                Zw, Aw = (Zs[:, :, pn], A[:, :, pn]) if order == "permuted" else (Zs, A)
                dWs = Zw.reshape(M, -1) @ Aw.reshape(s.nchan, -1).t()
            if mut == "row_swap4":
                # rows r <-> r + 4 inside every group of 8: a lane's accumulator registers hold rows r .. r + 3 of the MFMA C
                # layout and the other half-wave's lane the rows four further
                dWs = dWs.index_select(0, (torch.arange(M) ^ 4).clamp_max(M - 1).to(dev))
            if mut == "clamped_row_counted":
                dWs[M - 1] = dWs[M - 1] * (1 + npad)
            dW.index_put_((idx.reshape(-1),), dWs.reshape(-1), accumulate=True)
            if s.store:
                if order == "seq":
                    gv = torch.zeros(s.nchan, len(ps), NP, dtype=D, device=dev)
                    for m in range(M):
                        gv += Ws[m][:, None, None] * Z[m][None]
                elif order == "permuted":
                    gv = torch.einsum("mc,mpn->cpn", Ws[pm], Z[pm])
                else:
                    gv = torch.einsum("mc,mpn->cpn", Ws, Z)
                pv, mk = prev[:, qs], mask[:, qs]
                if absval:
                    pv = pv.abs()
                if s.accum and mut == "accum_after_mask":
                    gv = (torch.where(mk, gv, zero) if s.mask else gv) + pv
                else:
                    if s.accum:
                        gv = gv + pv
                    if s.mask:
                        gv = torch.where(mk, gv, zero)
                gs[:, qs] = gv
                if s.stats:
                    xs = true["g%d" % i][:, qs] if absval else gv
                    if mut != "pad_frames_counted":
                        xs = torch.where(live, xs, zero)
                    if mut == "last_tile_dropped":
                        xs = torch.where((torch.arange(NP, device=dev) >= (N - 1) // TILE * TILE)[None, None, :], zero, xs)
                    mean = torch.zeros_like(s.mean) if mut == "no_mean" else s.mean
                    cen = x[:, qs] - col(mean, D)
                    if D == torch.float32:
                        # the kernel's recovery of x - mean from the staged activation (fp32 fmas), where it uses it
                        k0, k1 = (s.c0, s.c1) if s.bn else (torch.ones_like(s.c0), torch.zeros_like(s.c1))
                        slow = slow_stat_channel(k0, k1)
                        ic0 = torch.where(slow, torch.zeros_like(k0), 1.0 / k0)
                        kz1 = (k1.double() * ic0.double() + mean.double()).float()
                        rec = (act[:, qs].double() * col(ic0) - col(kz1)).float()
                        cen = torch.where(slow[:, None, None], cen, rec)
                    if absval:
                        xs, cen = xs.abs(), cen.abs()
                    out["st0_%d" % i], out["st1_%d" % i] = fsum(xs), fsum(xs * cen)
        elif s.store and s.stats:
            out["st0_%d" % i] = out["st1_%d" % i] = torch.zeros(s.nchan, dtype=D, device=dev)
        if s.store:
            out["g%d" % i] = gs
    out["dW"] = dW
    return out


def split3(x):
    """x3_common.hpp's ctx_split2 on an fp32 tensor: (hi, mid, lo), each a bf16 value rounded to nearest, the residues
    taken in fp32"""
    bf = lambda t: t.to(torch.bfloat16).float()
    hi = bf(x)
    r = x - hi
    mid = bf(r)
    lo = bf(r - mid)
    return hi, mid, lo
