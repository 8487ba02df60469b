"""Plain torch restatement of what the recurrence kernels of gru.hip and the GRU cells of elementwise.hip compute, in the
kernels' own layouts (rows = units, last axis = frames / sequences).  dtype = float64 is the reference; float32 (torch's
exp and tanh on the CPU) is the yardstick `close` measures the tolerance with.

torch gate order (r, z, n):  r = s(gi_r + W_hr h + b_hr), z = s(gi_z + W_hz h + b_hz), n = tanh(gi_n + r (W_hn h + b_hn)),
h' = (1 - z) n + z h.  Backward per step: dh = dh_out + carry; dn = dh (1 - z); dnp = dn (1 - n^2);
dzp = dh (h_prev - n) z (1 - z); drp = dnp gh_n r (1 - r); dgi = (drp, dzp, dnp); dgh = (drp, dzp, dnp r);
carry = dh z + W_hh^T dgh.

`mut` names ONE deliberate error (tests/test_gru_ref_cpu.py passes such mutants through `close` in place of kernel output to
show that the comparison would catch a subtly wrong kernel); None everywhere else."""
import torch

MUTANTS = ("bhn_outside", "dzp_ht", "rev_forwards", "no_carry", "dghn_dnp", "swap_u4", "k_half", "hs_off")
# FGRU only, for the bf16-octet kernels of bf16_gru.hip (tests/bgru_ref.py): a bf16 rounding INSIDE the recurrence, where
# those kernels keep fp32 -- h rounded before it is carried into the next step, dgh rounded in front of the carry product
BF16_MUTANTS = ("h_rounded", "dgh_rounded")


def _swap_u4(t, axis):
    """rows u <-> u + 4 inside every group of 8 along `axis` (a unit axis, or several stacked): in the MFMA C layout a
    lane's accumulator registers hold units u .. u+3 and the other half-wave's lane the units four rows further"""
    return t.index_select(axis, torch.arange(t.shape[axis]) ^ 4)


def fgru_fwd(gi, whh, bhh, dtype=torch.float64, mut=None):
    """gi [6H][L][NP] (direction d, gate g, unit u at row d*3H + g*H + u), whh [2][3H][H], bhh [2][3H] ->
    hout [2H][L][NP], gates [2][4][H][L][NP] (r, z, n, W_hn h + b_hn).  Direction 1 walks positions L-1 .. 0."""
    gi, whh, bhh = gi.to(dtype), whh.to(dtype), bhh.to(dtype)
    H = whh.shape[2]
    L, NP = gi.shape[1:]
    hout = torch.zeros(2 * H, L, NP, dtype=dtype)
    gates = torch.zeros(2, 4, H, L, NP, dtype=dtype)
    for d in range(2):
        h = torch.zeros(H, NP, dtype=dtype)
        for t in range(L):
            pos = L - 1 - t if (d == 1 and mut != "rev_forwards") else t
            g = gi[d * 3 * H:(d + 1) * 3 * H, pos]
            gh = whh[d] @ h + bhh[d][:, None]
            r = torch.sigmoid(g[:H] + gh[:H])
            z = torch.sigmoid(g[H:2 * H] + gh[H:2 * H])
            ghn = gh[2 * H:]
            if mut == "bhn_outside":
                n = torch.tanh(g[2 * H:] + r * (ghn - bhh[d][2 * H:, None]) + bhh[d][2 * H:, None])
            else:
                n = torch.tanh(g[2 * H:] + r * ghn)
            h = (1 - z) * n + z * h
            hout[d * H:(d + 1) * H, pos] = h
            if mut == "h_rounded":
                h = h.bfloat16().to(dtype)
            for k, v in enumerate((r, z, n, ghn)):
                gates[d, k, :, pos] = v
    if mut == "swap_u4":
        hout, gates = _swap_u4(hout, 0), _swap_u4(gates, 2)
    return hout, gates


def fgru_bwd(dhout, hout, gates, whh, dtype=torch.float64, mut=None):
    """dhout, hout [2H][L][NP], gates [2][4][H][L][NP], whh [2][3H][H] -> dgi [6H][L][NP], dghn [2H][L][NP] (= dnp r, the
    third block of dgh; its first two are dgi's)."""
    dhout, hout, gates, whh = dhout.to(dtype), hout.to(dtype), gates.to(dtype), whh.to(dtype)
    H = whh.shape[2]
    L, NP = dhout.shape[1:]
    dgi = torch.zeros(6 * H, L, NP, dtype=dtype)
    dghn = torch.zeros(2 * H, L, NP, dtype=dtype)
    for d in range(2):
        carry = torch.zeros(H, NP, dtype=dtype)
        for t in range(L - 1, -1, -1):
            pos = L - 1 - t if d else t
            ppos = pos + 1 if d else pos - 1
            r, z, n, ghn = (gates[d, k, :, pos] for k in range(4))
            hp = hout[d * H:(d + 1) * H, ppos] if t > 0 else torch.zeros(H, NP, dtype=dtype)
            if mut == "dzp_ht":
                hp = hout[d * H:(d + 1) * H, pos]
            dh = dhout[d * H:(d + 1) * H, pos] + carry
            dnp = dh * (1 - z) * (1 - n * n)
            dzp = dh * (hp - n) * z * (1 - z)
            drp = dnp * ghn * r * (1 - r)
            dgn = dnp if mut == "dghn_dnp" else dnp * r
            dgi[d * 3 * H:(d + 1) * 3 * H, pos] = torch.cat((drp, dzp, dnp))
            dghn[d * H:(d + 1) * H, pos] = dgn
            carry = dh * z
            if mut == "dgh_rounded":
                carry = carry + whh[d].t() @ torch.cat((drp, dzp, dnp * r)).bfloat16().to(dtype)
            elif mut != "no_carry":
                carry = carry + whh[d].t() @ torch.cat((drp, dzp, dnp * r))
    if mut == "swap_u4":
        dgi, dghn = _swap_u4(dgi, 0), _swap_u4(dghn, 0)
    return dgi, dghn


def tgru_fwd(gi_all, whh, bhn, dtype=torch.float64, mut=None):
    """gi_all [3H][T][SP] (already carries b_ih + (b_hr, b_hz, 0)), whh [3H][H], bhn [H] -> hs [H][T+1][SP] with
    hs[:, 0] = 0 and h_t at position t + 1, gates [4][H][T][SP]."""
    gi_all, whh, bhn = gi_all.to(dtype), whh.to(dtype), bhn.to(dtype)
    H = whh.shape[1]
    T, SP = gi_all.shape[1:]
    hs = torch.zeros(H, T + 1, SP, dtype=dtype)
    gates = torch.zeros(4, H, T, SP, dtype=dtype)
    w = whh.clone()
    if mut == "k_half":
        w[:, H // 2:] = 0
    for t in range(T):
        g = gi_all[:, t]
        gh = w @ hs[:, t]
        r = torch.sigmoid(g[:H] + gh[:H])
        z = torch.sigmoid(g[H:2 * H] + gh[H:2 * H])
        ghn = gh[2 * H:] + bhn[:, None]
        if mut == "bhn_outside":
            n = torch.tanh(g[2 * H:] + r * gh[2 * H:] + bhn[:, None])
        else:
            n = torch.tanh(g[2 * H:] + r * ghn)
        hs[:, t + 1] = (1 - z) * n + z * hs[:, t]
        for k, v in enumerate((r, z, n, ghn)):
            gates[k, :, t] = v
    if mut == "hs_off":
        hs = torch.cat((hs[:, 1:], torch.zeros(H, 1, SP, dtype=dtype)), 1)
    if mut == "swap_u4":
        hs, gates = _swap_u4(hs, 0), _swap_u4(gates, 1)
    return hs, gates


def tgru_bwd(dhs, hs, gates, whh, S, dtype=torch.float64, mut=None):
    """dhs, hs [H][T+1][SP] (dL/dh_t at position t + 1; position 0 is not read), gates [4][H][T][SP], whh [3H][H] ->
    dgi_all rows (drp, dzp, dnp), dgh_all rows (drp, dzp, dnp r), both [3H][T][SP] and exactly zero for columns >= S
    (whatever dhs holds there)."""
    dhs, hs, gates, whh = dhs.to(dtype), hs.to(dtype), gates.to(dtype), whh.to(dtype)
    H = whh.shape[1]
    T, SP = gates.shape[2:]
    live = (torch.arange(SP) < S)[None, :]
    dgi = torch.zeros(3 * H, T, SP, dtype=dtype)
    dgh = torch.zeros(3 * H, T, SP, dtype=dtype)
    carry = torch.zeros(H, SP, dtype=dtype)
    w = whh.clone()
    if mut == "k_half":
        w[3 * H // 2:] = 0                 # the backward's K runs over the 3H gate rows
    for t in range(T - 1, -1, -1):
        r, z, n, ghn = (gates[k, :, t] for k in range(4))
        hp = hs[:, t + 1] if mut in ("dzp_ht", "hs_off") else hs[:, t]
        dh = torch.where(live, dhs[:, t + 1] + carry, torch.zeros((), dtype=dtype))
        dnp = dh * (1 - z) * (1 - n * n)
        dzp = dh * (hp - n) * z * (1 - z)
        drp = dnp * ghn * r * (1 - r)
        dnr = dnp if mut == "dghn_dnp" else dnp * r
        dgi[:, t] = torch.cat((drp, dzp, dnp))
        dgh[:, t] = torch.cat((drp, dzp, dnr))
        carry = dh * z
        if mut != "no_carry":
            carry = carry + w.t() @ torch.cat((drp, dzp, dnp * r))
    if mut == "swap_u4":
        dgi, dgh = _swap_u4(dgi, 0), _swap_u4(dgh, 0)
    return dgi, dgh


def gru_cell(gi, gh, h, dtype=torch.float64):
    """One step from full pre-activations: gi = W_ih x + b_ih, gh = W_hh h + b_hh as [3H][...], h [H][...] -> h', and the
    gate planes (r, z, n, gh_n) trunet_tgru_cell_fwd stores.  Covers trunet_gru_cell and trunet_tgru_cell_fwd."""
    gi, gh, h = gi.to(dtype), gh.to(dtype), h.to(dtype)
    H = h.shape[0]
    r = torch.sigmoid(gi[:H] + gh[:H])
    z = torch.sigmoid(gi[H:2 * H] + gh[H:2 * H])
    n = torch.tanh(gi[2 * H:] + r * gh[2 * H:])
    return (1 - z) * n + z * h, torch.stack((r, z, n, gh[2 * H:]))


def bound(ref64, ref32):
    """What `close` allows a kernel, from the references alone: e32 = max|fp32 restatement - fp64|, the bound
    4 e32 + 2e-6 max|fp64| on the maximum error, rel32 = relative L2 of the same difference, and 4 rel32 + 1e-6 on the
    relative L2.  Returns (e32, bound, rel32, rel_bound)."""
    d32 = ref32.double() - ref64
    e32, rel32 = float(d32.abs().max()), float(d32.norm()) / (float(ref64.norm()) + 1e-300)
    return e32, 4 * e32 + 2e-6 * float(ref64.abs().max()), rel32, 4 * rel32 + 1e-6


def close(got, ref64, ref32, what):
    """The one comparison of the GRU tests.  The tolerance is measured on the same inputs, against the reference and never
    against the kernel: e32 = max|fp32 restatement - fp64|, rel32 = relative L2 of the same difference.  Required:
    max|got - fp64| <= 4 e32 + 2e-6 max|fp64| (4: another summation order in the MFMA; 2e-6: hardware exp / rcp, ~1 ulp
    each over the handful of steps an error survives z h), relative L2 <= 4 rel32 + 1e-6, every value finite; no element
    is left out.  Returns (err, e32, bound, rel, rel_bound)."""
    got, ref64, ref32 = got.detach().cpu(), ref64.detach().cpu(), ref32.detach().cpu()
    assert ref64.dtype == torch.float64 and got.shape == ref64.shape == ref32.shape, (what, got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), "%s: not finite" % what
    assert bool(torch.isfinite(ref64).all()) and bool(torch.isfinite(ref32).all()), "%s: reference not finite" % what
    d = got.double() - ref64
    e32, bnd, rel32, rbound = bound(ref64, ref32)
    err, rel = float(d.abs().max()), float(d.norm()) / (float(ref64.norm()) + 1e-300)
    assert err <= bnd, "%s: max error %.3e > bound %.3e (e32 %.3e)" % (what, err, bnd, e32)
    assert rel <= rbound, "%s: relative L2 %.3e > bound %.3e (rel32 %.3e)" % (what, rel, rbound, rel32)
    return err, e32, bnd, rel, rbound
