"""What the bf16-octet recurrence kernels of bf16_gru.hip (trunet_bf16_gru_fwd / _bwd) are held to, on CPU tensors.

The recurrence is tests/gru_ref.py's (fgru_fwd / fgru_bwd) and is not restated here.  The kernels do its arithmetic in fp32
and never round inside it; only what they STORE is bf16, rounded to nearest even.  So every stored value is rne_bf16(y) of
some fp32 y that the fp32 pin's own bound admits: |y - ref64| <= B = gru_ref.bound(ref64, ref32), ref32 being the fp32
restatement on the same inputs.  Rounding is monotonic, hence the comparison is an interval with no tolerance of its own,

    rne_bf16(ref64 - B) <= stored <= rne_bf16(ref64 + B),

the endpoints taken to fp32 and moved outward by one fp32 ulp first (that absorbs the double rounding fp64 -> fp32 -> bf16).
Where both ends round to the same bf16 value the test pins the exact bits.  B never comes from a kernel's output.

Layout: an fp32 tensor [C][L][NP] is stored as bf16 octets [C/8][L][NP][8].  With gru_ref's row orders every tensor of the
kernels is that one map of its flattened channel axis:
    gi, dgi       [6H] -> 48 octets: direction d at octet 24 d, gate g at + 8 g
    hout, dhout, dghn [2H] -> 16 octets: direction d at octet 8 d
    gates         [2][4][H] -> 64 octets [dir][r, z, n, gh][H/8]"""
import torch

import gru_ref as R

H = 64
OCTETS = {"gi": 48, "dgi": 48, "hout": 16, "dhout": 16, "dghn": 16, "gates": 64}
GATE_NAMES = ("r", "z", "n", "ghn")


# ---------------------------------------------------------------------------------------------- rounding and octets
def rne(t):
    """fp32 / fp64 -> the nearest bf16 value (ties to even), as fp32"""
    return t.float().bfloat16().float()


def trunc(t):
    """fp32 -> bf16 by dropping the low 16 bits (what the kernels must NOT do), as fp32"""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def representable(t):
    return torch.equal(rne(t), t.float())


def to_octets(t):
    """fp32 [C][L][NP] (C % 8 == 0, bf16-representable or to be rounded RNE) -> bf16 [C/8][L][NP][8]: element (c, l, n) at
    (((c / 8) L + l) NP + n) 8 + c % 8"""
    C, L, NP = t.shape
    return t.reshape(C // 8, 8, L, NP).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)


def from_octets(o):
    """bf16 [C/8][L][NP][8] -> fp32 [C][L][NP]"""
    n, L, NP, _ = o.shape
    return o.permute(0, 3, 1, 2).reshape(n * 8, L, NP).float().contiguous()


def pack(name, t):
    """a tensor in gru_ref's shape ([6H] / [2H] / [2][4][H] leading, then [L][NP]) -> the kernels' octet tensor"""
    L, NP = t.shape[-2:]
    o = to_octets(t.reshape(-1, L, NP))
    assert o.shape[0] == OCTETS[name], (name, o.shape)
    return o


def unpack(name, o):
    assert o.shape[0] == OCTETS[name], (name, o.shape)
    t = from_octets(o)
    return t.reshape(2, 4, H, *t.shape[1:]) if name == "gates" else t


# ---------------------------------------------------------------------------------------------- the interval
def interval(ref64, ref32):
    """(lo, hi, B, e32): the closed interval of bf16 values (as fp32) a stored element may take"""
    assert ref64.dtype == torch.float64 and ref64.shape == ref32.shape
    assert bool(torch.isfinite(ref64).all()) and bool(torch.isfinite(ref32).all()), "reference not finite"
    e32, B = R.bound(ref64, ref32)[:2]
    inf = torch.full(ref64.shape, float("inf"))
    lo = torch.nextafter((ref64 - B).float(), -inf)
    hi = torch.nextafter((ref64 + B).float(), inf)
    return rne(lo), rne(hi), B, e32


def outside(got, lo, hi):
    """share of the elements that are not finite or not in [lo, hi] (-0 and +0 compare equal)"""
    got = got.float()
    return float((~(torch.isfinite(got) & (got >= lo) & (got <= hi))).double().mean())


def inside(got, ref64, ref32, what):
    """The one comparison of the bf16 recurrence tests; every element counts.  Returns the three figures that are reported
    and not asserted: (max|got - fp64|, B, share of elements whose interval is a single bf16 value)."""
    got = got.detach().cpu().float()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    assert representable(got), "%s: not bf16 values" % what
    lo, hi, B, _ = interval(ref64, ref32)
    assert bool(torch.isfinite(got).all()), "%s: not finite" % what
    bad = ~((got >= lo) & (got <= hi))
    n = int(bad.sum())
    if n:
        i = int((torch.where(got < lo, lo - got, got - hi) * bad).flatten().argmax())
        raise AssertionError("%s: %d of %d elements outside the interval (B %.3e); worst: got %.9g, interval [%.9g, %.9g], "
                             "fp64 %.12g" % (what, n, got.numel(), B, got.flatten()[i], lo.flatten()[i], hi.flatten()[i],
                                             ref64.flatten()[i]))
    return float((got.double() - ref64).abs().max()), B, float((lo == hi).double().mean())


# ---------------------------------------------------------------------------------------------- references of a case
def fwd_refs(c):
    """c.gi (bf16-representable), c.whh, c.bhh (fp32) -> c.f64, c.f32 = (hout, gates) of the restatement, and c.state: the
    fp64 forward rounded to bf16 -- exactly what the backward kernel reads when it is tested alone"""
    assert representable(c.gi) and representable(c.dhout)
    c.f64 = R.fgru_fwd(c.gi, c.whh, c.bhh, torch.float64)
    c.f32 = R.fgru_fwd(c.gi, c.whh, c.bhh, torch.float32)
    c.state = tuple(rne(t) for t in c.f64)
    return c


def bwd_refs(dhout, state, whh):
    """(fp64, fp32) backward of the restatement on a stored (bf16-representable) state"""
    assert all(representable(t) for t in (dhout,) + tuple(state))
    return R.fgru_bwd(dhout, *state, whh, torch.float64), R.fgru_bwd(dhout, *state, whh, torch.float32)


def fwd_items(out, c):
    """out = (hout, gates) of a candidate -> (name, got, ref64, ref32) of hout and the four gate planes"""
    items = [("hout", out[0], c.f64[0], c.f32[0])]
    return items + [(n, out[1][:, k], c.f64[1][:, k], c.f32[1][:, k]) for k, n in enumerate(GATE_NAMES)]


def bwd_items(out, r64, r32):
    return [("dgi", out[0], r64[0], r32[0]), ("dghn", out[1], r64[1], r32[1])]


# ---------------------------------------------------------------------------------------------- stand-ins for the kernels
def swap_frames(t):
    """frames 2 c + e <-> c + 32 e inside every block of 64 (gru.hip's and bf16_gru.hip's column maps of a two-block
    workgroup): the value of frame 2 c + e lands at frame c + 32 e"""
    NP = t.shape[-1]
    n = torch.arange(NP)
    j = n % 64
    return t.index_select(-1, n - j + 2 * (j % 32) + j // 32)


def standin_fwd(gi, whh, bhh, mut=None, rnd=rne):
    """The fp32 restatement, stored through `rnd`, in the forward kernel's place; `mut` names ONE deliberate error (a
    mutant of gru_ref, or of the octet plumbing)"""
    if mut == "dir1_octet0":                   # direction 1 of gi read from octet 0 instead of octet 24
        gi = torch.cat((gi[:3 * H], gi[:3 * H]))
    hout, gates = R.fgru_fwd(gi, whh, bhh, torch.float32, mut if mut in R.MUTANTS + R.BF16_MUTANTS else None)
    if mut == "swap_n_gh":                     # the n and gh planes stored in each other's place
        gates = gates[:, [0, 1, 3, 2]]
    if mut == "swap_frames":
        hout, gates = swap_frames(hout), swap_frames(gates)
    return rnd(hout), rnd(gates)


def standin_bwd(dhout, state, whh, mut=None, rnd=rne):
    hout, gates = state
    if mut == "swap_n_gh":                     # ... and read from each other's place
        gates = gates[:, [0, 1, 3, 2]]
    dgi, dghn = R.fgru_bwd(dhout, hout, gates, whh, torch.float32, mut if mut in R.MUTANTS + R.BF16_MUTANTS else None)
    if mut == "swap_frames":
        dgi, dghn = swap_frames(dgi), swap_frames(dghn)
    return rnd(dgi), rnd(dghn)
