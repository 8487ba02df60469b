"""The FGRU / TGRU recurrence kernels through the C ABI against tests/gru_ref.py: input regimes, launch helpers and the
case functions tests/test_gru_gpu.py calls in process.

As a program (``python tests/gru_cases.py OUT.json``) it runs CHILD_CASES of the FGRU kernels and writes the errors plus a
checksum of every output tensor as JSON: gru_ne() in gru.hip latches TRUNET_GRU_NE at its first call, so the kernel
instances the default does not pick (gru_fwd_kernel<1>, gru_bwd_kernel<2>) can only be reached from a fresh interpreter."""
import hashlib
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gru_ref as R  # noqa: E402

# regime -> (W_hh scale, gi scale); draws are N(0,1) times the scale from a seeded CPU generator, b_hh is 0.1 N(0,1)
REGIMES = {
    "ordinary": (0.15, 1.0),         # the regime of the block tests; the tightest bound
    "trained": (0.6, 3.0),           # large recurrent gain, |gh_n| up to ~16
    "saturated": (1.0, 30.0),        # two thirds of z within 1e-6 of 0 or 1: z (1 - z) and 1 - n^2 vanish
    "overflow": (0.15, 200.0),       # exp overflows to inf in both signs; everything must stay finite
    "long": (0.3, 2.0),              # meant for L = 33 / T = 41
    "no_recurrence": (0.0, 1.0),     # pure gate math: the unit-to-row map with nothing to hide it
}
GATE_NAMES = ("r", "z", "n", "ghn")
FH, TH = 64, 128

FGRU_SHAPES = [(L, NP) for L in (1, 2, 16, 17, 33) for NP in (128, 384, 512)]
FGRU_CASES = ([("ordinary", L, NP) for L, NP in FGRU_SHAPES] + [(r, 16, 384) for r in REGIMES if r != "ordinary"]
              + [("long", 33, 384), ("overflow", 5, 384)])
TGRU_SHAPES = [(T, SP, S) for T in (1, 2, 9, 41) for SP, S in ((32, 32), (32, 5), (96, 70), (64, 33))]
TGRU_CASES = ([("ordinary", T, SP, S) for T, SP, S in TGRU_SHAPES] + [(r, 9, 96, 70) for r in REGIMES if r != "ordinary"]
              + [("long", 41, 96, 70)])
# what the child interpreters (one per TRUNET_GRU_NE value) run: every regime, L = 1, odd L, one and several workgroups
CHILD_CASES = [(r, 16, 384) for r in REGIMES] + [("ordinary", 1, 128), ("ordinary", 17, 512), ("long", 33, 128)]


def _gen(*key):
    return torch.Generator().manual_seed(int(hashlib.sha1(repr(key).encode()).hexdigest()[:8], 16))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def fgru_inputs(regime, L, NP, H=FH):
    ws, gs = REGIMES[regime]
    g = _gen("fgru", regime, L, NP)
    return types.SimpleNamespace(regime=regime, L=L, NP=NP, H=H, whh=_randn(g, 2, 3 * H, H) * ws,    # per direction
                                 bhh=_randn(g, 2, 3 * H) * 0.1, gi=_randn(g, 6 * H, L, NP) * gs,
                                 dhout=_randn(g, 2 * H, L, NP))


def tgru_inputs(regime, T, SP, S, H=TH):
    ws, gs = REGIMES[regime]
    g = _gen("tgru", regime, T, SP, S)
    c = types.SimpleNamespace(regime=regime, T=T, SP=SP, S=S, H=H, whh=_randn(g, 3 * H, H) * ws, bhn=_randn(g, H) * 0.1,
                              gi=_randn(g, 3 * H, T, SP) * gs, dhs=_randn(g, H, T + 1, SP))
    c.dhs_nan = c.dhs.clone()
    c.dhs_nan[:, :, S:] = float("nan")         # padded sequences carry no gradient, whatever the buffer holds there
    c.dhs[:, :, S:] = 0.0
    return c


def fgru_refs(c):
    """fp64 reference and fp32 restatement of forward, backward on that forward (`pair`), and backward on the fp64 state
    rounded to fp32 (`iso`: what isolates the backward kernel) -- computed once per case"""
    c.f64 = R.fgru_fwd(c.gi, c.whh, c.bhh, torch.float64)
    c.f32 = R.fgru_fwd(c.gi, c.whh, c.bhh, torch.float32)
    c.state = tuple(t.float() for t in c.f64)
    c.pair64 = R.fgru_bwd(c.dhout, *c.f64, c.whh, torch.float64)
    c.pair32 = R.fgru_bwd(c.dhout, *c.f32, c.whh, torch.float32)
    c.iso64 = R.fgru_bwd(c.dhout, *c.state, c.whh, torch.float64)
    c.iso32 = R.fgru_bwd(c.dhout, *c.state, c.whh, torch.float32)
    return c


def tgru_refs(c):
    c.f64 = R.tgru_fwd(c.gi, c.whh, c.bhn, torch.float64)
    c.f32 = R.tgru_fwd(c.gi, c.whh, c.bhn, torch.float32)
    c.state = tuple(t.float() for t in c.f64)
    c.pair64 = R.tgru_bwd(c.dhs_nan, *c.f64, c.whh, c.S, torch.float64)
    c.pair32 = R.tgru_bwd(c.dhs_nan, *c.f32, c.whh, c.S, torch.float32)
    c.iso64 = R.tgru_bwd(c.dhs_nan, *c.state, c.whh, c.S, torch.float64)
    c.iso32 = R.tgru_bwd(c.dhs_nan, *c.state, c.whh, c.S, torch.float32)
    return c


# ---------------------------------------------------------------------------------------------- launches
def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.float32)


def gpu_fgru_fwd(gi, whh, bhh, want_gates=True):
    """trunet_gru_fwd on CPU tensors; outputs are prefilled with NaN.  Returns (hout, gates or None) on the CPU."""
    from tinyrecurrentunet_amd import _lib as Lb
    H, (L, NP) = whh.shape[2], gi.shape[1:]
    gi, whh, bhh = gi.cuda().contiguous(), whh.cuda().contiguous(), bhh.cuda().contiguous()
    hout = _nan(2 * H, L, NP)
    gates = _nan(2, 4, H, L, NP) if want_gates else None
    Lb.check(Lb.lib().trunet_gru_fwd(Lb.ptr(gi), Lb.ptr(whh[0]), Lb.ptr(bhh[0]), Lb.ptr(whh[1]), Lb.ptr(bhh[1]), Lb.ptr(hout),
                                     Lb.ptr(gates), H, L, NP, Lb.stream()), "gru_fwd")
    torch.cuda.synchronize()
    return hout.cpu(), (gates.cpu() if want_gates else None)


def gpu_fgru_bwd(dhout, hout, gates, whh):
    from tinyrecurrentunet_amd import _lib as Lb
    H, (L, NP) = whh.shape[2], dhout.shape[1:]
    dhout, hout, gates, whh = (t.float().cuda().contiguous() for t in (dhout, hout, gates, whh))
    dgi, dghn = _nan(6 * H, L, NP), _nan(2 * H, L, NP)
    Lb.check(Lb.lib().trunet_gru_bwd(Lb.ptr(dhout), Lb.ptr(hout), Lb.ptr(gates), Lb.ptr(whh[0]), Lb.ptr(whh[1]), Lb.ptr(dgi),
                                     Lb.ptr(dghn), H, L, NP, NP, Lb.stream()), "gru_bwd")
    torch.cuda.synchronize()
    return dgi.cpu(), dghn.cpu()


def gpu_tgru_fwd(gi, whh, bhn, want_gates=True):
    """trunet_tgru_rec_fwd; hs is prefilled with NaN except column 0 = h_{-1} = 0, which the kernel must leave alone"""
    from tinyrecurrentunet_amd import _lib as Lb
    H, (T, SP) = whh.shape[1], gi.shape[1:]
    gi, whh, bhn = gi.cuda().contiguous(), whh.cuda().contiguous(), bhn.cuda().contiguous()
    hs = _nan(H, T + 1, SP)
    hs[:, 0] = 0.0
    gates = _nan(4, H, T, SP) if want_gates else None
    Lb.check(Lb.lib().trunet_tgru_rec_fwd(Lb.ptr(gi), Lb.ptr(whh), Lb.ptr(bhn), Lb.ptr(hs), Lb.ptr(gates), H, T, SP,
                                          Lb.stream()), "tgru_rec_fwd")
    torch.cuda.synchronize()
    return hs.cpu(), (gates.cpu() if want_gates else None)


def gpu_tgru_bwd(dhs, hs, gates, whh, S):
    from tinyrecurrentunet_amd import _lib as Lb
    H, (T, SP) = whh.shape[1], gates.shape[2:]
    dhs, hs, gates, whh = (t.float().cuda().contiguous() for t in (dhs, hs, gates, whh))
    dgi, dgh = _nan(3 * H, T, SP), _nan(3 * H, T, SP)
    Lb.check(Lb.lib().trunet_tgru_rec_bwd(Lb.ptr(dhs), Lb.ptr(hs), Lb.ptr(gates), Lb.ptr(whh), Lb.ptr(dgi), Lb.ptr(dgh), H, T,
                                          SP, S, Lb.stream()), "tgru_rec_bwd")
    torch.cuda.synchronize()
    return dgi.cpu(), dgh.cpu()


# ---------------------------------------------------------------------------------------------- comparison and report
def report(line):
    """one line per case: printed, and appended to parity_gru.txt in the directory TRUNET_PARITY_DIR names (relative to
    the repository root), where that is set and the directory exists"""
    ne = os.environ.get("TRUNET_GRU_NE")
    if ne:
        line = "[TRUNET_GRU_NE=%s] %s" % (ne, line)
    from convt_cases import report as write
    write(line, "parity_gru.txt")


def compare(tag, items):
    """items: (name, got, ref64, ref32).  Every figure is printed BEFORE the first assertion fires; returns
    {name: (err, e32, bound)}."""
    res, fails = {}, []
    for name, got, r64, r32 in items:
        try:
            err, e32, bound = R.close(got, r64, r32, "%s %s" % (tag, name))[:3]
            res[name] = (err, e32, bound)
        except AssertionError as e:
            d32 = float((r32.double() - r64).abs().max())
            err = float((got.double() - r64).abs().max())
            res[name] = (err, d32, 4 * d32 + 2e-6 * float(r64.abs().max()))
            fails.append(str(e))
    report("%s: kernel error / e32 / bound  " % tag + "  ".join("%s %.2e/%.2e/%.2e" % ((n,) + res[n]) for n in res))
    assert not fails, "\n".join(fails)
    return res


def _planes(gates, axis):
    return [(GATE_NAMES[k], gates.select(axis, k)) for k in range(4)]


def checksum(t):
    return hashlib.sha1(t.contiguous().numpy().tobytes()).hexdigest()


def fgru_tag(c, what):
    return "FGRU %s %s L=%d NP=%d" % (what, c.regime, c.L, c.NP)


def check_fgru_fwd(c):
    """hout and the four gate planes against fp64; gates = NULL gives the same hout bit for bit"""
    hout, gates = gpu_fgru_fwd(c.gi, c.whh, c.bhh)
    items = [("hout", hout, c.f64[0], c.f32[0])]
    items += [(n, p, c.f64[1][:, k], c.f32[1][:, k]) for k, (n, p) in enumerate(_planes(gates, 1))]
    res = compare(fgru_tag(c, "fwd"), items)
    hout_e, _ = gpu_fgru_fwd(c.gi, c.whh, c.bhh, want_gates=False)
    assert torch.equal(hout_e, hout), "gates = NULL changes hout"
    return res, {"hout": hout, "gates": gates}


def check_fgru_bwd(c, own, fwd_out=None):
    """own = False: backward on the fp64 forward state rounded to fp32 (the kernel alone); own = True: on the forward
    kernel's own outputs (the pair as the engine runs it)"""
    if own:
        st = fwd_out or gpu_fgru_fwd(c.gi, c.whh, c.bhh)
        r64, r32 = c.pair64, c.pair32
    else:
        st, r64, r32 = c.state, c.iso64, c.iso32
    dgi, dghn = gpu_fgru_bwd(c.dhout, st[0], st[1], c.whh)
    res = compare(fgru_tag(c, "bwd(own fwd)" if own else "bwd(ref state)"),
                  [("dgi", dgi, r64[0], r32[0]), ("dghn", dghn, r64[1], r32[1])])
    return res, {"dgi": dgi, "dghn": dghn}


def tgru_tag(c, what):
    return "TGRU %s %s T=%d SP=%d S=%d" % (what, c.regime, c.T, c.SP, c.S)


def check_tgru_fwd(c):
    hs, gates = gpu_tgru_fwd(c.gi, c.whh, c.bhn)
    assert bool((hs[:, 0] == 0).all()), "hs[:, 0] (h_{-1}) was written"
    items = [("hs", hs, c.f64[0], c.f32[0])]
    items += [(n, p, c.f64[1][k], c.f32[1][k]) for k, (n, p) in enumerate(_planes(gates, 0))]
    res = compare(tgru_tag(c, "fwd"), items)
    hs_e, _ = gpu_tgru_fwd(c.gi, c.whh, c.bhn, want_gates=False)
    assert torch.equal(hs_e, hs), "gates = NULL changes hs"
    return res, {"hs": hs, "gates": gates}


def check_tgru_bwd(c, own, fwd_out=None):
    """dhs holds NaN at the columns >= S: the live columns must come out bit for bit as with zeros there, the dead ones
    exactly zero"""
    if own:
        st = fwd_out or gpu_tgru_fwd(c.gi, c.whh, c.bhn)
        r64, r32 = c.pair64, c.pair32
    else:
        st, r64, r32 = c.state, c.iso64, c.iso32
    dgi, dgh = gpu_tgru_bwd(c.dhs_nan, st[0], st[1], c.whh, c.S)
    res = compare(tgru_tag(c, "bwd(own fwd)" if own else "bwd(ref state)"),
                  [("dgi_all", dgi, r64[0], r32[0]), ("dgh_all", dgh, r64[1], r32[1])])
    dgi0, dgh0 = gpu_tgru_bwd(c.dhs, st[0], st[1], c.whh, c.S)
    assert torch.equal(dgi0, dgi) and torch.equal(dgh0, dgh), "NaN in dhs at columns >= S reaches the outputs"
    assert bool((dgi[:, :, c.S:] == 0).all()) and bool((dgh[:, :, c.S:] == 0).all()), "dead columns are not exactly zero"
    return res, {"dgi_all": dgi, "dgh_all": dgh}


def run_fgru_cases(cases=CHILD_CASES):
    """forward, backward on the reference state and backward on the forward's own outputs of every case; returns
    {"errors": {case: {tensor: [err, e32, bound]}}, "sums": {case: {tensor: sha1}}} (raises where a bound is missed)"""
    out = {"errors": {}, "sums": {}}
    for regime, L, NP in cases:
        c = fgru_refs(fgru_inputs(regime, L, NP))
        key = "%s,%d,%d" % (regime, L, NP)
        err, sums = {}, {}
        r, o = check_fgru_fwd(c)
        err.update(r), sums.update({k: checksum(v) for k, v in o.items()})
        r, o2 = check_fgru_bwd(c, own=False)
        err.update({"iso." + k: v for k, v in r.items()}), sums.update({"iso." + k: checksum(v) for k, v in o2.items()})
        r, o2 = check_fgru_bwd(c, own=True, fwd_out=(o["hout"], o["gates"]))
        err.update({"own." + k: v for k, v in r.items()}), sums.update({"own." + k: checksum(v) for k, v in o2.items()})
        out["errors"][key], out["sums"][key] = {k: list(v) for k, v in err.items()}, sums
    return out


if __name__ == "__main__":
    result = run_fgru_cases()
    result["TRUNET_GRU_NE"] = os.environ.get("TRUNET_GRU_NE")
    text = json.dumps(result)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)
    else:
        print(text)
