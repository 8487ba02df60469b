"""The bf16-octet recurrence kernels of bf16_gru.hip through the C ABI against tests/bgru_ref.py: inputs (the regimes and
seeding of tests/gru_cases.py, gi and dhout rounded to bf16 once), launch helpers with guarded outputs, and the case
functions tests/test_bgru_gpu.py calls in process.  tests/test_bgru_ref_cpu.py passes the CPU stand-ins of bgru_ref through
the same case functions in the kernels' place.

As a program (``python tests/bgru_cases.py OUT.json``) it runs gru_cases.CHILD_CASES and writes the figures plus a checksum
of every output tensor as JSON: bgru_ne() in bf16_gru.hip latches TRUNET_GRU_NE at its first call, so the kernel instances
the default does not pick (bgru_fwd_kernel<1>, bgru_bwd_kernel<2>) can only be reached from a fresh interpreter."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bgru_ref as B  # noqa: E402
import gru_cases as G  # noqa: E402

H = B.H
CASES = G.FGRU_CASES
CHILD_CASES = G.CHILD_CASES
PARITY = "parity_bgru.txt"


def inputs(regime, L, NP):
    """gru_cases.fgru_inputs with gi and dhout rounded to bf16 once: the kernel and both references see the same numbers;
    W_hh and b_hh stay fp32"""
    c = G.fgru_inputs(regime, L, NP)
    c.gi, c.dhout = B.rne(c.gi), B.rne(c.dhout)
    return c


def case(regime, L, NP):
    return B.fwd_refs(inputs(regime, L, NP))


# ---------------------------------------------------------------------------------------------- launches
def _guarded(octets, L, NP):
    """a NaN-filled bf16 output of `octets` octet planes with one more octet behind it"""
    flat = torch.full(((octets * L * NP + 1) * 8,), float("nan"), device="cuda", dtype=torch.bfloat16)
    return flat, flat[:octets * L * NP * 8].view(octets, L, NP, 8)


def _launched(what, flat, ins):
    """after the launch: the guard octet is still NaN, every input holds the bits it held"""
    torch.cuda.synchronize()
    for f in flat:
        assert bool(torch.isnan(f[-8:]).all()), "%s: the octet behind an output was written" % what
    for name, dev, host in ins:
        assert torch.equal(dev.cpu().view(-1).view(torch.uint8), host.contiguous().view(-1).view(torch.uint8)), \
            "%s: input %s changed" % (what, name)


def gpu_bgru_fwd(gi, whh, bhh, want_gates=True):
    """trunet_bf16_gru_fwd on CPU fp32 tensors in gru_ref's shapes (gi holds bf16 values or NaN).  Returns (hout, gates or
    None) as fp32 on the CPU."""
    from tinyrecurrentunet_amd import _lib as Lb
    L, NP = gi.shape[1:]
    gi16 = B.pack("gi", gi)
    ins = [("gi", gi16.cuda(), gi16), ("whh", whh.cuda().contiguous(), whh), ("bhh", bhh.cuda().contiguous(), bhh)]
    (_, gid, _), (_, wd, _), (_, bd, _) = ins
    hflat, hout = _guarded(B.OCTETS["hout"], L, NP)
    gflat, gates = _guarded(B.OCTETS["gates"], L, NP) if want_gates else (None, None)
    Lb.check(Lb.lib().trunet_bf16_gru_fwd(Lb.ptr16(gid), Lb.ptr(wd[0]), Lb.ptr(bd[0]), Lb.ptr(wd[1]), Lb.ptr(bd[1]),
                                          Lb.ptr16(hout), Lb.ptr16(gates), H, L, NP, Lb.stream()), "bf16_gru_fwd")
    _launched("bf16_gru_fwd", [hflat] + ([gflat] if want_gates else []), ins)
    return B.unpack("hout", hout.cpu()), (B.unpack("gates", gates.cpu()) if want_gates else None)


def gpu_bgru_bwd(dhout, state, whh):
    """trunet_bf16_gru_bwd; state = (hout, gates) as stored (bf16 values).  Returns (dgi, dghn) as fp32 on the CPU."""
    from tinyrecurrentunet_amd import _lib as Lb
    L, NP = dhout.shape[1:]
    host = [("dhout", B.pack("dhout", dhout)), ("hout", B.pack("hout", state[0])), ("gates", B.pack("gates", state[1])),
            ("whh", whh)]
    ins = [(n, t.cuda().contiguous(), t) for n, t in host]
    dd, hd, gd, wd = (t for _, t, _ in ins)
    iflat, dgi = _guarded(B.OCTETS["dgi"], L, NP)
    nflat, dghn = _guarded(B.OCTETS["dghn"], L, NP)
    Lb.check(Lb.lib().trunet_bf16_gru_bwd(Lb.ptr16(dd), Lb.ptr16(hd), Lb.ptr16(gd), Lb.ptr(wd[0]), Lb.ptr(wd[1]),
                                          Lb.ptr16(dgi), Lb.ptr16(dghn), H, L, NP, Lb.stream()), "bf16_gru_bwd")
    _launched("bf16_gru_bwd", [iflat, nflat], ins)
    return B.unpack("dgi", dgi.cpu()), B.unpack("dghn", dghn.cpu())


# ---------------------------------------------------------------------------------------------- comparison and report
def report(line):
    ne = os.environ.get("TRUNET_GRU_NE")
    if ne:
        line = "[TRUNET_GRU_NE=%s] %s" % (ne, line)
    from convt_cases import report as write
    write(line, PARITY)


def compare(tag, items):
    """items: (name, got, ref64, ref32).  Every figure is printed BEFORE the first assertion fires; returns
    {name: (err, B, pinned share)} -- reported, not asserted; what is asserted is bgru_ref.inside."""
    res, fails = {}, []
    for name, got, r64, r32 in items:
        try:
            res[name] = B.inside(got, r64, r32, "%s %s" % (tag, name))
        except AssertionError as e:
            lo, hi, bnd, _ = B.interval(r64, r32)
            res[name] = (float((got.double() - r64).abs().max()), bnd, float((lo == hi).double().mean()))
            fails.append(str(e))
    report("%s: kernel error / B / pinned share  " % tag
           + "  ".join("%s %.2e/%.2e/%.1f%%" % (n, res[n][0], res[n][1], 100 * res[n][2]) for n in res))
    assert not fails, "\n".join(fails)
    return res


def tag(c, what):
    return "BGRU %s %s L=%d NP=%d" % (what, c.regime, c.L, c.NP)


def check_fwd(c, fwd=gpu_bgru_fwd):
    """hout and the four gate planes inside their intervals; gates = NULL gives the same hout bit for bit"""
    hout, gates = fwd(c.gi, c.whh, c.bhh)
    res = compare(tag(c, "fwd"), B.fwd_items((hout, gates), c))
    if fwd is gpu_bgru_fwd:
        hout_e, _ = fwd(c.gi, c.whh, c.bhh, want_gates=False)
        assert torch.equal(hout_e, hout), "gates = NULL changes hout"
    return res, {"hout": hout, "gates": gates}


def check_bwd(c, own, fwd_out=None, dhout=None, fwd=gpu_bgru_fwd, bwd=gpu_bgru_bwd, what=None):
    """own = False: the backward kernel on the fp64 forward's state rounded to bf16 (the kernel alone); own = True: on the
    forward kernel's own stored outputs, the references recomputed on them (the pair as the engine runs it)"""
    state = (fwd_out or fwd(c.gi, c.whh, c.bhh)) if own else c.state
    dhout = c.dhout if dhout is None else dhout
    r64, r32 = B.bwd_refs(dhout, state, c.whh)
    out = bwd(dhout, state, c.whh)
    res = compare(tag(c, what or ("bwd(own fwd)" if own else "bwd(ref state)")), B.bwd_items(out, r64, r32))
    return res, {"dgi": out[0], "dghn": out[1]}, r64


def run_cases(cases=CHILD_CASES, fwd=gpu_bgru_fwd, bwd=gpu_bgru_bwd):
    """forward, backward on the reference state and backward on the forward's own outputs of every case; returns
    {"figures": {case: {tensor: [err, B, pinned]}}, "sums": {case: {tensor: sha1}}} (raises where an interval is missed)"""
    out = {"figures": {}, "sums": {}}
    for regime, L, NP in cases:
        c = case(regime, L, NP)
        fig, sums = {}, {}
        r, o = check_fwd(c, fwd)
        fig.update(r), sums.update({k: G.checksum(v) for k, v in o.items()})
        for own, pre in ((False, "iso."), (True, "own.")):
            r, o2, _ = check_bwd(c, own, fwd_out=(o["hout"], o["gates"]), fwd=fwd, bwd=bwd)
            fig.update({pre + k: v for k, v in r.items()}), sums.update({pre + k: G.checksum(v) for k, v in o2.items()})
        key = "%s,%d,%d" % (regime, L, NP)
        out["figures"][key], out["sums"][key] = {k: list(v) for k, v in fig.items()}, sums
    return out


if __name__ == "__main__":
    result = run_cases()
    result["TRUNET_GRU_NE"] = os.environ.get("TRUNET_GRU_NE")
    text = json.dumps(result)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)
    else:
        print(text)
