"""GPU: the depthwise-conv kernels (csrc/depthwise.hip) held to recorded bits, through the C ABI only.

tests/golden/dwconv_bits.json holds the sha256 of every output tensor and every partials tensor of the cases below, as the
library of the commit BEFORE the seven kernels were built from one window-walk source computed them
(tests/golden/make_dwconv_bits.py).  Every later build has to give the same bits:

  * fp32 sequence: trunet_dwconv_fwd, trunet_dwconv_bwd with z = the forward output, trunet_dwconv_bwd_rz under
    TRUNET_DW_RZ=2, at the three window shapes, ragged lengths, one and two positions; channel 5 has a BatchNorm scale of
    exactly zero and channel 3 an offset beyond 2^16 times its scale (the two triggers of the rz kernel's re-read path);
  * fp32 with NP / 4 = 8256 frame quads: 64 threads take a second trip of the grid-stride loop (DW2_FB * 256 = 8192);
  * bf16 octet layout: trunet_bf16_dwconv_fwd, trunet_bf16_dwconv_bwd at the same shapes (1, 2 and 4 position chunks in
    either direction) and at NP = 33024;
  * the tap-gather fallback, (K, S) = (5, 1) and (3, 3), which trunet_dwconv_bwd_rz refuses.

Every case also checks that a second launch gives the same bits, that the outputs (pre-filled with NaN) are finite
everywhere a kernel has to write, and that a guard channel (octet) behind them is still NaN.  Inputs come from a seeded CPU
generator."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dwconv_bits.json")

SHAPES = [(3, 1, 13), (5, 2, 21), (3, 2, 33), (5, 2, 128), (3, 1, 2), (5, 2, 3)]
# name -> (kind, K, S, Lin, C, N, NP)
CASES = {}
for _k, _s, _l in SHAPES:
    CASES["f32_k%ds%d_L%d" % (_k, _s, _l)] = ("f32", _k, _s, _l, 16, 1300, 1536)
    CASES["bf16_k%ds%d_L%d" % (_k, _s, _l)] = ("bf16", _k, _s, _l, 16, 1300, 1536)
CASES["f32_trip2_k3s1_L64"] = ("f32", 3, 1, 64, 8, 33000, 33024)
CASES["f32_trip2_k5s2_L21"] = ("f32", 5, 2, 21, 8, 33000, 33024)
CASES["bf16_wide_k3s1_L64"] = ("bf16", 3, 1, 64, 8, 33000, 33024)
CASES["gather_k5s1_L9"] = ("gather", 5, 1, 9, 16, 1300, 1536)
CASES["gather_k3s3_L10"] = ("gather", 3, 3, 10, 16, 1300, 1536)


def _sha(t):
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


_last = {}                                      # the operands of the last case and a copy: its second run reuses them


def _operands(name, K, Lin, Lout, Cn, NP):
    if name not in _last:
        _last.clear()
        o = _make_operands(name, K, Lin, Lout, Cn, NP)
        _last[name] = (o, {k: v.clone() for k, v in o.items()})
    return _last[name][0]


def inputs_untouched(name):
    """no launch of the case wrote into one of its inputs (they are shared between its two runs)"""
    o, copy = _last[name]
    return all(torch.equal(o[k].view(torch.int32), copy[k].view(torch.int32)) for k in o)


def _make_operands(name, K, Lin, Lout, Cn, NP):
    g = torch.Generator().manual_seed(int(hashlib.sha256(name.encode()).hexdigest()[:8], 16))
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    o = dict(zin=rnd(Cn, Lin, NP), sc=rnd(Cn) * 0.3 + 1, sh=rnd(Cn) * 0.2, mean=rnd(Cn) * 0.1, w=rnd(Cn, 1, K) * 0.5,
             b=rnd(Cn) * 0.1, dy=rnd(Cn, Lout, NP), z=rnd(Cn, Lout, NP), ca=rnd(Cn) * 0.5 + 1, cb=rnd(Cn) * 0.1,
             cc=rnd(Cn) * 0.05)
    o["sc"][5], o["sh"][5] = 0.0, 0.3           # BatchNorm weight exactly zero
    o["sc"][3], o["sh"][3] = 1e-6, 0.3          # |sh| > 65536 |sc|
    return {k: v.to(DEV) for k, v in o.items()}


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def _written(name, t, rows):
    """t: NaN-filled buffer with one guard channel (octet) behind `rows` leading ones"""
    assert torch.isfinite(t[:rows].float()).all(), "%s: not finite everywhere" % name
    assert torch.isnan(t[rows:].float()).all(), "%s: written past the last channel" % name
    return _sha(t[:rows])


def _run_f32(name, kind, K, S, Lin, Cn, N, NP):
    from tinyrecurrentunet_amd import _lib as L
    from tinyrecurrentunet_amd._lib import check, ptr
    lib, st = L.lib(), L.stream()
    Lout = (Lin + 2 * (K // 2) - K) // S + 1
    o = _operands(name, K, Lin, Lout, Cn, NP)
    sha = {}
    z = _nan(Cn + 1, Lout, NP)
    part = _nan(lib.trunet_dwconv_nparts(Lout) * Cn * 2)
    check(lib.trunet_dwconv_fwd(ptr(o["zin"]), ptr(o["sc"]), ptr(o["sh"]), ptr(o["w"]), ptr(o["b"]), ptr(z), ptr(part), Cn, K, S,
                                Lin, Lout, NP, N, st), "fwd")
    sha["fwd.z"] = _written("fwd.z", z, Cn)
    sha["fwd.partials"] = _written("fwd.partials", part, part.numel())
    zf = z[:Cn].contiguous()
    nparts = lib.trunet_dwconv_bwd_nparts(Lin)
    for tag in ("bwd", "bwd_rz"):
        din, pr, wp, bp = _nan(Cn + 1, Lin, NP), _nan(nparts * Cn * 2), _nan(nparts * Cn * K), _nan(nparts * Cn)
        tail = (ptr(o["ca"]), ptr(o["cb"]), ptr(o["cc"]), ptr(o["zin"]), ptr(o["sc"]), ptr(o["sh"]), ptr(o["mean"]), ptr(o["w"]),
                ptr(din), ptr(pr), ptr(wp), ptr(bp), Cn, K, S, Lin, Lout, NP, N, st)
        if tag == "bwd":
            check(lib.trunet_dwconv_bwd(ptr(o["dy"]), ptr(zf), *tail), tag)
        else:
            prev = os.environ.get("TRUNET_DW_RZ")
            os.environ["TRUNET_DW_RZ"] = "2"     # also below 32 output positions
            try:
                rc = lib.trunet_dwconv_bwd_rz(ptr(o["dy"]), ptr(o["b"]), *tail)
            finally:
                if prev is None:
                    del os.environ["TRUNET_DW_RZ"]
                else:
                    os.environ["TRUNET_DW_RZ"] = prev
            if kind == "gather":
                assert rc == L.TRUNET_ENOTSUP, rc
                torch.cuda.synchronize()
                assert torch.isnan(din).all() and torch.isnan(pr).all(), "a refused launch wrote"
                continue
            check(rc, tag)
        sha[tag + ".dy_in"] = _written(tag + ".dy_in", din, Cn)
        for nm, t in (("partials_in", pr), ("w_partials", wp), ("b_partials", bp)):
            sha["%s.%s" % (tag, nm)] = _written("%s.%s" % (tag, nm), t, t.numel())
    return sha


def _to_oct(x):
    Cn, Ln, NP = x.shape
    return x.view(Cn // 8, 8, Ln, NP).permute(0, 2, 3, 1).contiguous().bfloat16()


def _run_bf16(name, kind, K, S, Lin, Cn, N, NP):
    from tinyrecurrentunet_amd import _lib as L
    from tinyrecurrentunet_amd._lib import check, ptr, ptr16
    lib, st = L.lib(), L.stream()
    Lout = (Lin + 2 * (K // 2) - K) // S + 1
    o = _operands(name, K, Lin, Lout, Cn, NP)
    zin16, dy16, z16 = _to_oct(o["zin"]), _to_oct(o["dy"]), _to_oct(o["z"])
    sha = {}
    zout = _nan(Cn // 8 + 1, Lout, NP, 8, dtype=torch.bfloat16)
    part = _nan(lib.trunet_bf16_dw_nparts(NP, Lout) * Cn * 2)
    check(lib.trunet_bf16_dwconv_fwd(ptr16(zin16), ptr(o["sc"]), ptr(o["sh"]), ptr(o["w"]), ptr(o["b"]), ptr16(zout), ptr(part),
                                     Cn, K, S, Lin, Lout, NP, N, st), "fwd")
    sha["fwd.z"] = _written("fwd.z", zout, Cn // 8)
    sha["fwd.partials"] = _written("fwd.partials", part, part.numel())
    nparts = lib.trunet_bf16_dw_nparts(NP, Lin)
    din = _nan(Cn // 8 + 1, Lin, NP, 8, dtype=torch.bfloat16)
    pr, wp, bp = _nan(nparts * Cn * 2), _nan(nparts * Cn * K), _nan(nparts * Cn)
    check(lib.trunet_bf16_dwconv_bwd(ptr16(dy16), ptr16(z16), ptr(o["ca"]), ptr(o["cb"]), ptr(o["cc"]), ptr16(zin16), ptr(o["sc"]),
                                     ptr(o["sh"]), ptr(o["mean"]), ptr(o["w"]), ptr16(din), ptr(pr), ptr(wp), ptr(bp), Cn, K, S,
                                     Lin, Lout, NP, N, st), "bwd")
    sha["bwd.dy_in"] = _written("bwd.dy_in", din, Cn // 8)
    for nm, t in (("partials_in", pr), ("w_partials", wp), ("b_partials", bp)):
        sha["bwd." + nm] = _written("bwd." + nm, t, t.numel())
    return sha


def run_case(name):
    """-> {tensor name: sha256} of everything the case's launches wrote"""
    c = CASES[name]
    return (_run_bf16 if c[0] == "bf16" else _run_f32)(name, *c)


@pytest.fixture(scope="module")
def golden_bits():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_dwconv_bits(name, golden_bits):
    sha = run_case(name)
    assert name in golden_bits, "no recorded bits for this case: run tests/golden/make_dwconv_bits.py on the parent build"
    diff = sorted(k for k in set(sha) | set(golden_bits[name]) if sha.get(k) != golden_bits[name].get(k))
    assert not diff, "%s: differ from the recorded bits: %s" % (name, ", ".join(diff))
    assert inputs_untouched(name), "a kernel wrote into one of its inputs"
    assert run_case(name) == sha, "two runs of the same launches differ"
    assert inputs_untouched(name), "a kernel wrote into one of its inputs"
