"""GPU: conv_gemm_kernel (gemm_conv.hip), the forward implicit GEMM on the fp32 MFMA, after its epilogue and loop
bookkeeping were rewritten (buffer-addressed rows, per-row parameters in registers, uniform flag / bound branches,
compile-time ring depth).  The rewrite must not change one output bit, so every case checks three things:

  * output rows and statistics against a float64 product of the same fp32 operands.  Output: the rigorous bound of an fp32
    dot product of K terms in any summation order, |err| <= (K + 3) 2^-24 (|W| |v| + |bias| + |old|) per element (K
    multiply-adds, the bias add, the accumulate add, one spare).  Statistics: 2e-5 of the largest statistic, the bound
    tests/test_gemm_x3_gpu.py holds the fp32-MFMA kernel to;
  * sha256 of the output rows and of the statistics partials equal to tests/golden/conv_gemm_fp32_bits.json, recorded once
    with the library of the commit before the rewrite (tests/golden/make_conv_gemm_bits.py);
  * a second run gives the same bits.

Inputs come from a seeded CPU generator.  Rows past M are guarded: the output buffer has extra rows that must stay NaN."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_gemm_fp32_bits.json")
GUARD = 8          # rows behind the M output rows that no launch may touch


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, dtype=torch.float32) * scale


def _x(g, C, Ln, NP, N):
    x = _randn(g, C, Ln, NP)
    x[:, :, N:] = 0.0                          # padding frames: finite
    return x


def _bn(g, C):
    return dict(c0=torch.rand(C, generator=g, dtype=torch.float32) + 0.5, c1=_randn(g, C, scale=0.3))


def _pointwise(M, K, P, N, NP, seed, bn=True, wscale=0.2):
    def make():
        g = torch.Generator().manual_seed(seed)
        W = _randn(g, M, K, scale=wscale)
        seg = dict(x=_x(g, K, P, NP, N), mul=1, off=0, div=1, woff=0, **(_bn(g, K) if bn else {}))
        return dict(M=M, segs=[seg], W=W, ldw_m=K, ldw_c=1, P=P, N=N, NP=NP, g=g)
    return make


def _two_sources():
    g = torch.Generator().manual_seed(5)
    N, NP, P = 600, 768, 8
    W = _randn(g, 64, 192, scale=0.15)
    s1 = dict(x=_x(g, 64, 7, NP, N), mul=1, div=1, off=-1, woff=0, **_bn(g, 64))      # one position of left padding
    s2 = dict(x=_x(g, 128, 8, NP, N), mul=1, div=1, off=0, woff=64, **_bn(g, 128))
    return dict(M=64, segs=[s1, s2], W=W, ldw_m=192, ldw_c=1, P=P, N=N, NP=NP, g=g)


def _transposed(k, s):
    def make():
        g = torch.Generator().manual_seed(10 * k + s)
        N, NP, Lin = 300, 512, 6
        pad = s // 2
        Lo = (Lin - 1) * s - 2 * pad + k
        W = _randn(g, 64, 64, k, scale=0.2)           # (Ci, Co, k): ldw_m = k, ldw_c = Co * k, woff = tap
        x = _x(g, 64, Lin, NP, N)
        bn = _bn(g, 64)
        segs = [dict(x=x, mul=1, off=pad - kk, div=s, woff=kk, **bn) for kk in range(k)]
        # the output tensor has two more positions than the launch writes: out_L != P
        return dict(M=64, segs=segs, W=W, ldw_m=k, ldw_c=64 * k, P=Lo, N=N, NP=NP, out_L=Lo + 2, out_pos_off=1, g=g)
    return make


def _masked(accum):
    def make():
        c = _pointwise(64, 64, 4, 300, 512, 77 + accum)()
        g = c["g"]
        c["zmask"] = _randn(g, 64 + GUARD, 4, 512)
        c["e0"] = torch.rand(64, generator=g, dtype=torch.float32) + 0.5
        c["e1"] = _randn(g, 64, scale=0.3)
        c["e2"] = _randn(g, 64, scale=0.3)
        if accum:
            c["old"] = _randn(g, 64 + GUARD, 4, 512)
        return c
    return make


CASES = {
    "wide_rs4_partial_tile": _pointwise(128, 128, 7, 700, 768, 1),
    "two_sources_left_pad": _two_sources,
    "transposed_k3s1": _transposed(3, 1),
    "transposed_k5s2": _transposed(5, 2),
    "transposed_k3s2": _transposed(3, 2),
    "three_row_blocks": _pointwise(384, 128, 4, 500, 512, 9, bn=False, wscale=0.1),
    "nw4_one_valid_frame": _pointwise(128, 64, 5, 257, 512, 3),
    "many_tiles_per_workgroup": _pointwise(64, 128, 33, 12000, 12032, 4),
    "ragged_row_block": _pointwise(40, 64, 3, 300, 512, 6),
    "no_partial_tile": _pointwise(64, 64, 4, 512, 512, 7),
    "single_frame": _pointwise(64, 64, 4, 1, 256, 8),
    "epl1_mask_stats": _masked(0),
    "epl2_mask_accum": _masked(1),
}
# the template instance each case must reach: (rs, nw, epl) of trunet_conv_gemm_plan
INSTANCE = {"wide_rs4_partial_tile": (4, 8, 0), "two_sources_left_pad": (2, 8, 0), "three_row_blocks": (4, 8, 0),
            "nw4_one_valid_frame": (4, 4, 0), "many_tiles_per_workgroup": (2, 4, 0), "ragged_row_block": (2, 4, 0),
            "epl1_mask_stats": (2, 8, 1), "epl2_mask_accum": (2, 4, 2)}


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def _reference(c, bias):
    """float64 output rows [M][P][NP], the per-element magnitude |W| |v| + |bias| + |old| and the statistics [M][2]"""
    M, P, NP, N = c["M"], c["P"], c["NP"], c["N"]
    off = c.get("out_pos_off", 0)
    Wf = c["W"].double().reshape(-1).to(DEV)
    ref = torch.zeros(M, P, NP, dtype=torch.float64, device=DEV)
    mag = torch.zeros_like(ref)
    for p in range(P):
        for s in c["segs"]:
            qn = p * s["mul"] + s["off"]
            if qn < 0 or qn % s["div"] or qn // s["div"] >= s["x"].shape[1]:
                continue
            v = s["x"][:, qn // s["div"]].double().to(DEV)
            if s.get("c0") is not None:
                v = torch.relu(s["c0"].double().to(DEV)[:, None] * v + s["c1"].double().to(DEV)[:, None])
            Cn = v.shape[0]
            idx = (torch.arange(M, device=DEV)[:, None] * c["ldw_m"] + torch.arange(Cn, device=DEV)[None, :] * c["ldw_c"]
                   + s["woff"])
            ref[:, p] += Wf[idx] @ v
            mag[:, p] += Wf[idx].abs() @ v.abs()
    ref += bias.double().to(DEV)[:, None, None]
    mag += bias.double().abs().to(DEV)[:, None, None]
    if c.get("old") is not None:
        old = c["old"][:M, off:off + P].double().to(DEV)
        ref += old
        mag += old.abs()
    if c.get("zmask") is not None:
        z = c["zmask"][:M, off:off + P].double().to(DEV)
        keep = (c["e0"].double().to(DEV)[:, None, None] * z + c["e1"].double().to(DEV)[:, None, None]) > 0
        ref = torch.where(keep, ref, torch.zeros_like(ref))
        second = ref * (z - c["e2"].double().to(DEV)[:, None, None])
    else:
        keep = None
        second = ref * ref
    st = torch.stack([ref[:, :, :N].sum((1, 2)), second[:, :, :N].sum((1, 2))], 1)
    return ref, mag, keep, st


def run_case(name):
    """-> (case dict, output rows [M][P][NP] on the GPU, raw statistics partials, sha256 of both)"""
    from tinyrecurrentunet_amd import _lib as L
    from tinyrecurrentunet_amd._lib import EPI_ACCUM, PRO_BNRELU, PRO_NONE, make_seg
    from tinyrecurrentunet_amd.engine import TRUNetEngine, Workspace
    import ctypes as C
    c = CASES[name]()
    M, P, NP, N = c["M"], c["P"], c["NP"], c["N"]
    out_L, off = c.get("out_L", P), c.get("out_pos_off", 0)
    bias = _randn(c["g"], M, scale=0.3)
    dev = {}

    def d(t):                                   # one device copy per host tensor (the taps share their source)
        if t is None:
            return None
        if id(t) not in dev:
            dev[id(t)] = t.to(DEV)
        return dev[id(t)]
    segs = [make_seg(d(s["x"]), s["x"].shape[0], s["x"].shape[1], s["mul"], s["off"], s["div"], s["woff"],
                     PRO_BNRELU if s.get("c0") is not None else PRO_NONE, c0=d(s.get("c0")), c1=d(s.get("c1")))
            for s in c["segs"]]
    lib = L.lib()
    prev = lib.trunet_gemm_x3_enable(-1)
    try:
        lib.trunet_gemm_x3_enable(0)
        eng, w = TRUNetEngine(None), Workspace(torch.device(DEV))
        out = torch.full((M + GUARD, out_L, NP), float("nan"), device=DEV)
        kw = {}
        if c.get("zmask") is not None:
            kw = dict(zmask=d(c["zmask"]), e0=d(c["e0"]), e1=d(c["e1"]), e2=d(c["e2"]))
        if c.get("old") is not None:
            out.copy_(d(c["old"]))
            out[M:] = float("nan")
            kw["epi"] = EPI_ACCUM
        a = eng._gemm_args(N=N, NP=NP, P=P, M=M, out=out, out_L=out_L, W=d(c["W"]), ldw_m=c["ldw_m"], ldw_c=c["ldw_c"],
                           segs=segs, bias=d(bias))
        a.epi |= kw.get("epi", 0) | (L.EPI_MASK if kw.get("zmask") is not None else 0)
        v = [C.c_int() for _ in range(6)]
        L.check(lib.trunet_conv_gemm_plan(a, *[C.byref(x) for x in v]), "plan")
        rs, kc, nb, two, epl, nw = [x.value for x in v]
        print("%s: conv_gemm_kernel<%d, %d, %s, %d, %d>, %d ring slots" % (name, rs, kc, "true" if two else "false", epl, nw, nb))
        assert nw > 0, "the fp32-MFMA kernel is under test, the plan says x3"
        if name in INSTANCE:
            assert (rs, nw, epl) == INSTANCE[name], (rs, nw, epl)
        nparts = eng._gemm(w, N=N, NP=NP, P=P, M=M, out=out, out_L=out_L, W=d(c["W"]), ldw_m=c["ldw_m"], ldw_c=c["ldw_c"],
                           segs=segs, bias=d(bias), out_pos_off=off, stats=M, **kw)
        torch.cuda.synchronize()
    finally:
        lib.trunet_gemm_x3_enable(prev)
    assert torch.isnan(out[M:]).all(), "rows past M were written"
    if out_L != P:
        assert torch.isnan(out[:M, :off]).all() and torch.isnan(out[:M, off + P:]).all(), "positions outside the launch were written"
    rows = out[:M, off:off + P].contiguous()
    part = w.t["partials"][:nparts * M * 2].clone()
    c["bias"] = bias
    return c, rows, part.view(nparts, M, 2), {"out": _sha(rows), "partials": _sha(part)}


@pytest.fixture(scope="module")
def golden_bits():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_conv_gemm_fp32_bits_and_float64(name, golden_bits):
    c, rows, part, sha = run_case(name)
    M, N = c["M"], c["N"]
    K = sum(s["x"].shape[0] for s in c["segs"])
    ref, mag, keep, st_ref = _reference(c, c["bias"])
    assert torch.isfinite(rows).all()
    err = (rows.double() - ref).abs()
    bound = (K + 3) * 2.0 ** -24 * mag + 1e-30
    if keep is not None:
        # a value within its rounding error of the mask threshold may fall on either side: e0 z + e1 is one fp32 fma
        z = c["zmask"][:M, c.get("out_pos_off", 0):c.get("out_pos_off", 0) + c["P"]].double().to(DEV)
        t = c["e0"].double().to(DEV)[:, None, None] * z + c["e1"].double().to(DEV)[:, None, None]
        sure = t.abs() > 2.0 ** -23 * (t.abs() + 1.0)
        err, bound = err[sure], bound[sure]
    worst = (err / bound).max().item()
    print("%s: worst |err| / ((K + 3) 2^-24 (|W||v| + |bias| + |old|)) = %.3f, max |err| / max |out| = %.2e" % (
        name, worst, err.max().item() / ref.abs().max().item()))
    assert worst <= 1.0, worst
    st = part.double().sum(0)
    dst = (st - st_ref).abs().max().item() / st_ref.abs().max().item()
    print("%s: statistics vs float64: %.2e of the largest" % (name, dst))
    assert dst < 2e-5, dst
    # bit for bit what the kernel computed before the epilogue rewrite
    assert name in golden_bits, "no recorded bits for this case: run tests/golden/make_conv_gemm_bits.py on the parent build"
    assert sha["out"] == golden_bits[name]["out"], "output rows differ from the recorded bits"
    assert sha["partials"] == golden_bits[name]["partials"], "statistics partials differ from the recorded bits"
    # and the same bits again
    _, _, _, sha2 = run_case(name)
    assert sha2 == sha, "two runs of the same launch differ"
