"""GPU: the depth-2 ring instances of conv_gemm_kernel (gemm_conv.hip, NBT == 2) over long chunk sequences.

These instances run the chunk loop in their own order (MFMAs of chunk i, then the DMA wait and the prologue pass on chunk
i + 1, then the barrier).  tests/test_conv_gemm_epilogue_gpu.py reaches them only with one tile per workgroup; here every
workgroup owns two to three tiles, so the loop crosses tile boundaries, takes the ragged last chunk of a tile (K = 112) and
walks the taps of a stride-2 transposed conv.  Every case checks:

  * through trunet_conv_gemm_plan that the launch is a depth-2 instance with the expected (rs, nw, epl): a case that no
    longer reaches one fails;
  * the float64 bounds of tests/test_conv_gemm_epilogue_gpu.py: |err| <= (K + 3) 2^-24 (|W| |v| + |bias|) per element,
    statistics within 2e-5 of the largest;
  * sha256 of the output rows and of the statistics partials equal to tests/golden/conv_gemm_ring2_bits.json, recorded with
    the library of the commit before the reordering (tests/golden/make_conv_gemm_ring2_bits.py);
  * a second run gives the same bits;
  * the guard rows past M are still NaN.

Inputs come from a seeded CPU generator; BN+ReLU prologue and statistics are on in every case."""
import ctypes as C
import json
import os

import pytest
import torch

import test_conv_gemm_epilogue_gpu as T

pytestmark = pytest.mark.gpu
DEV = T.DEV
GUARD = T.GUARD
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_gemm_ring2_bits.json")


def _transposed_k5s2():
    """ConvTranspose1d 64 -> 64, k = 5, s = 2 over Lin = 20 positions: Lo = 41, taps of either parity"""
    g = torch.Generator().manual_seed(52)
    k, s, N, NP, Lin = 5, 2, 4000, 4096, 20
    pad = s // 2
    Lo = (Lin - 1) * s - 2 * pad + k
    assert Lo == 41
    W = T._randn(g, 64, 64, k, scale=0.2)             # (Ci, Co, k): ldw_m = k, ldw_c = Co * k, woff = tap
    x = T._x(g, 64, Lin, NP, N)
    bn = T._bn(g, 64)
    segs = [dict(x=x, mul=1, off=pad - kk, div=s, woff=kk, **bn) for kk in range(k)]
    return dict(M=64, segs=segs, W=W, ldw_m=k, ldw_c=64 * k, P=Lo, N=N, NP=NP, out_L=Lo + 2, out_pos_off=1, g=g)


CASES = {
    # 768 tiles of 256 frames over 256 workgroups: three tiles each, four chunks per tile
    "wide_rs4_many_tiles": T._pointwise(128, 128, 12, 16000, 16384, 21),
    # the same with K = 112: the last chunk of every tile has 16 rows (clamped rows in the DMA and the prologue pass)
    "wide_rs4_ragged_k": T._pointwise(128, 112, 12, 16000, 16384, 22),
    # 656 tiles of 256 frames over 256 workgroups: two or three tiles each, two or three taps of two chunks per tile
    "wide_rs2_transposed_k5s2": _transposed_k5s2,
    # 768 tiles of 128 frames over 512 workgroups (two per CU): one or two tiles each, two chunks per tile
    "nw4_two_per_cu": T._pointwise(128, 64, 12, 8100, 8192, 23),
}
# (rs, nw, epl) and the ring depth trunet_conv_gemm_plan must report
INSTANCE = {"wide_rs4_many_tiles": (4, 8, 0), "wide_rs4_ragged_k": (4, 8, 0), "wide_rs2_transposed_k5s2": (2, 8, 0),
            "nw4_two_per_cu": (4, 4, 0)}
DEPTH = 2


def run_case(name):
    """-> (case dict, output rows [M][P][NP] on the GPU, statistics partials [nparts][M][2], sha256 of both)"""
    from tinyrecurrentunet_amd import _lib as L
    from tinyrecurrentunet_amd._lib import PRO_BNRELU, make_seg
    from tinyrecurrentunet_amd.engine import TRUNetEngine, Workspace
    c = CASES[name]()
    M, P, NP, N = c["M"], c["P"], c["NP"], c["N"]
    out_L, off = c.get("out_L", P), c.get("out_pos_off", 0)
    bias = T._randn(c["g"], M, scale=0.3)
    dev = {}

    def d(t):                                   # one device copy per host tensor (the taps share their source)
        if id(t) not in dev:
            dev[id(t)] = t.to(DEV)
        return dev[id(t)]
    segs = [make_seg(d(s["x"]), s["x"].shape[0], s["x"].shape[1], s["mul"], s["off"], s["div"], s["woff"], PRO_BNRELU,
                     c0=d(s["c0"]), c1=d(s["c1"])) for s in c["segs"]]
    lib = L.lib()
    prev = lib.trunet_gemm_x3_enable(-1)
    try:
        lib.trunet_gemm_x3_enable(0)
        eng, w = TRUNetEngine(None), Workspace(torch.device(DEV))
        out = torch.full((M + GUARD, out_L, NP), float("nan"), device=DEV)
        geo = dict(N=N, NP=NP, P=P, M=M, out=out, out_L=out_L, W=d(c["W"]), ldw_m=c["ldw_m"], ldw_c=c["ldw_c"], segs=segs,
                   bias=d(bias))
        a = eng._gemm_args(**geo)
        v = [C.c_int() for _ in range(6)]
        L.check(lib.trunet_conv_gemm_plan(a, *[C.byref(x) for x in v]), "plan")
        rs, kc, nb, two, epl, nw = [x.value for x in v]
        print("%s: conv_gemm_kernel<%d, %d, %s, %d, %d>, %d ring slots" % (name, rs, kc, "true" if two else "false", epl, nw, nb))
        assert (rs, nw, epl) == INSTANCE[name] and kc == 32 and not two, (rs, kc, two, epl, nw)
        assert nb == DEPTH, "the launch no longer reaches a depth-2 instance: %d ring slots" % nb
        nparts = eng._gemm(w, out_pos_off=off, stats=M, **geo)
        torch.cuda.synchronize()
    finally:
        lib.trunet_gemm_x3_enable(prev)
    assert torch.isnan(out[M:]).all(), "rows past M were written"
    if out_L != P:
        assert torch.isnan(out[:M, :off]).all() and torch.isnan(out[:M, off + P:]).all(), "positions outside the launch were written"
    rows = out[:M, off:off + P].contiguous()
    part = w.t["partials"][:nparts * M * 2].clone()
    c["bias"] = bias
    return c, rows, part.view(nparts, M, 2), {"out": T._sha(rows), "partials": T._sha(part)}


@pytest.fixture(scope="module")
def golden_bits():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_conv_gemm_ring2_bits_and_float64(name, golden_bits):
    c, rows, part, sha = run_case(name)
    K = sum(s["x"].shape[0] for s in c["segs"])
    ref, mag, _, st_ref = T._reference(c, c["bias"])
    assert torch.isfinite(rows).all()
    worst = ((rows.double() - ref).abs() / ((K + 3) * 2.0 ** -24 * mag + 1e-30)).max().item()
    print("%s: worst |err| / ((K + 3) 2^-24 (|W||v| + |bias|)) = %.3f" % (name, worst))
    assert worst <= 1.0, worst
    del ref, mag
    st = part.double().sum(0)
    dst = (st - st_ref).abs().max().item() / st_ref.abs().max().item()
    print("%s: statistics vs float64: %.2e of the largest" % (name, dst))
    assert dst < 2e-5, dst
    # bit for bit what the kernel computed before the loop of the depth-2 instances was reordered
    assert name in golden_bits, "no recorded bits for this case: run tests/golden/make_conv_gemm_ring2_bits.py on the parent build"
    assert sha["out"] == golden_bits[name]["out"], "output rows differ from the recorded bits"
    assert sha["partials"] == golden_bits[name]["partials"], "statistics partials differ from the recorded bits"
    # and the same bits again
    del rows, part
    _, _, _, sha2 = run_case(name)
    assert sha2 == sha, "two runs of the same launch differ"
