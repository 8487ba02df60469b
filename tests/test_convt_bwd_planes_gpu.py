"""The split instances of the fused ConvTranspose backward kernel (convt_bwd_kernel<K, S, true>) keep dz as bf16 planes, split
once by the prologue pass; the stride-2 instances do so on a ring with one step of DMA lead (csrc/convt_bwd.hip, CtLds::LA).
Here each is held against the fp32-MFMA instance of the same kernel (<K, S, false>, two steps of lead, no planes) on the same
inputs through the C ABI: both multiply the same fp32 numbers, so every output may differ by fp32 rounding only -- the A/B
bound of test_gemm_x3_gpu.test_x3_fused_backward_kernels_vs_their_fp32_mfma_instances, 2e-5 relative L2 per tensor.

Shapes: Lin 7 and 20 (Lout 13 / 15 and 39 / 41 for stride 2: the 5- and 7-deep dz rings and the 3-deep source ring wrap
several times, the last step has no successor to request) at N = 300 and 777 (a ragged last tile, workgroups without a
chunk), and N = 8300 in NP = 8448: 264 chunks over 256 workgroups, so eight workgroups walk a second chunk on rings the first
left behind.  (3, 1) runs the same cases as a control.  Against float64 the kernels are pinned by test_convt_bwd_gpu.py."""
import functools

import pytest
import torch

import convt_cases as G

pytestmark = pytest.mark.gpu

AB_BOUND = 2e-5
KS = ((5, 2), (3, 2), (3, 1))
SHAPES = ((7, 384, 300), (7, 896, 777), (20, 384, 300), (20, 896, 777), (7, 8448, 8300))
CASES = [(K, S, "ordinary", Lin, NP, N) for K, S in KS for Lin, NP, N in SHAPES]


@functools.lru_cache(maxsize=2)
def _fp32_instance(case):
    """inputs of the case and the fp32-MFMA instance's outputs on them: the reference, launched once and left unchanged"""
    c = G.inputs(case)
    return c, G.launch(c, "fp32")


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("case", CASES, ids=G.case_id)
def test_plane_instance_matches_the_fp32_mfma_instance(case):
    """dW and db (per-workgroup partial images and their sums), g and the statistics partials of the split instance within
    2e-5 relative L2 of the fp32-MFMA instance's; a second launch repeats every output bit; and the contract's exact parts
    over NaN-prefilled gradient and statistics buffers and sentinel-framed images: every element written, g = 0 for the
    padding frames >= N, nothing outside the weight slot and the bias row, zeros from the workgroups that own no chunk"""
    c, ref = _fp32_instance(case)
    got = G.launch(c, "split")
    tag = G.tag_of(c, "split")
    K = c.K
    slot = lambda o: o.wimg[:, G.W_OFF:G.W_OFF + G.C * G.C * K]
    brow = lambda o: o.bimg[:, G.B_OFF:G.B_OFF + G.C]
    sa, sb = G.sums(c, got), G.sums(c, ref)
    figures = {"dW partials": _rel_l2(slot(got), slot(ref)), "db partials": _rel_l2(brow(got), brow(ref)),
               "g": _rel_l2(got.dsrc, ref.dsrc), "statistics partials": _rel_l2(got.parts, ref.parts)}
    figures.update({k: _rel_l2(sa[k], sb[k]) for k in ("dW", "db", "st0", "st1")})
    print("%s vs fp32-MFMA instance, relative L2: %s" % (tag, "  ".join("%s %.2e" % kv for kv in figures.items())))
    assert float(ref.dsrc.norm()) > 0 and float(slot(ref).norm()) > 0
    for name, e in figures.items():
        assert e <= AB_BOUND, (tag, name, e)
    G.same_bits(got, G.launch(c, "split"), "%s: second launch" % tag)
    G.exactness(c, got, tag)
    G.exactness(c, ref, G.tag_of(c, "fp32"))
