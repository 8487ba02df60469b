"""The BatchNorm statistics chain and the block-boundary kernels on their own, through the C ABI, against the float64
restatements of tests/bn_ref.py: trunet_bn_finalize_fwd / _bwd, trunet_bn_eval_affine, trunet_relu_bwd_stats,
trunet_from_frames_last_affine, trunet_conv_first_fwd, trunet_sumsq (elementwise.hip) and trunet_reduce_partials
(gemm_conv.hip), at the smallest shapes that reach their edges (tests/bn_cases.py, where the tolerances are derived).  Every
output element of every case is compared; outputs are prefilled with NaN and every buffer has a sentinel behind it.
DESIGN.md, "What pins the BatchNorm chain and the block-boundary kernels", has the table of what a run measured."""
import pytest
import torch

import bn_cases as G

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nparts", G.NPARTS)
def test_finalize_kernels_match_fp64_at_the_partial_image_edges(nparts):
    """both finalize kernels at nparts around their 256-row stride, C = 1 / 24 / 192, count = 1690 / 1 / 2^24 + 3; the
    forward one with running statistics NULL and non-NULL x counter NULL and non-NULL at EVERY count (momentum 0.1 and 1.0
    with running statistics: running_var's unbiased branch at count > 1 and the biased one at count == 1): the
    one-rounding outputs (mean, rstd, dgamma, dbeta, ca, cb, cc) within 2 U |ref| + D sum|terms|, the fp32-arithmetic ones (scale, shift, running statistics) within (r + 1) U
    sum|terms|; afterwards the consumed partial image is exactly +0 everywhere (the PREZERO producers rely on it), the
    int64 counter rose by exactly 1 (its neighbour untouched) and no sentinel moved"""
    for case in G.FIN_CASES:
        if case[0] == nparts:
            c = G.fin_inputs(case)
            G.judge_fin_fwd(c, G.fin_fwd_gpu(c))
            if case in G.FIN_BWD_CASES:
                G.judge_fin_bwd(c, G.fin_bwd_gpu(c))


@pytest.mark.parametrize("case", G.REG_CASES)
def test_finalize_fwd_regimes_stay_inside_the_conditioning_bound(case):
    """partials built as double sums per part rounded to fp32; channels: mean ~ 0, |mean| / std = 5, |mean| / std = 100, a
    constant 0.7 (variance clamps at 0: rstd finite and at most 1 / sqrt(eps)), gamma < 0, gamma = 0 (scale exactly 0, shift
    exactly beta).  mean, rstd, scale and shift against float64 of the DATA within twice the conditioning bound"""
    c = G.reg_inputs(case)
    G.judge_reg(c, G.reg_gpu(c))


@pytest.mark.parametrize("Cn", G.EVAL_C)
def test_eval_affine_matches_fp64(Cn):
    """C around the 128-thread block; a channel with running_var = 0 and one with a negative weight"""
    c = G.eval_inputs(Cn)
    G.judge_eval(c, G.eval_gpu(c))


@pytest.mark.parametrize("case", G.RELU_CASES, ids=G.relu_id)
def test_relu_bwd_stats_matches_fp64(case):
    """plain ReLU (scale / shift / mean / partials NULL) and BatchNorm + ReLU with statistics: masked dy bit-exact against
    the restatement (strict >: the planted pre = 0 elements are masked; channels with scale < 0, with scale 0 and shift > 0 /
    < 0), exactly +0 for frames >= N although dy and z hold NaN there; every partial row finite, rows of workgroups without
    an item exactly 0; summed over the parts, both sums through convt_ref.close against float64, the yardstick the
    element-wise worse of a per-workgroup sequential fp32 chain and sums blocked by 128"""
    c = G.relu_inputs(case)
    G.judge_relu(c, G.relu_gpu(c))


@pytest.mark.parametrize("case", G.FFL_CASES, ids=G.ffl_id)
def test_from_frames_last_affine_matches_fp64(case):
    """channel boundaries inside the 32-row tiles, relu on and off (negative results come through), negative and zero
    scales, NaN in the frames >= N; within 2 U (|scale x| + |shift|); nothing written beyond N C L"""
    c = G.ffl_inputs(case)
    G.judge_ffl(c, G.ffl_gpu(c))


@pytest.mark.parametrize("S,Lin", G.CF_SL)
def test_conv_first_matches_fp64(S, Lin):
    """Cin 3 / 4, Cout 5 / 64, NP 128 / 384, all NP columns: F.conv1d(padding = S // 2) + ReLU in double through
    convt_ref.close, the yardstick the worse of torch's fp32 conv and one sequential fma-free chain over (ci, k)"""
    for case in G.CF_CASES:
        if case[2:4] == (S, Lin):
            c = G.cf_inputs(case)
            G.judge_cf(c, G.cf_gpu(c))


@pytest.mark.parametrize("nparts", G.RP_NPARTS)
def test_reduce_partials_matches_fp64(nparts):
    """both instantiations (numel <= 4096 with nparts >= 64, and the rest), accumulate = 0 on a NaN-prefilled out (one
    rounding) and accumulate = 1 (r = 2); the partial image is left as it was"""
    for case in G.RP_CASES:
        if case[0] == nparts:
            c = G.rp_inputs(case)
            G.judge_rp(c, G.rp_gpu(c))


def test_sumsq_matches_fp64():
    """n around the float4 and the 1024-thread edges, from an aligned pointer and from one a float further (the scalar
    path): one rounding of the double sum"""
    for case in G.SQ_CASES:
        c = G.sq_inputs(case)
        G.judge_sq(c, G.sq_gpu(c))


@pytest.mark.parametrize("case", G.CHAIN_CASES, ids=G.chain_id)
def test_chain_matches_fp64_autograd(case):
    """finalize_fwd -> relu_bwd_stats -> finalize_bwd on the GPU, dz = ca dy + cb z + cc formed in torch from the kernels'
    fp32 coefficients: dz, dgamma, dbeta against float64 autograd through relu(F.batch_norm(z, training = True)) with
    torch's own fp32 autograd as yardstick; a second run repeats every output of every stage bit for bit"""
    c = G.chain_inputs(case)
    got = G.chain_gpu(c)
    G.judge_chain(c, got)
    G.chain_same_bits(got, G.chain_gpu(c))


@pytest.mark.parametrize("case", G.CHAIN_ILL, ids=G.chain_id)
def test_ill_conditioned_chain_stays_inside_the_conditioning_bound(case):
    """|mean| / std = 100: the variance is sumsq / count - mean^2 in double, but from fp32 partial sums -- a design limit.
    The chain is held to the analytic conditioning bound (bn_cases.judge_chain_ill), not to torch's fp32 autograd; the line
    it prints says how many times torch's fp32 error the kernels' is"""
    c = G.chain_inputs(case)
    G.judge_chain_ill(c, G.chain_gpu(c))
