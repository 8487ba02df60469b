"""The loss tail of fft.hip on its own, through the C ABI, against the float64 restatement of tests/losstail_ref.py:
trunet_mask_istft_fwd / trunet_mask_istft_bwd, trunet_l1_grad, trunet_reduce_cols, trunet_stft_mag / trunet_stft_mag_bwd,
trunet_stft_loss_fwd / trunet_stft_loss_fwdgrad / trunet_stft_loss_bwd_gather, trunet_loss_finalize and
trunet_loss_grad_gather, at the smallest shapes that reach their edges (tests/losstail_cases.py, where the cases, the
tolerances and the generator's conditions are stated).  Every output element of every case is compared; outputs are
prefilled with NaN, every buffer has a sentinel behind it, and a repeat launch must give the same bits.
DESIGN.md, "What pins the loss tail", has the table of what a run measured."""
import pytest
import torch

import losstail_cases as G

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", G.STFT_SHAPES, ids=lambda s: "n%d-h%d-w%d-L%d" % s)
def test_stft_kernels_match_fp64(shape):
    """trunet_stft_mag, trunet_stft_mag_bwd (a random cotangent), trunet_stft_loss_fwd, trunet_stft_loss_fwdgrad and
    trunet_stft_loss_bwd_gather on every regime of the shape: magnitudes, the three sums per frame, both gradient frame
    tables, the recomputing backward's frames and gradient, all through convt_ref.close; fwdgrad's sums bit-equal to fwd's;
    c_sc OLA(fr_sc) + c_mag OLA(fr_mag) (trunet_loss_grad_gather on fwdgrad's own tables) inside close of the same float64
    gradient as trunet_stft_loss_bwd_gather on the same coefficients; x == y everywhere gives exact zeros"""
    for case in G.STFT_CASES:
        if case[:4] == shape:
            c = G.stft_inputs(case)
            got = G.stft_gpu(c)
            G.judge_stft(c, got)
            G.same_bits(got, G.stft_gpu(c), G.stft_id(case))


@pytest.mark.parametrize("nres", G.GATHER_CASES)
def test_loss_grad_gather_matches_fp64(nres):
    """trunet_loss_grad_gather on random frame tables of 0, 1, 3 and 8 mixed resolutions (compile-time and runtime sizes,
    wl == n, odd wl, hop > wl) at one L that is no multiple of 256, random coefficients, g_loss = 2.5, audio == clean on a
    stretch: the adjoint of the reflect pad written as a scatter is the reference"""
    c = G.gather_inputs(nres)
    got = G.gather_gpu(c)
    G.judge_gather(c, got)
    G.same_bits(got, G.gather_gpu(c), "gather nres %d" % nres)


@pytest.mark.parametrize("T", G.MASK_T)
def test_mask_istft_forward_and_backward_match_fp64(T):
    """trunet_mask_istft_fwd (frames, audio, the L1 block sums of trunet_mask_istft_l1_nparts(B, L) entries, the 128-sample
    tail block of L = 128 odd included) and trunet_mask_istft_bwd at B = 3, beta 0.5 and 2.0, with and without clean, on
    generic outputs, c0 exactly +-1 and beyond, exactly-zero phase pairs and pairs on the negative real axis (+0 and -0)"""
    for case in G.MASK_CASES:
        if case[0] == T:
            c = G.mask_inputs(case)
            got = G.mask_gpu(c)
            G.judge_mask(c, got)
            G.same_bits(got, G.mask_gpu(c), G.mask_id(case))


def test_reduce_cols_is_one_rounding_of_the_exact_sum():
    """trunet_reduce_cols at 1, 1023, 1024, 1025, 4096, 4097 and 8197 rows (the 4096-row main loop against its tail), 1 and
    3 columns"""
    for case in G.RC_CASES:
        c = G.rc_inputs(case)
        G.judge_rc(c, G.rc_gpu(c))


def test_loss_finalize_matches_its_counted_roundings_and_leaves_its_scratch_zero():
    """trunet_loss_finalize over the same row classes, nres 0 / 1 / 3 / 8, stft_lambda 0 / 0.7 / 1, sc_lambda != mag_lambda,
    a resolution with S1 == 0 (c_sc exactly 0, everything finite); two launches on one scratch buffer give the same bits and
    leave it all zero"""
    for case in G.FIN_CASES:
        c = G.fin_inputs(case)
        G.judge_fin(c, G.fin_gpu(c))


def test_l1_grad_is_exact():
    """trunet_l1_grad: scale * sign(den - clean), exact bits, 0 where den == clean, n around the 256-thread block"""
    for n in G.L1_N:
        c = G.l1_inputs(n)
        got = G.l1_gpu(c)
        G.judge_l1(c, got)
        G.same_bits(got, G.l1_gpu(c), "l1_grad %d" % n)


def test_identical_signals_give_a_zero_loss_and_an_exactly_zero_finite_gradient():
    """x == y everywhere, through the fused chain trunet_stft_loss_fwdgrad -> trunet_loss_finalize ->
    trunet_loss_grad_gather and through stft_loss.py's autograd path (trunet_stft_loss_fwd, trunet_reduce_cols,
    trunet_stft_loss_bwd_gather): every loss term is 0 and every gradient element is finite and exactly 0, as torch has it
    (tests/test_losstail_ref_cpu.py).  Before the S1 == 0 branch the coefficient 1 / (sqrt(S1) sqrt(S2)) was inf and the
    gradient NaN in every sample."""
    got = G.identical_chain_gpu()
    v, g = got["vals"], got["g_audio"]
    print("IDENTICAL fused: vals %s  max|g| %s" % (v.tolist(), float(g.abs().max())))
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(g).all())
    assert bool((v[:4] == 0).all()) and bool((v[5::2] == 0).all()) and bool((v[6::2] > 0).all())
    assert bool((g == 0).all())
    from tinyrecurrentunet_amd import stft_loss as sl
    n_res = list(zip(*G.IDENT_RES))
    mr = sl.MultiResolutionSTFTLoss(fft_sizes=list(n_res[0]), hop_sizes=list(n_res[1]), win_lengths=list(n_res[2]),
                                    sc_lambda=0.5, mag_lambda=0.5).cuda()
    y = (G.AMP * G._rn(G._gen("identical"), 2, G.IDENT_L)).cuda()
    x = y.clone().requires_grad_(True)
    sc, mag = mr(x, y)
    (2.5 * (sc + mag)).backward()
    print("IDENTICAL autograd: sc %s mag %s max|g| %s" % (float(sc), float(mag), float(x.grad.abs().max())))
    assert float(sc) == 0 and float(mag) == 0
    assert bool(torch.isfinite(x.grad).all()) and bool((x.grad == 0).all())
