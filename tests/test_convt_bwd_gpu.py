"""The fused ConvTranspose1d(64 -> 64) + BatchNorm backward kernels on their own, through the C ABI, against the float64
restatement of tests/convt_ref.py: convt_bwd_kernel<K, S, false> (fp32 MFMA), convt_bwd_kernel<K, S, true> (three-term
bf16 split, the default) and bconvt_bwd_kernel<K, S> (bf16 octets), for (K, S) in {(3,1), (3,2), (5,2)}, at the smallest
shapes that take every branch of their run-start, ring and chunk logic (tests/convt_cases.py).  Every element is compared;
the tolerance is convt_ref.close's, measured from the fp32 restatement (the bf16 emulation for the bf16 kernel) on the same
inputs.  DESIGN.md, "What pins the ConvTranspose backward kernels", has the table of what a run measured."""
import pytest
import torch

import convt_cases as G
import convt_ref as R

pytestmark = pytest.mark.gpu


def _case(case, bf16):
    return G.build(case, bf16) if G.is_big(case) else G.small(case, bf16)


def _mid(K, S, inst, regime="ordinary"):
    return (K, S, regime, G.MID_LIN) + (G.B16_MID if inst == "bf16" else G.F32_MID)


def test_torch_octet_packing_is_the_librarys():
    """the octet images the bf16 launches are fed are built in plain torch (index permutation + bf16 rounding): bit for bit
    what trunet_bf16_from_frames_last writes, and from_octets undoes it"""
    t = G.inputs((5, 2, "ordinary", 3, 192, 130)).dy
    ours = G.to_octets(t)
    assert torch.equal(ours.view(torch.int16), G.gpu_from_frames_last(t).view(torch.int16))
    assert torch.equal(G.from_octets(ours), R.bf16_round(t))


@pytest.mark.parametrize("case", G.F32_CASES, ids=G.case_id)
def test_fp32_and_split_kernels_match_fp64(case):
    """dW, db, dsrc and both statistics columns of the fp32-MFMA and of the split instance through `close`, then what must
    hold exactly: no NaN left in dsrc or the statistics rows, dsrc = 0 for frames >= N, the sentinels around the weight slot
    and the bias row untouched, all-zero images and rows from the workgroups that own no chunk, and the regime's exact
    zeros (masked-off tile, channels with pre <= 0 everywhere -- the one with pre = 0 tells > from >= --, zero cotangent)"""
    c = _case(case, False)
    for inst in ("fp32", "split"):
        G.check_case(c, inst)


@pytest.mark.parametrize("case", G.B16_CASES, ids=G.case_id)
def test_bf16_kernel_matches_fp64(case):
    """the same for the octet kernel, fp64 on the same bf16 inputs as reference and the rounding emulation as yardstick;
    prezero = 0 on NaN-prefilled statistics rows and prezero = 1 on zeroed ones give identical bits in every output"""
    c = _case(case, True)
    _, o = G.check_case(c, "bf16")
    o1 = G.launch(c, "bf16", prezero=True)
    G.same_bits(o, o1, "prezero = 1 against prezero = 0")


@pytest.mark.parametrize("inst", G.INSTANCES)
@pytest.mark.parametrize("K,S", G.KS)
def test_two_launches_are_bit_identical_and_bias_is_optional(K, S, inst):
    """determinism at the mid shape and at Lin = 9 ending inside a chunk: a second launch on the same inputs repeats every
    output bit for bit; b_partials = NULL changes nothing else"""
    small_npn = G.B16_NPN[1] if inst == "bf16" else G.F32_NPN[2]
    for case in (_mid(K, S, inst), (K, S, "ordinary", 9) + small_npn):
        c = _case(case, inst == "bf16")
        o1, o2 = G.launch(c, inst), G.launch(c, inst)
        G.same_bits(o1, o2, "%s: second launch" % G.tag_of(c, inst))
        o3 = G.launch(c, inst, bias=False)
        G.same_bits(o1, o3, "%s: b_partials = NULL" % G.tag_of(c, inst), skip=("bimg",))


@pytest.mark.parametrize("inst", G.INSTANCES)
@pytest.mark.parametrize("K,S", G.KS)
def test_dsrc_columns_do_not_see_their_neighbours(K, S, inst):
    """the data gradient has no cross-frame term: a 128-frame case embedded at a frame offset (another workgroup, another
    chunk) in a 384-frame launch whose other columns hold zeros, then `trained`-regime values times 100, gives the dsrc
    columns of the stand-alone launch bit for bit"""
    bf16 = inst == "bf16"
    off = 192 if bf16 else 160
    c = _case((K, S, "ordinary", 5, 128, 128), bf16)
    alone = G.launch(c, inst).dsrc
    loud = G.inputs((K, S, "trained", 5, 384, 384), bf16)
    for scale in (0.0, 100.0):
        e = G.inputs((K, S, "ordinary", 5, 384, 384), bf16)
        for k in ("ca", "cb", "cc", "s_scale", "s_shift", "s_mean", "W"):
            setattr(e, k, getattr(c, k))
        for k in ("dy", "z", "src"):
            t = getattr(loud, k) * scale
            t = R.bf16_round(t) if bf16 else t                           # the octet images hold bf16 values
            t[:, :, off:off + 128] = getattr(c, k)
            setattr(e, k, t)
        got = G.launch(e, inst).dsrc
        assert torch.equal(got[:, :, off:off + 128], alone), "%s: neighbours scaled %g" % (G.tag_of(c, inst), scale)
        assert scale == 0.0 or bool((got[:, :, :off] != 0).any())
