"""trunet_bf16_pw_bwd (bwgrad_kernel<true, *, true> in csrc/bf16.hip) and the unfused trunet_bf16_wgrad instances on their
own, through the C ABI, against the float64 restatement of tests/pwbwd16_ref.py.  `ordinary` cases go through
convt_ref.close with the fp32 emulation as the yardstick; `exact` cases must give the restatement's bits (the condition is
proven on the reference alone in tests/test_pwbwd16_ref_cpu.py).  Every launch runs on NaN-prefilled outputs between
sentinels; every comparison covers every element."""
import pytest
import torch

import pwbwd16_cases as PC
import pwbwd16_ref as R

pytestmark = pytest.mark.gpu

NS = PC.NS


@pytest.mark.parametrize("case", PC.SMALL, ids=PC.case_id)
def test_fused_backward_small_cases(case):
    PC.check_case(PC.small(case))


@pytest.mark.parametrize("case", PC.MID + PC.BIG, ids=PC.case_id)
def test_fused_backward_many_steps_per_workgroup(case):
    """1-2, 2-3 and 3-4 steps per workgroup, runs that cross chunk boundaries; the references are computed on the GPU in
    float64 / fp32 (yardstick: the blocked order alone, the tighter choice)"""
    c = PC.refs(PC.inputs(case), seq=False, dev="cuda")
    _, o = PC.check_case(c)
    assert bool(o.own.all())


STAT_CASES = [("enc128", "ordinary", 192, 130, 3), ("dec_pad", "ordinary", 64, 33, 3), ("seg3", "exact", 192, 130, 2)]


@pytest.mark.parametrize("case", STAT_CASES, ids=PC.case_id)
def test_prezeroed_statistics_rows_give_the_same_bits(case):
    """TRUNET_DG_PREZERO on zeroed rows and no flag on NaN-prefilled rows: identical bits in every output"""
    c = PC.small(case)
    PC.same_bits(PC.gpu_pw_bwd(c), PC.gpu_pw_bwd(c, prezero=True), "prezero " + PC.case_id(case))


@pytest.mark.parametrize("case", STAT_CASES + [("m16", "ordinary", PC.MID_NP, PC.MID_N, 5)], ids=PC.case_id)
def test_two_launches_give_the_same_bits_and_the_bias_rows_are_optional(case):
    c = PC.small(case) if PC.is_small(case) else PC.inputs(case)
    o1, o2, o3 = PC.gpu_pw_bwd(c), PC.gpu_pw_bwd(c), PC.gpu_pw_bwd(c, bias=False)
    PC.same_bits(o1, o2, "second launch " + PC.case_id(case))
    PC.same_bits(o1, o3, "b_partials = NULL " + PC.case_id(case), skip=("bimg",))


def _embed(c, NP, at, fill):
    """the case's frames at [at, at + c.NP) of an NP-frame launch (N = NP: every frame live); the other columns hold
    `fill` times seeded random bf16 values"""
    g = torch.Generator().manual_seed(at + NP)

    def wide(t):
        w = R.bf16_round(fill * torch.randn(t.shape[0], t.shape[1], NP, generator=g))
        w[:, :, at:at + c.NP] = t
        return w
    big = PC.to_device(c, "cpu")
    big.NP, big.N = NP, NP
    big.dy, big.z = wide(c.dy), wide(c.z)
    for s, sb in zip(c.segs, big.segs):
        sb.x, sb.prev = wide(s.x), wide(s.prev)
        if not s.bn:
            sb.x = sb.x.clamp_min(0) if bool((s.x >= 0).all()) else sb.x
    return big


@pytest.mark.parametrize("sig", ["enc128", "dec_crop", "seg3"])
def test_data_gradient_columns_do_not_see_their_neighbours(sig):
    """the data gradient has no cross-frame term: a 64-frame case embedded at frame 64 (another chunk, another workgroup) of
    a 192-frame launch whose other columns hold zeros, then values times 100, gives the stand-alone launch's out[s] columns
    bit for bit"""
    c = PC.inputs((sig, "ordinary", 64, 64, 3))
    alone = PC.gpu_pw_bwd(c)
    for fill in (0.0, 100.0):
        o = PC.gpu_pw_bwd(_embed(c, 192, 64, fill))
        for i in range(len(c.segs)):
            assert not bool(torch.isnan(PC.from_octets(o.out16[i])).any())
            assert torch.equal(o.out16[i][:, :, 64:128].view(torch.int16), alone.out16[i].view(torch.int16)), \
                "%s fill %g: out[%d] columns depend on their neighbours" % (sig, fill, i)


@pytest.mark.parametrize("two", [True, False], ids=["bnbwd_dz", "plain_dz"])
@pytest.mark.parametrize("case", PC.WGRAD_CASES, ids=PC.case_id)
def test_unfused_weight_gradient_instances(case, two):
    """trunet_bf16_wgrad = bwgrad_kernel<*, *, false>: every line under test but the data-gradient blocks, the 8-row and the
    4-channel thin shapes included, on NaN-prefilled partial images"""
    PC.check_wgrad(PC.small(case) if PC.is_small(case) else PC.inputs(case), two)


def _refusal(name):
    """(case, expected code name, what to change in the valid argument block)"""
    from tinyrecurrentunet_amd import _lib as Lb
    base = ("bn64", "ordinary", 64, 33, 3)

    def seg(**kw):
        def f(a):
            for k, v in kw.items():
                setattr(a.w.seg[0], k, v)
        return f

    def top(**kw):
        def f(a):
            for k, v in kw.items():
                setattr(a.w, k, v)
        return f

    def flags(a):
        a.dg.flags[0] = Lb.DG_STORE | Lb.DG_STATS

    def nrt(a):
        a.dg.nrt_total = 3

    def wide(a):        # 32 octets in one source: past the 24 the LDS image holds
        a.w.seg[0].nchan, a.dg.nrt_total = 256, 8
    return {
        "M8": (base, "TRUNET_ENOTSUP", top(M=8)),
        "nchan48": (base, "TRUNET_ENOTSUP", seg(nchan=48)),
        "pos_div2": (base, "TRUNET_ENOTSUP", seg(pos_div=2)),
        "a_mode_none": (base, "TRUNET_ENOTSUP", top(a_mode=Lb.PRO_NONE)),
        "M128_K192": (("m128k192", "ordinary", 64, 33, 3), "TRUNET_ENOTSUP", lambda a: None),
        "octets25": (base, "TRUNET_ENOTSUP", seg(nchan=200)),
        "octets32": (("m16", "ordinary", 64, 33, 3), "TRUNET_ENOTSUP", wide),
        "stats_without_mask": (base, "TRUNET_EINVAL", flags),
        "nrt_total": (base, "TRUNET_EINVAL", nrt),
    }[name]


@pytest.mark.parametrize("name", ["M8", "nchan48", "pos_div2", "a_mode_none", "M128_K192", "octets25", "octets32",
                                  "stats_without_mask", "nrt_total"])
def test_refusals_leave_every_output_untouched(name):
    from tinyrecurrentunet_amd import _lib as Lb
    case, code, change = _refusal(name)
    c = PC.inputs(case)
    a, b = PC.pw_bwd_args(c)
    change(a)
    bufs = [b.wimg, b.bimg] + b.outs + [p for p in b.parts if p is not None]
    before = [t.clone() for t in bufs]
    rc = Lb.lib().trunet_bf16_pw_bwd(a, Lb.stream())
    torch.cuda.synchronize()
    assert rc == getattr(Lb, code), (name, rc)
    for t, t0 in zip(bufs, before):
        as_int = lambda v: v.view(torch.int16 if v.dtype == torch.bfloat16 else torch.int32)
        assert torch.equal(as_int(t), as_int(t0)), "%s: a refused call wrote to an output" % name
