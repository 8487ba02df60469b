"""trunet_pw_bwd (the six pw_bwd_kernel instances of csrc/pw_bwd.hip, each on the fp32 MFMA and on the three-term bf16 split)
and trunet_conv_wgrad on its own (conv_wgrad_kernel<true / false>, the four instances of csrc/wgrad_small.hip), through the C
ABI, against the float64 restatement of tests/pwbwd_ref.py.  Every output goes through convt_ref.close with the fp32
restatement as the yardstick, every element compared; `exact` cases must give the restatement's bits as well (the condition is
proven on the reference alone in tests/test_pwbwd_ref_cpu.py).  Every launch runs as the engine launches it: an image stride
larger than the weight, the weight slot and the bias row inside larger buffers between sentinels, NaN where the launch must
write, live random values in the frames >= N of every input (tests/pwbwd_cases.py has the case table, the instance each
signature reaches and the tile geometry).

Out of scope: the vector-ALU kernel behind TRUNET_PWB_THIN_VALU=1 and the two-waves-per-row-tile schedule behind
TRUNET_PWB_KSPLIT=0 -- both switches are read once per process, so a test inside this process cannot reach them -- and the
32-bit row offset limit of the epilogue, whose refusal needs tensors of 2^31 bytes."""
import functools

import pytest
import torch

import pwbwd_cases as PC
import pwbwd_ref as R

pytestmark = pytest.mark.gpu

NS = PC.NS
MODES = [pytest.param(True, id="x3"), pytest.param(False, id="f32mfma")]


@pytest.mark.parametrize("x3", MODES)
@pytest.mark.parametrize("case", PC.SMALL, ids=PC.case_id)
def test_fused_backward_small_cases(case, x3):
    PC.check_case(PC.small(case), x3)


@functools.lru_cache(maxsize=2)
def _large(case):
    """inputs and references of a mid / big case, computed on the GPU in float64 / fp32 once for both MFMA modes
    (yardstick: the blocked order alone, the tighter choice)"""
    return PC.refs(PC.inputs(case, "cuda"), seq=False, dev="cuda")


@pytest.mark.parametrize("x3", MODES)
@pytest.mark.parametrize("case", PC.MID + PC.BIG, ids=PC.case_id)
def test_fused_backward_many_tiles_per_workgroup(case, x3):
    """NB, NB + 1 and >= 2 NB + 1 tiles per workgroup, runs that start mid-position and cross into the next one"""
    _, o = PC.check_case(_large(case), x3)
    assert bool(o.own.all())


STAT_CASES = [("enc128", "ordinary", 384, 130, 2), ("dec_pad", "ordinary", 128, 97, 3), ("bn64", "exact", 384, 130, 2),
              ("gru_b", "ordinary", 384, 64, 2)]


@pytest.mark.parametrize("x3", MODES)
@pytest.mark.parametrize("case", STAT_CASES, ids=PC.case_id)
def test_prezeroed_statistics_rows_give_the_same_bits(case, x3):
    """TRUNET_DG_PREZERO on zeroed rows and no flag on NaN-prefilled rows: identical bits in every output"""
    c = PC.small(case)
    PC.same_bits(PC.gpu_pw_bwd(c, x3), PC.gpu_pw_bwd(c, x3, prezero=True), "prezero " + PC.case_id(case))


@pytest.mark.parametrize("x3", MODES)
@pytest.mark.parametrize("case", STAT_CASES + [("plain128", "ordinary", PC.MID_NP, PC.MID_N, 4)], ids=PC.case_id)
def test_two_launches_give_the_same_bits_and_the_bias_rows_are_optional(case, x3):
    c = PC.small(case) if PC.is_small(case) else PC.inputs(case, "cuda")
    o1, o2, o3 = PC.gpu_pw_bwd(c, x3), PC.gpu_pw_bwd(c, x3), PC.gpu_pw_bwd(c, x3, bias=False)
    PC.same_bits(o1, o2, "second launch " + PC.case_id(case))
    PC.same_bits(o1, o3, "b_partials = NULL " + PC.case_id(case), skip=("bimg",))


def _embed(c, NP, at, fill):
    """the case's frames at [at, at + c.NP) of an NP-frame launch (N = NP: every frame live); the other columns hold
    `fill` times seeded random values"""
    g = torch.Generator().manual_seed(at + NP)

    def wide(t):
        w = fill * torch.randn(t.shape[0], t.shape[1], NP, generator=g)
        w[:, :, at:at + c.NP] = t
        return w
    big = PC.to_device(c, "cpu")
    big.NP, big.N = NP, NP
    big.dy, big.z = wide(c.dy), wide(c.z)
    for s, sb in zip(c.segs, big.segs):
        sb.x, sb.prev = wide(s.x), wide(s.prev)
    return big


@pytest.mark.parametrize("x3", MODES)
@pytest.mark.parametrize("sig", ["enc128", "plain64", "dec_crop", "bn64", "thin8"])
def test_data_gradient_columns_do_not_see_their_neighbours(sig, x3):
    """the data gradient has no cross-frame term: a 128-frame case embedded at frame 128 (other tiles, other workgroups) of a
    384-frame launch whose other columns hold zeros, then values times 100, gives the stand-alone launch's out[s] columns
    bit for bit"""
    c = PC.inputs((sig, "ordinary", 128, 128, 3))
    alone = PC.gpu_pw_bwd(c, x3)
    for fill in (0.0, 100.0):
        o = PC.gpu_pw_bwd(_embed(c, 384, 128, fill), x3)
        for i in range(len(c.segs)):
            assert not bool(torch.isnan(o.out[i]).any())
            assert torch.equal(o.out[i][:, :, 128:256].contiguous().view(torch.int32), alone.out[i].view(torch.int32)), \
                "%s fill %g: out[%d] columns depend on their neighbours" % (sig, fill, i)


@pytest.mark.parametrize("case,two", PC.WGRAD_CASES, ids=lambda v: PC.case_id(v) if isinstance(v, tuple) else ("two" if v else "plain"))
def test_weight_gradient_entry_point_on_its_own(case, two):
    """trunet_conv_wgrad: conv_wgrad_kernel<true / false> at a pointwise signature, over the five taps of a stride-2
    transposed conv and with 192 rows; the four wgrad_small.hip instances, the two behind NP % 256 != 0 included (the case
    table of tests/pwbwd_cases.py says which launch reaches which)"""
    PC.check_wgrad(PC.small(case) if PC.is_small(case) else PC.inputs(case, "cuda"), two)


def test_segments_are_built_like_the_engines():
    """the Seg blocks of the launch helper against engine.Act.seg on the same tensors, field by field"""
    from tinyrecurrentunet_amd import _lib as Lb
    from tinyrecurrentunet_amd.engine import Act
    c = PC.inputs(("dec_pad", "ordinary", 128, 97, 3))
    keep = ([], {})
    for s, left in zip(c.segs, (1, 0)):
        x = s.x.cuda()
        mine = PC._seg(Lb, s, x, keep)
        k = keep[1].get(id(s.c0))
        bn = NS(scale=k["c0"], shift=k["c1"]) if s.bn else None
        theirs = Act(x, s.nchan, s.L, bn).seg(pos_off=-left, woff=s.woff)
        for name, _ in Lb.Seg._fields_:
            assert getattr(mine, name) == getattr(theirs, name), name


def _refusal(name):
    """(case, expected code name, what to change in the valid argument block)"""
    from tinyrecurrentunet_amd import _lib as Lb
    base = ("bn64", "ordinary", 128, 97, 3)

    def seg(**kw):
        def f(a, b):
            for k, v in kw.items():
                setattr(a.w.seg[0], k, v)
        return f

    def top(**kw):
        def f(a, b):
            for k, v in kw.items():
                setattr(a.w, k, v)
        return f

    def flags(fl):
        def f(a, b):
            a.dg[0].flags = fl
        return f

    def zmask(a, b):        # a tensor of the same shape that is not the segment's src0
        other = torch.zeros_like(b.xs[0])
        b.keep[0].append(other)
        a.dg[0].zmask = Lb.ptr(other)
    none = lambda a, b: None
    sig = lambda s: (s, "ordinary", 128, 97, 3)
    return {
        "zmask_not_src0": (base, "TRUNET_ENOTSUP", zmask),
        "nchan48": (base, "TRUNET_ENOTSUP", seg(nchan=48)),
        "pos_div2": (base, "TRUNET_ENOTSUP", seg(pos_div=2)),
        "a_mode_none": (base, "TRUNET_ENOTSUP", top(a_mode=Lb.PRO_NONE)),
        "M160": (sig("m160"), "TRUNET_ENOTSUP", none),
        "row_tiles3": (sig("k96"), "TRUNET_ENOTSUP", none),
        "row_tiles5": (sig("k160"), "TRUNET_ENOTSUP", none),
        "row_tiles8": (sig("k256"), "TRUNET_ENOTSUP", none),
        "M8_two_row_tiles": (sig("m8k64"), "TRUNET_ENOTSUP", none),
        "M128_six_row_tiles": (sig("m128k192"), "TRUNET_ENOTSUP", none),
        "stats_on_row_tile4": (sig("stats_tile4"), "TRUNET_ENOTSUP", none),
        "accum_without_mask": (sig("plain128"), "TRUNET_ENOTSUP", flags(Lb.DG_STORE | Lb.DG_ACCUM)),
        "stats_without_mask": (base, "TRUNET_EINVAL", flags(Lb.DG_STORE | Lb.DG_STATS)),
    }[name]


@pytest.mark.parametrize("name", ["zmask_not_src0", "nchan48", "pos_div2", "a_mode_none", "M160", "row_tiles3", "row_tiles5",
                                  "row_tiles8", "M8_two_row_tiles", "M128_six_row_tiles", "stats_on_row_tile4",
                                  "accum_without_mask", "stats_without_mask"])
def test_refusals_leave_every_output_untouched(name):
    """every argument block stays inside the allocated buffers even if the call wrongly launched"""
    from tinyrecurrentunet_amd import _lib as Lb
    case, code, change = _refusal(name)
    c = PC.inputs(case)
    a, b = PC.pw_bwd_args(c)
    change(a, b)
    bufs = [b.wimg, b.bimg] + b.outs + [p for p in b.parts if p is not None]
    before = [t.clone() for t in bufs]
    rc = Lb.lib().trunet_pw_bwd(a, Lb.stream())
    torch.cuda.synchronize()
    assert rc == getattr(Lb, code), (name, rc)
    for t, t0 in zip(bufs, before):
        assert torch.equal(t.view(torch.int32), t0.view(torch.int32)), "%s: a refused call wrote to an output" % name
