"""trunet_bf16_gemm (bgemm_kernel in csrc/bf16.hip) and the two weight packers on their own, through the C ABI, against the
float64 restatement of tests/bgemm_ref.py.  `ordinary` and `zero` cases go through convt_ref.close with the fp32 emulation
as the yardstick; `exact` cases must give the restatement's bits (the condition is proven on the reference alone in
tests/test_bgemm_ref_cpu.py).  Every launch writes into NaN-prefilled buffers inside a guard frame the test owns (two guard
octets behind the 16 a launch may have, one position before and behind the tensor): whatever lies outside the rows and
positions the launch owns must come back bit for bit.  Every case asserts the template instance it reaches."""
import ctypes

import pytest
import torch

import bgemm_cases as PC
import bgemm_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", PC.not_m96(PC.SMALL), ids=PC.case_id)
def test_small_cases(case):
    PC.check_case(PC.small(case))


@pytest.mark.parametrize("case", PC.only_m96(PC.SMALL), ids=PC.case_id)
def test_96_rows_take_the_guarded_instance(case):
    """three row tiles: the second wave of a split tile owns ONE.  The FULL instances gave it two -- A fragments past the
    LDS image, stores to octets 12 .. 15 of a 12-octet tensor, which the guard frame here would catch"""
    PC.check_case(PC.small(case))


@pytest.mark.parametrize("case", PC.WRAP, ids=PC.case_id)
def test_second_trip_of_the_tile_loop(case):
    """just over one sweep of the tile slots: some waves own two tiles (statistics over both), most one; the references are
    computed on the GPU in float64 / fp32 (yardstick: the blocked and permuted orders, the tighter choice)"""
    c = PC.refs(PC.inputs(case), seq=False, dev="cuda")
    PC.check_case(c)


STAT_CASES = [("dec_pad", "ordinary", 192, 130, 3), ("dg128_KSA", "exact", 64, 33, 3)]


@pytest.mark.parametrize("case", STAT_CASES, ids=PC.case_id)
def test_prezeroed_partials_give_the_same_bits(case):
    """TRUNET_EPI_PREZERO on zeroed partials and no flag on NaN-prefilled ones: identical bits in every output"""
    c = PC.small(case)
    PC.same_bits(PC.gpu_gemm(c), PC.gpu_gemm(c, prezero=True), "prezero " + PC.case_id(case))


@pytest.mark.parametrize("case", STAT_CASES + [("gru_proj", "ordinary", 192, 130, 3), ("m72", "ordinary", 192, 130, 3),
                                               ("pw64", "ordinary", 44032, 43990, 3)], ids=PC.case_id)
def test_two_launches_give_the_same_bits(case):
    c = PC.small(case) if PC.is_small(case) else PC.inputs(case)
    PC.same_bits(PC.gpu_gemm(c), PC.gpu_gemm(c), "second launch " + PC.case_id(case))


def test_both_packers_write_the_image_of_pack_image():
    """every signature's image (every chunk of the GRU projection) from trunet_bf16_pack_weight and from ONE
    trunet_bf16_pack_weights_batch launch over all of them (max_elems from the largest): bitwise pack_image; the batch
    launch writes nothing behind an image shorter than the largest"""
    from tinyrecurrentunet_amd import _lib as Lb
    items = []
    for sig in PC.SIGS:
        c = PC.inputs((sig, "ordinary", 64, 33, 3))
        c.W = PC.master_weight(c)
        assert float((R.bf16_round(c.W) != c.W).float().mean()) > 0.9
        W = c.W.cuda()
        items += [(c, W, c.w_m_off + off) for off in c.chunks]
    batch = PC.pack_batch(Lb, items)
    sizes = {PC.image_elems(c) for c, _, _ in items}
    assert len(sizes) > 4
    for (c, W, off), img in zip(items, batch):
        want = R.pack_image(c.W, c.M, c.ldw_m, c.ldw_c, off, PC.seg_list(c)).reshape(-1)
        one, _ = PC.pack_single(Lb, c, W, off)
        torch.cuda.synchronize()
        assert torch.equal(PC.bits(one.cpu()), want), "%s: trunet_bf16_pack_weight differs from pack_image" % c.sig
        img = img.cpu()
        assert torch.equal(PC.bits(img[:-PC.PART_GUARD]), want), "%s: trunet_bf16_pack_weights_batch differs from pack_image" % c.sig
        assert bool((img[-PC.PART_GUARD:] == PC.SENT).all()), "%s: the batched launch wrote behind the image" % c.sig


def test_every_instance_of_the_dispatch_is_reached():
    """the plan of every signature (host only) is the instance the signature was written for, and together they are all
    instances trunet_bf16_gemm has"""
    reached = {}
    for sig in PC.SIGS:
        c = PC.inputs((sig, "ordinary", 64, 33, 3))
        a, _ = PC.gemm_args(c, c.chunks[-1])
        reached[sig] = PC.plan(a)
        assert reached[sig] == c.inst, (sig, reached[sig], c.inst)
    got = set(reached.values())
    for inst in sorted(PC.INSTANCES):
        print("bgemm_kernel<%d, %d, %d, %s>: %s" % (inst[:3] + ("true" if inst[3] else "false",
                                                               ", ".join(s for s, i in reached.items() if i == inst) or "NOT REACHED")))
    assert got == PC.INSTANCES, "instances not reached: %s; unknown: %s" % (PC.INSTANCES - got, got - PC.INSTANCES)


def _refusal(name):
    """(expected code name, what to change in the valid argument block of dec_pad)"""
    from tinyrecurrentunet_amd import _lib as Lb

    def top(**kw):
        def f(a):
            for k, v in kw.items():
                setattr(a, k, v)
        return f

    def mixed(a):
        a.seg[1].mode = Lb.PRO_BNBWD
        a.seg[1].src1, a.seg[1].c0, a.seg[1].c1, a.seg[1].c2 = a.seg[0].src0, a.seg[0].c0, a.seg[0].c0, a.seg[0].c0

    def f32_stats(a):
        a.epi = PC.B | PC.F | PC.S

    def past(a):
        a.out_pos_off += 3           # p_begin + P + out_pos_off = out_L + 1
    return {"M129": ("TRUNET_ENOTSUP", top(M=129, M_stat=129)), "nks25": ("TRUNET_ENOTSUP", top(nks_total=25)),
            "mixed_bnbwd": ("TRUNET_ENOTSUP", mixed), "f32out_stats": ("TRUNET_EINVAL", f32_stats),
            "window_past_out_L": ("TRUNET_EINVAL", past), "window_before_0": ("TRUNET_EINVAL", top(out_pos_off=-1))}[name]


@pytest.mark.parametrize("name", ["M129", "nks25", "mixed_bnbwd", "f32out_stats", "window_past_out_L", "window_before_0"])
def test_refusals_leave_every_output_untouched(name):
    from tinyrecurrentunet_amd import _lib as Lb
    code, change = _refusal(name)
    c = PC.inputs(("dec_pad", "ordinary", 64, 33, 3))
    a, b = PC.gemm_args(c)
    change(a)
    before = [b.out.clone(), b.part.clone()]
    v = [ctypes.c_int(-9) for _ in range(4)]
    assert Lb.lib().trunet_bf16_gemm_plan(a, *[ctypes.byref(x) for x in v]) == getattr(Lb, code), name
    assert [x.value for x in v] == [-9] * 4
    rc = Lb.lib().trunet_bf16_gemm(a, Lb.stream())
    torch.cuda.synchronize()
    assert rc == getattr(Lb, code), (name, rc)
    for t, t0 in zip([b.out, b.part], before):
        assert torch.equal(PC.bits(t), PC.bits(t0)), "%s: a refused call wrote to an output" % name
