"""tests/bgemm_ref.py and the case list of tests/bgemm_cases.py on their own, without a GPU: the restatement equals torch's
conv1d / conv_transpose1d / autograd of the layers it stands for, the `exact` regime is exact in fp32 in every summation
order (the condition that lets tests/test_bgemm_gpu.py demand equal bits), float64 and the kernel's fp32 fma agree on every
mask bit, the tile geometry the list promises is in it, pack_image round-trips against bf16(W), every mutant of the
restatement is rejected by a listed small case and every ordinary case accepts the `permuted` fp32 result as "got"."""
import pytest
import torch
import torch.nn.functional as Fn

import bgemm_cases as PC
import bgemm_ref as R

D = torch.float64


def _double(c):
    """the case with every operand in float64 (no bf16 anywhere: bf16 = False below)"""
    for s in c.segs:
        s.x = s.x.double()
    return c


def test_restatement_is_conv_transpose1d_of_the_tap_segments():
    """ConvTranspose1d(64 -> 64, k, s, padding s / 2) of relu(c0 x + c1): the launch's window is the P positions in the middle
    of an output of out_L = P + 2, whose first and last position the launch must leave alone"""
    for sig, Kt, S_ in (("convt_k3s1", 3, 1), ("convt_k5s2", 5, 2), ("convt_k3s2", 3, 2)):
        c = _double(PC.inputs((sig, "ordinary", 64, 33, 5)))
        Lin = c.segs[0].L
        for s in c.segs[1:]:
            s.x, s.c0, s.c1 = c.segs[0].x, c.segs[0].c0, c.segs[0].c1           # one source tensor under every tap
        act = torch.relu(c.segs[0].c0.double()[:, None, None] * c.segs[0].x + c.segs[0].c1.double()[:, None, None])
        W = c.W[:64 * 64 * Kt].double().view(64, 64, Kt)                        # [ci][co][k]
        want = Fn.conv_transpose1d(act.permute(2, 0, 1), W, c.b.double(), stride=S_, padding=S_ // 2).permute(1, 2, 0)
        got = R.bgemm(c, D, bf16=False)["out"]
        assert want.shape[1] >= c.P and Lin == (c.P + S_ - 1) // S_
        assert float((got[:, 1:1 + c.P] - want[:, :c.P]).abs().max()) < 1e-12
        assert torch.equal(got[:, 0], c.old[:, 0].double()) and torch.equal(got[:, -1], c.old[:, -1].double())


def test_restatement_is_the_strided_first_conv_and_the_padded_concat():
    c = _double(PC.inputs(("first", "ordinary", 64, 33, 3)))
    for s in c.segs[1:]:
        s.x = c.segs[0].x
    W = c.W[:64 * 20].double().view(64, 4, 5)
    want = torch.relu(Fn.conv1d(c.segs[0].x.permute(2, 0, 1), W, c.b.double(), stride=2, padding=1)).permute(1, 2, 0)
    got = R.bgemm(c, D, bf16=False)["out"]
    assert want.shape[1] == c.P and float((got - want).abs().max()) < 1e-12
    # decoder pointwise conv over cat(F.pad(x1, (1, 0)), skip): the first source shifted by one position
    c = _double(PC.inputs(("dec_pad", "ordinary", 64, 33, 3)))
    s0, s1 = c.segs
    a0 = torch.relu(s0.c0.double()[:, None, None] * s0.x + s0.c1.double()[:, None, None])
    cat = torch.cat([Fn.pad(a0.transpose(1, 2), (1, 0)).transpose(1, 2), s1.x])           # [192][P][NP]
    want = Fn.conv1d(cat.permute(2, 0, 1), c.W[:64 * 192].double().view(64, 192, 1), c.b.double()).permute(1, 2, 0)
    got = R.bgemm(c, D, bf16=False)
    assert float((got["out"] - want).abs().max()) < 1e-12
    live = want[:, :, :c.N]
    assert float((got["st0"] - live.sum((1, 2))).abs().max()) < 1e-9
    assert float((got["st1"] - (live * live).sum((1, 2))).abs().max()) < 1e-9


def test_restatement_is_autograd_of_a_pointwise_layer_behind_a_relu():
    """dg128_KSA: out = [e0 zmask + e1 > 0] (W[:, 64:]^T dz + old), dz = ca dy + cb z + cc, statistics against zmask - e2"""
    c = PC.inputs(("dg128_KSA", "ordinary", 64, 33, 3))
    s = c.segs[0]
    dz = (s.c0.double()[:, None, None] * s.x.double() + s.c1.double()[:, None, None] * s.z.double() + s.c2.double()[:, None, None])
    W = c.W[:64 * 192].double().view(64, 192)
    src = torch.randn(128, 3, 64, dtype=D, requires_grad=True)
    y = torch.einsum("mc,cpn->mpn", W[:, 64:], src)
    g, = torch.autograd.grad((y * dz).sum(), src)
    keep = (c.e0.double()[:, None, None] * c.zmask.double() + c.e1.double()[:, None, None]) > 0
    want = torch.where(keep, g + c.old.double(), torch.zeros((), dtype=D))
    got = R.bgemm(c, D, bf16=False)
    assert float((got["out"] - want).abs().max()) < 1e-12
    live = want[:, :, :c.N]
    cen = c.zmask.double()[:, :, :c.N] - c.e2.double()[:, None, None]
    assert float((got["st0"] - live.sum((1, 2))).abs().max()) < 1e-9
    assert float((got["st1"] - (live * cen).sum((1, 2))).abs().max()) < 1e-9


def test_gru_projection_chunks_make_one_384_row_product():
    c = _double(PC.inputs(("gru_proj", "ordinary", 64, 33, 3)))
    s = c.segs[0]
    act = torch.relu(s.c0.double()[:, None, None] * s.x + s.c1.double()[:, None, None])
    want = torch.einsum("mc,cpn->mpn", c.W[:384 * 128].double().view(384, 128), act) + c.b.double()[:, None, None]
    assert float((R.bgemm(c, D, bf16=False)["out"] - want).abs().max()) < 1e-12


def _ties(val):
    """(rounded up, rounded down) counts of the bf16 ties among val (float64 values that fp32 holds exactly)"""
    r = R.bf16_round(val)
    ulp = 2.0 ** (torch.floor(torch.log2(val.abs().clamp_min(2.0 ** -60))) - 7)
    tie = (val != 0) & (torch.remainder(val / ulp, 1.0) == 0.5)
    return int((tie & (r.abs() > val.abs())).sum()), int((tie & (r.abs() < val.abs())).sum())


@pytest.mark.parametrize("case", PC.EXACT, ids=PC.case_id)
def test_exact_regime_is_exact_in_fp32_in_every_order(case):
    """every value a row's chain can meet is a multiple of the row unit and the sum of the terms' magnitudes -- the largest
    partial sum any order can meet -- stays below 2^24 units: fp32 holds every partial sum exactly.  Then, directly: fp32 in
    three orders == float64, bit for bit, rows and (where their own budget holds) statistics."""
    c = PC.inputs(case)
    ref = R.bgemm(c, D, bf16=True)
    raw = R.bgemm(c, D, bf16=True, mut="stats_from_unrounded")           # the same rows; nothing else differs
    mags = R.bgemm(c, D, bf16=True, absval=True)
    win = R.window(c)
    unit = PC.row_unit(c)
    q = ref["out"][:, win] / unit
    assert torch.equal(q, q.round()), "rows are not on their grid"
    assert torch.equal(raw["out"], ref["out"])
    count = float(mags["out"][:, win].abs().max()) / unit
    print("%s out: largest sum of magnitudes %.0f units of 2^24 = 16777216" % (PC.case_id(case), count))
    assert count < 2 ** 24
    PC.refs(c)
    for k in c.exact_stats:
        print("%s %s: sum of magnitudes %.0f units; bitwise: %s" % (PC.case_id(case), k, float(mags[k].max()) / PC.stat_unit(c, k),
                                                                     c.exact_stats[k]))
        qs = ref[k] / PC.stat_unit(c, k)
        assert torch.equal(qs, qs.round())
    for order in R.ORDERS:
        got = R.bgemm(c, torch.float32, order, bf16=True)
        assert torch.equal(got["out"].double(), ref["out"]), "fp32 %s differs from float64 in the rows" % order
        for k, ok in c.exact_stats.items():
            if ok:
                assert torch.equal(got[k].double(), ref[k]), "fp32 %s differs from float64 in %s" % (order, k)


def test_exact_regime_meets_bf16_ties_in_both_directions():
    """the stored rows of the exact cases need more than 8 bits and hit ties that round up and ties that round down, in the
    forward, the data-gradient and the plain signatures; the BatchNorm-backward prologue's own rounding meets both as well"""
    for sig in ("enc128", "dec_pad", "convt_k5s2", "dg128_KSA", "plain_KS64", "nks24", "m72"):
        c = PC.inputs((sig, "exact", 192, 130, 2))
        before = R.bgemm(c, D, bf16=True, raw=True)
        val = before["raw"]
        up, down = _ties(val[:c.M, R.window(c)])
        moved = float((R.bf16_round(val) != val).double().mean())
        print("%s: %d ties up, %d ties down, %.1f %% of the rows move when rounded" % (sig, up, down, 100 * moved))
        assert up > 10 and down > 10, (sig, up, down, moved)
        assert torch.equal(R.bf16_round(val), before["out"])
    s = PC.inputs(("dg128_KS", "exact", 192, 130, 2)).segs[0]
    dz = s.c0.double()[:, None, None] * s.x.double() + s.c1.double()[:, None, None] * s.z.double() + s.c2.double()[:, None, None]
    up, down = _ties(dz)
    assert up > 10 and down > 10


@pytest.mark.parametrize("case", [c for c in PC.SMALL if c[1] != "exact" and PC.SIGS[c[0]].epi & PC.K and c[2:] == (192, 130, 3 - (c[1] == "zero"))],
                         ids=PC.case_id)
def test_mask_sign_is_the_same_in_float64_and_in_the_fp32_fma(case):
    """fmaf(e0, z, e1) is correctly rounded: its sign is the sign of the exact value.  e0 z is exact in float64 for a bf16 z
    (24 + 8 bits), so the float64 sum is correctly rounded as well and rounding to fp32 keeps sign and zero."""
    c = PC.inputs(case)
    assert torch.equal(R.bf16_round(c.zmask), c.zmask) and c.e0.dtype == c.e1.dtype == torch.float32
    pre64 = c.e0.double()[:, None, None] * c.zmask[:c.M].double() + c.e1.double()[:, None, None]
    prod, e1 = c.e0.double()[:, None, None] * c.zmask[:c.M].double(), c.e1.double()[:, None, None].expand_as(pre64)
    bb = pre64 - prod
    err = (prod - (pre64 - bb)) + (e1 - bb)                     # TwoSum: pre64 + err is the exact value
    assert bool((err[pre64 == 0] == 0).all()) and bool((err.abs() <= pre64.abs() * 2.0 ** -52).all())
    assert torch.equal(pre64 > 0, pre64.float() > 0) and torch.equal(pre64 == 0, pre64.float() == 0)
    assert bool((pre64 == 0).any()) and bool((pre64 > 0).any()) and bool((pre64 < 0).any())
    if c.regime == "zero":                                      # the known subset: every third frame of one row
        assert bool((pre64[PC.EDGE_CH % c.M, :, ::3] == 0).all())


def test_case_list_holds_the_tile_geometry_it_promises():
    for case in PC.SMALL:
        assert set(PC.tiles_owned(case[0], case[2], case[4]).tolist()) <= {0, 1}
    for case in PC.WRAP:
        own = PC.tiles_owned(case[0], case[2], case[4])
        total, n = case[4] * (case[2] // 64), PC.GRID * PC.tslots(case[0])
        assert set(own.tolist()) == {1, 2} and n < total < n + 64 and total % n, (case, total, n)
        assert int(own.sum()) == total and 0 < int((own == 2).sum()) < n // 8
    assert len(PC.WRAP) == 4
    assert [PC.tslots(c[0]) for c in PC.WRAP] == [4, 4, 2, 4] and [PC.SIGS[c[0]].inst[0] for c in PC.WRAP] == [2, 4, 2, 2]
    P5 = [c for c in PC.WRAP if c[4] == 5]
    # stride 2048 = 409 chunks of 5 positions + 3: a slot's second tile lies in another chunk at another position
    assert len(P5) == 1 and (PC.GRID * 4) % 5 != 0
    assert {(c[2], c[3]) for c in PC.ORDINARY_SMALL} == set(PC.SMALL_NPN)
    for sig in PC.SIGS:
        for NP, N in PC.SMALL_NPN:
            assert sum(1 for c in PC.ORDINARY_SMALL if c[0] == sig and (c[2], c[3]) == (NP, N)) == 2
        assert any(c[0] == sig for c in PC.EXACT) and any(c[0] == sig for c in PC.ZERO)
    assert {s.inst for s in PC.SIGS.values()} == PC.INSTANCES
    c = PC.inputs(("dec_crop", "ordinary", 64, 33, 3))
    assert c.segs[0].L == 5 and [R.seg_q(c.segs[0], p) for p in range(3)] == [1, 2, 3]
    c = PC.inputs(("dec_pad", "ordinary", 64, 33, 3))
    assert [R.seg_q(c.segs[0], p) for p in range(3)] == [None, 0, 1]
    c = PC.inputs(("convt_k5s2", "ordinary", 64, 33, 3))
    assert [[R.seg_q(s, p) for s in c.segs] for p in range(3)] == [[None, 0, None, None, None], [1, None, 0, None, None],
                                                                    [None, 1, None, 0, None]]
    c = PC.inputs(("first", "ordinary", 64, 33, 3))
    assert [R.seg_q(s, 0) for s in c.segs] == [None, 0, 1, 2, 3] and [R.seg_q(s, 2) for s in c.segs] == [3, 4, 5, 6, None]


@pytest.mark.parametrize("sig", ["enc128", "dec_pad", "convt_k5s2", "first", "dec5_ct", "dg128_KS", "m44", "seg24", "nks24", "m72"])
def test_pack_image_round_trips_against_the_rounded_weight(sig):
    """reading the image back through the fragment layout gives bf16(W) at every (m, channel) of every segment, and zero in
    every padded element"""
    c = PC.inputs((sig, "ordinary", 64, 33, 3))
    c.W = PC.master_weight(c)
    assert float((R.bf16_round(c.W) != c.W).float().mean()) > 0.9          # an fp32 weight: the rounding is the packer's
    off = c.w_m_off + c.chunks[-1]
    img = R.pack_image(c.W, c.M, c.ldw_m, c.ldw_c, off, PC.seg_list(c)).view(torch.bfloat16).float()
    nks = sum(R.ksteps(s.nchan) for s in c.segs)
    assert img.shape == ((c.M + 31) // 32, nks, 64, 8)
    seen = torch.zeros_like(img, dtype=torch.bool)
    ks0 = 0
    for s in c.segs:
        A = R.weight(c, s, off, s.woff, torch.float32, R.bf16_round, (c.M + 7) // 8 * 8)
        for m in range(c.M):
            for ch in range(s.nchan):
                at = (m // 32, ks0 + ch // 16, 32 * ((ch % 16) // 8) + m % 32, ch % 8)
                assert img[at] == A[m, ch], (m, ch)
                seen[at] = True
        ks0 += R.ksteps(s.nchan)
    assert bool((img[~seen] == 0).all()) and int(seen.sum()) == c.M * sum(s.nchan for s in c.segs)


def _rejects(case, mut):
    """does the comparison of the GPU test reject the mutant's fp32 output on this case?"""
    c = PC.small(case)
    return PC.rejected(c, R.bgemm(c, torch.float32, "blocked", mut=mut))[1]


# the cases tried, most telling first; every one is in the GPU test's list
MUTANT_CASES = [("dg128_KSA", "exact", 64, 33, 3), ("dg64_KSA", "exact", 64, 33, 3), ("dec_pad", "exact", 64, 33, 3),
                ("convt_k5s2", "exact", 64, 33, 3), ("gru_proj", "exact", 64, 33, 3), ("m44", "exact", 64, 33, 3),
                ("m44_KS", "exact", 64, 33, 3), ("dg128_KSA", "zero", 192, 130, 2), ("dg128_KSA", "ordinary", 192, 130, 3),
                ("dec_pad", "ordinary", 192, 130, 3), ("convt_k5s2", "ordinary", 192, 130, 3), ("gru_proj", "ordinary", 64, 33, 3),
                ("dg64_KSA", "ordinary", 64, 33, 3), ("m44", "ordinary", 192, 130, 3), ("enc128", "ordinary", 192, 130, 3)]


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_every_mutant_is_rejected_by_a_listed_small_case(mut):
    assert all(c in PC.SMALL for c in MUTANT_CASES)
    caught = [(PC.case_id(case), f[0]) for case in MUTANT_CASES for f in [_rejects(case, mut)] if f]
    print("mutant %s rejected by: %s" % (mut, "; ".join("%s (%s)" % ck for ck in caught) or "NOTHING"))
    assert caught, "mutant %s passes every listed case: the case list is too weak" % mut
    by_close = [ck for ck in caught if "-exact-" not in ck[0]]
    print("mutant %s: %s" % (mut, "also rejected by `close` against the yardstick" if by_close else
                             "rejected by bit equality in the exact regime only"))


@pytest.mark.parametrize("case", [c for c in PC.SMALL if c[1] != "exact"], ids=PC.case_id)
def test_every_ordinary_case_accepts_the_permuted_emulation(case):
    """`permuted` is part of the yardstick, so this holds by construction for c >= 1; what it checks is that every case's
    reference and yardstick can be built, are finite and pass their own comparison (with the blocked order as well)"""
    c = PC.small(case)
    for order in ("permuted", "blocked"):
        res, fails = PC.rejected(c, R.bgemm(c, torch.float32, order))
        assert not fails, fails


def test_unmutated_emulation_passes_every_mutant_case():
    for case in MUTANT_CASES:
        assert not _rejects(case, None), case
