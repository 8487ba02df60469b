"""tests/pwbwd_ref.py and the case list of tests/pwbwd_cases.py on their own, without a GPU: the fp32 orders of the
restatement hold each other through `close`, the `exact` regime is exact in fp32 in every summation order and under the
three-term split (the condition that lets tests/test_pwbwd_gpu.py demand equal bits), the tile geometry the list promises is
in it, every mutant of the restatement is rejected by a listed small case, and the segment arguments of the cases are the
ones engine.py passes."""
import pytest
import torch

import pwbwd_cases as PC
import pwbwd_ref as R

D = torch.float64


@pytest.mark.parametrize("case", [c for c in PC.SMALL if c[1] != "exact"], ids=PC.case_id)
def test_fp32_orders_hold_each_other(case):
    """`permuted` is no part of the yardstick: holding it (and the two orders that are) to the reference through `close`
    checks c and f on every small case without a GPU -- the second statistics column, recovered through a / c0, included"""
    c = PC.small(case)
    perm = R.pw_bwd(c, torch.float32, "permuted")
    for k in R.outputs(c):
        for name, got in (("permuted", perm), ("blocked", c.blk), ("seq", c.seq)):
            R.close(got[k], c.ref64[k], c.yard[k], "%s %s %s" % (PC.case_id(case), name, k))


# units of the `exact` regime's grids: dz 2^-8, activations 2^-4, W 2^-2, prev / x / mean 2^-3
UNITS = {"dW": 2.0 ** -12, "db": 2.0 ** -8, "g": 2.0 ** -10, "st0": 2.0 ** -10, "st1": 2.0 ** -13}
EXACT_VIEWS = [(c, None) for c in PC.EXACT] + [(c, two) for c, two in PC.WGRAD_CASES if c[1] == "exact"]


@pytest.mark.parametrize("case,view", EXACT_VIEWS, ids=lambda v: PC.case_id(v) if isinstance(v, tuple) else str(v))
def test_exact_regime_is_exact_in_fp32_in_every_order_and_under_the_split(case, view):
    """every term of every output is a multiple of the output's unit and the sum of the terms' magnitudes -- the largest
    partial sum any order can meet -- stays below 2^24 units: fp32 holds every partial sum exactly.  Then, directly: fp32 in
    three orders == float64, bit for bit.  The operands of both GEMMs (dz, the activations, W) split into hi + mid + lo
    exactly with lo == 0, so the three products x3_common.hpp drops are zero."""
    c = PC.inputs(case)
    if view is not None:
        c = PC.wgrad_view(c, view)
    ref = R.pw_bwd(c, D)
    mags = R.pw_bwd(c, D, absval=True)
    for k in R.outputs(c):
        unit = UNITS["g" if k[0] == "g" else k.split("_")[0]]
        q = ref[k] / unit
        assert torch.equal(q, q.round()), "%s: not on its grid" % k
        count = float(mags[k].abs().max()) / unit
        print("%s %s: largest sum of magnitudes %.0f units of 2^24 = 16777216" % (PC.case_id(case), k, count))
        assert count < 2 ** 24, "%s: %s needs %.0f units: over the fp32 budget" % (PC.case_id(case), k, count)
    for order in R.ORDERS:
        got = R.pw_bwd(c, torch.float32, order)
        for k in R.outputs(c):
            assert torch.equal(got[k].double(), ref[k]), "%s: fp32 %s differs from float64 in %s" % (PC.case_id(case), order, k)
    rows = slice(c.a_m_off, c.a_m_off + c.M)
    col = lambda v: v[:, None, None]
    dz = col(c.ca[rows]) * c.dy[rows] + (col(c.cb[rows]) * c.z[rows] + col(c.cc[rows])) if c.bnbwd else c.dy[rows]
    ops = [dz, c.W] + [(col(s.c0) * s.x + col(s.c1)).clamp_min(0) if s.bn else s.x for s in c.segs]
    for t in ops:
        hi, mid, lo = R.split3(t)
        assert torch.equal(hi + mid + lo, t) and torch.equal((hi.double() + mid.double() + lo.double()).float(), t)
        assert bool((lo == 0).all())
    if view is None:
        for s in c.segs:
            if s.mask:      # the regime exercises what it is for: pre is exactly 0 on some elements, > 0 and (BN) < 0 on others
                pre = col(s.c0.double()) * s.x.double() + col(s.c1.double())
                assert bool((pre == 0).any()) and bool((pre > 0).any()) and (not s.bn or bool((pre < 0).any()))


def test_every_regime_carries_the_special_channels():
    for regime in PC.REGIMES:
        c = PC.small(("enc128", regime, 384, 130, 2))
        s = c.segs[0]
        pre = s.c0.double()[:, None, None] * s.x.double() + s.c1.double()[:, None, None]
        assert s.c0[PC.ON_CH] == 0 and bool((pre[PC.ON_CH] > 0).all())
        assert s.c0[PC.OFF_CH] == 0 and bool((pre[PC.OFF_CH] < 0).all())
        assert bool((pre[PC.ZERO_CH] == 0).all())
        z = pre[PC.ZERO_AT_CH] == 0
        assert s.c0[PC.ZERO_AT_CH] != 0 and bool(z.any()) and not bool(z.all())
        assert abs(float(s.c1[PC.RATIO_CH])) > 65536 * abs(float(s.c0[PC.RATIO_CH])) > 0 and bool((pre[PC.RATIO_CH] > 0).all())
        slow = R.slow_stat_channel(s.c0, s.c1)
        assert bool(slow[[PC.ON_CH, PC.OFF_CH, PC.ZERO_CH, PC.RATIO_CH]].all()) and not bool(slow[PC.ZERO_AT_CH])
        assert bool((s.c0 < 0).any())
        p = PC.small(("thin8", regime, 384, 130, 2)).segs[1]
        assert not p.bn and bool((p.x == 0).any()) and bool((p.x >= 0).all())          # a plain post-ReLU source
        assert bool((c.dy[:, :, c.N:] != 0).any()) == (regime != "zero_cotangent")      # live padding frames
        assert bool((s.x[:, :, c.N:] != 0).any()) and bool((s.prev[:, :, c.N:] != 0).any()) and bool((c.z[:, :, c.N:] != 0).any())


def test_case_list_holds_the_tile_geometry_it_promises():
    # G workgroups, tile = (position, 32 frames), position slowest: the ranges partition [0, total)
    for NP, P in ((384, 2), (8320, 3), (16512, 5)):
        r = PC.tile_ranges(NP, P)
        assert r[0][0] == 0 and r[-1][1] == P * NP // 32 and all(r[i][1] == r[i + 1][0] for i in range(PC.G - 1))
    nbs = {s: PC.nb_of(s) for s in PC.SIGS}
    assert set(nbs.values()) == {3, 4} and nbs["enc128"] == 3 and nbs["bn64"] == 4
    # every signature: workgroups without tiles and with one, a run that starts mid-position
    for sig in PC.SIGS:
        ks = set()
        for c in PC.SMALL:
            if c[0] == sig:
                assert c[2] % 128 == 0 and c[3] <= c[2]
                ks |= PC.kinds(c[2], c[4], nbs[sig])
        assert ks >= {"0", "1", "mid_start"}, (sig, ks)
        assert {(c[2], c[3]) for c in PC.ORDINARY_SMALL if c[0] == sig} >= {(NP, N) for NP, N, _ in PC.SMALL_NPN}
        assert any(c[0] == sig for c in PC.EXACT) and any(c[0] == sig for c in PC.ZERO)
    # the mid and big cases: every instance and every NB; NB, NB + 1 and >= 2 NB + 1 tiles, runs that cross into the next
    # position, for each NB that occurs
    assert {PC.INSTANCE[c[0]] for c in PC.MID + PC.BIG} == set(PC.INSTANCE.values())
    for nb in (3, 4):
        ks = set()
        for c in PC.MID + PC.BIG:
            if nbs[c[0]] == nb:
                ks |= PC.kinds(c[2], c[4], nb)
        assert ks >= {"NB", "NB+1", ">=2NB+1", "mid_start", "crossing"}, (nb, ks)
    assert all(PC.tiles_owned(c[2], c[4]).min() >= 1 for c in PC.MID + PC.BIG)
    # frames: N ends in each of the four 32-frame tiles of a 128-frame chunk; a tile wholly beyond N; N = NP; N = 1; an NP
    # that is an odd multiple of 128
    npn = {(c[2], c[3]) for c in PC.SMALL}
    assert {((N - 1) % 128) // 32 for _, N in npn if N % 32} == {0, 1, 2, 3}
    assert any(N == NP for NP, N in npn) and any(N == 1 for NP, N in npn) and any((NP // 128) % 2 == 1 and NP > 128 for NP, N in npn)
    assert any((N + 31) // 32 < NP // 32 for NP, N in npn)
    assert (PC.MID_NP // 128) % 2 == 1 and (PC.BIG_NP // 128) % 2 == 1
    c = PC.inputs(("dec_crop", "ordinary", 128, 97, 3))
    assert R.positions(c.segs[0], c) == ([0, 1, 2], [1, 2, 3]) and c.segs[0].L == 5         # positions 0 and L - 1 unvisited
    c = PC.inputs(("dec_pad", "ordinary", 128, 97, 3))
    assert R.positions(c.segs[0], c) == ([1, 2], [0, 1]) and c.segs[0].L == 2               # p = 0 reads the F.pad zero


def test_segments_are_the_ones_the_engine_passes():
    """recorded from engine.py: the decoder's pointwise conv over [x1 | skip] passes x1.seg(pos_off=-left, woff=0) and
    skip.seg(woff=x1.C) with left = 1 for the F.pad and -1 for the crop; a ConvTranspose1d(k, stride s, padding pad) weight
    gradient passes seg(pos_off=pad - kk, woff=kk, pos_div=s) with ldw_m = k, ldw_c = Co k; the strided first conv
    seg(pos_mul=s, pos_off=kk - pad, woff=kk) with ldw_m = C k, ldw_c = k; the GRU input projection's row blocks
    (a_m_off, w_m_off, b_off, M) = (3 H d + r0, r0, r0, m) for (r0, m) in ((0, 128), (128, 3 H - 128)), H = 64"""
    f = lambda s: (s.nchan, s.L, s.pos_mul, s.pos_off, s.pos_div, s.woff, s.bn)
    P = 5
    c = PC.inputs(("dec_pad", "ordinary", 128, 97, P))
    assert [f(s) for s in c.segs] == [(64, P - 1, 1, -1, 1, 0, True), (128, P, 1, 0, 1, 64, False)] and (c.ldw_m, c.ldw_c) == (192, 1)
    c = PC.inputs(("dec_crop", "ordinary", 128, 97, P))
    assert [f(s) for s in c.segs] == [(64, P + 2, 1, 1, 1, 0, True), (128, P, 1, 0, 1, 64, False)]
    k, s_, pad = 5, 2, 1
    c = PC.inputs(("ct_taps", "ordinary", 256, 200, P))
    assert [f(s) for s in c.segs] == [(64, 2, 1, pad - kk, s_, kk, True) for kk in range(k)] and (c.ldw_m, c.ldw_c) == (k, 64 * k)
    assert P == (2 - 1) * s_ - 2 * pad + k
    c = PC.inputs(("first_taps", "ordinary", 256, 200, 3))
    assert [f(s) for s in c.segs] == [(4, 7, s_, kk - pad, 1, kk, False) for kk in range(k)] and (c.ldw_m, c.ldw_c) == (4 * k, k)
    assert 3 == (7 + 2 * pad - k) // s_ + 1
    H = 64
    blocks = [(d * 3 * H + r0, r0, r0, m) for d in (0, 1) for r0, m in ((0, 128), (128, 3 * H - 128))]
    for sig in ("gru_a", "gru_b"):
        c = PC.inputs((sig, "ordinary", 128, 97, 3))
        assert (c.a_m_off, c.w_m_off, c.b_off, c.M) in blocks and c.dy.shape[0] == 6 * H and c.ldw_m == 128
        assert c.w_numel >= 3 * H * 128


def _rejects(case, mut):
    """does the comparison of the GPU test reject the mutant's fp32 output on this case?"""
    c = PC.small(case)
    got = R.pw_bwd(c, torch.float32, "blocked", mut=mut)
    for k in R.outputs(c):
        if c.regime == "exact" and not torch.equal(got[k].double(), c.ref64[k]):
            return k
        try:
            R.close(got[k], c.ref64[k], c.yard[k], k)
        except AssertionError:
            return k
    return None


# the cases tried, most telling first; every one is in the GPU test's list
MUTANT_CASES = [("enc128", "ordinary", 384, 130, 2), ("dec_crop", "ordinary", 128, 97, 3), ("dec_pad", "ordinary", 384, 130, 2),
                ("thin8", "ordinary", 384, 130, 2), ("m96", "ordinary", 384, 130, 2), ("gru_b", "ordinary", 384, 130, 2),
                ("enc128", "exact", 384, 130, 2), ("dec_crop", "exact", 128, 97, 2)]


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_every_mutant_is_rejected_by_a_listed_small_case(mut):
    assert all(c in PC.SMALL for c in MUTANT_CASES)
    caught = [(PC.case_id(case), k) for case in MUTANT_CASES for k in [_rejects(case, mut)] if k]
    print("mutant %s rejected by: %s" % (mut, ", ".join("%s (%s)" % ck for ck in caught) or "NOTHING"))
    assert caught, "mutant %s passes every listed case: the case list is too weak" % mut
    by_close = [ck for ck in caught if "-ordinary-" in ck[0]]
    assert by_close, "mutant %s is rejected by bit equality in the exact regime only, never by `close`" % mut


def test_unmutated_restatement_passes_the_comparison_it_is_the_yardstick_of():
    for case in MUTANT_CASES:
        assert _rejects(case, None) is None
