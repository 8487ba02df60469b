"""tests/pwbwd16_ref.py and the case list of tests/pwbwd16_cases.py on their own, without a GPU: the restatement equals
torch.autograd of the network's composition, the `exact` regime is exact in fp32 in every summation order (the condition that
lets tests/test_pwbwd16_gpu.py demand equal bits), float64 and the kernel's fp32 fma agree on every mask bit, the step
geometry the list promises is in it, and every mutant of the restatement is rejected by a listed small case."""
import pytest
import torch

import pwbwd16_cases as PC
import pwbwd16_ref as R

D = torch.float64


def _autograd_case(sig, NP, N, P):
    """the case with z = the layer's own conv output and (ca, cb, cc) = the training-mode BatchNorm backward of it, all in
    float64, and torch.autograd's gradients of sum(dy BatchNorm(z)) over the live frames"""
    c = PC.inputs((sig, "ordinary", NP, N, P))
    M = c.M
    g = torch.Generator().manual_seed(5)
    gamma, bias = torch.rand(M, generator=g, dtype=D) + 0.5, torch.randn(M, generator=g, dtype=D)
    c.W, c.dy = c.W.double().requires_grad_(), c.dy.double()
    bias.requires_grad_()
    leaves, cols = [], []
    for s in c.segs:
        x = s.x.double()
        leaf = (s.c0.double()[:, None, None] * x + s.c1.double()[:, None, None]) if s.bn else x.clone()
        leaf.requires_grad_()
        leaves.append(leaf)
        act = torch.relu(leaf) if (s.bn or s.mask) else leaf          # a masked plain source is a post-ReLU tensor
        if not s.bn:
            assert not s.mask or bool((x >= 0).all())
        # F.pad / crop: position p of the layer reads source position p + off, zero outside [0, L)
        lo, hi = max(0, -s.off), max(0, P + s.off - s.L)
        a = torch.nn.functional.pad(act[:, max(0, s.off):min(s.L, P + s.off)].transpose(1, 2), (lo, hi)).transpose(1, 2)
        assert a.shape[1] == P
        cols.append(a)
    z = torch.nn.functional.conv1d(torch.cat(cols).permute(2, 0, 1), c.W[:, :, None], bias).permute(1, 2, 0)   # [M][P][NP]
    zl = z[:, :, :N]
    mu, var = zl.mean((1, 2)), zl.var((1, 2), unbiased=False)
    r = (var + 1e-5).rsqrt()
    yhat = (zl - mu[:, None, None]) * r[:, None, None]
    loss = (c.dy[:, :, :N] * (gamma[:, None, None] * yhat)).sum()
    grads = torch.autograd.grad(loss, [c.W, bias] + leaves)
    with torch.no_grad():
        m1, m2 = c.dy[:, :, :N].mean((1, 2)), (c.dy[:, :, :N] * yhat).mean((1, 2))
        c.ca, c.cb, c.cc = gamma * r, -gamma * r * r * m2, gamma * r * (mu * r * m2 - m1)
        c.z, c.W = z.detach(), c.W.detach()
    return c, grads


@pytest.mark.parametrize("sig,NP,N,P", [("enc128", 64, 33, 3), ("dec_pad", 64, 33, 3), ("dec_crop", 64, 50, 2),
                                        ("seg3", 64, 64, 3)])
def test_restatement_is_autograd_of_the_composition(sig, NP, N, P):
    c, grads = _autograd_case(sig, NP, N, P)
    out = R.pw_bwd(c, D, bf16=False)
    rel = lambda a, b: float((a - b).norm() / (b.norm() + 1e-300))
    assert rel(out["dW"], grads[0]) < 1e-11, rel(out["dW"], grads[0])
    assert float((out["db"] - grads[1]).abs().max()) < 1e-9 * float(c.dy.abs().sum())        # sum dz: ~0 behind a BatchNorm
    for i, s in enumerate(c.segs):
        want = s.prev.double().clone()
        p0, p1, off = R.p_range(s, c.P)
        vis = slice(p0 + off, p1 + off)
        want[:, vis] = grads[2 + i][:, vis]
        if s.accum:     # the gradient the skip connection left there joins before the ReLU mask
            pv = s.prev.double()[:, vis]
            want[:, vis] += torch.where(PC.mask64(s)[:, vis], pv, torch.zeros((), dtype=D)) if s.mask else pv
        got = out["g%d" % i]
        assert rel(got, want) < 1e-11, (i, rel(got, want))
        assert bool((grads[2 + i][:, :, N:] == 0).all())
        unv = torch.ones(s.L, dtype=torch.bool)
        unv[vis] = False
        assert torch.equal(got[:, unv], s.prev.double()[:, unv]) and bool((grads[2 + i][:, unv] == 0).all())
        if s.stats:
            live = want[:, vis, :N]
            st0, st1 = live.sum((1, 2)), (live * (s.x.double()[:, vis, :N] - s.mean.double()[:, None, None])).sum((1, 2))
            assert rel(out["st0_%d" % i], st0) < 1e-11 and rel(out["st1_%d" % i], st1) < 1e-11


# units of the `exact` regime's grids: dz 2^-8, activations 2^-4, W 2^-2, prev / x / mean 2^-3
UNITS = {"dW": 2.0 ** -12, "db": 2.0 ** -8, "g": 2.0 ** -10, "st0": 2.0 ** -10, "st1": 2.0 ** -13}


EXACT_VIEWS = [(c, None) for c in PC.EXACT] + [(c, two) for c in PC.WGRAD_CASES if c[1] == "exact" for two in (True, False)]


@pytest.mark.parametrize("case,view", EXACT_VIEWS, ids=lambda v: PC.case_id(v) if isinstance(v, tuple) else str(v))
def test_exact_regime_is_exact_in_fp32_in_every_order(case, view):
    """every term of every output is a multiple of the output's unit and the sum of the terms' magnitudes -- the largest
    partial sum any order can meet -- stays below 2^24 units: fp32 (MFMA accumulators, bias sums, butterflies, the
    accumulate add) holds every partial sum exactly.  Then, directly: fp32 in three orders == float64, bit for bit."""
    c = PC.inputs(case)
    if view is not None:            # as trunet_bf16_wgrad sees the case: dz BatchNorm backward (True) or dy itself (False)
        c = PC.wgrad_view(c, view)
    ref = R.pw_bwd(c, D, bf16=True)
    mags = R.pw_bwd(c, D, bf16=True, absval=True)
    for k in R.outputs(c):
        unit = UNITS[k.split("_")[0].rstrip("0123456789") if k[0] == "g" else k.split("_")[0]]
        q = ref[k] / unit
        assert torch.equal(q, q.round()), "%s: not on its grid" % k
        if k[0] == "g":
            s = c.segs[int(k[1:])]
            p0, p1, off = R.p_range(s, c.P)
            count = float(mags[k][:, p0 + off:p1 + off].abs().max()) / unit if p1 > p0 else 0.0   # before its 8-bit rounding
        else:
            count = float(mags[k].abs().max()) / unit
        print("%s %s: largest sum of magnitudes %.0f units of 2^24 = 16777216" % (PC.case_id(case), k, count))
        assert count < 2 ** 24, "%s: %s needs %.0f units: over the fp32 budget" % (PC.case_id(case), k, count)
    for order in R.ORDERS:
        got = R.pw_bwd(c, torch.float32, order, bf16=True)
        for k in R.outputs(c):
            assert torch.equal(got[k].double(), ref[k]), "%s: fp32 %s differs from float64 in %s" % (PC.case_id(case), order, k)
    # the regime exercises what it is for: dz needs more than 8 bits, ties included; pre is exactly 0 on some frames
    dz = c.ca.double()[:, None, None] * c.dy.double() + c.cb.double()[:, None, None] * c.z.double() + c.cc.double()[:, None, None]
    moved = R.bf16_round(dz) != dz
    ulp = 2.0 ** (torch.floor(torch.log2(dz.abs().clamp_min(2.0 ** -20))) - 7)
    ties = (torch.remainder(dz / ulp, 1.0) == 0.5)
    if view is not False:
        assert float(moved.double().mean()) > 0.05 and int(ties.sum()) > 10, (float(moved.double().mean()), int(ties.sum()))
    for s in c.segs:
        if s.mask:
            pre = s.c0.double()[:, None, None] * s.x.double() + s.c1.double()[:, None, None]
            assert bool((pre == 0).any()) and bool((pre > 0).any()) and (not s.bn or bool((pre < 0).any()))


@pytest.mark.parametrize("case", [c for c in PC.SMALL if c[1] == "ordinary"], ids=PC.case_id)
def test_mask_sign_is_the_same_in_float64_and_in_the_fp32_fma(case):
    """fmaf(e0, z, e1) is correctly rounded: its sign is the sign of the exact value, and rounding never turns a non-zero
    value into zero (no underflow at these magnitudes).  e0 z is exact in float64 for a bf16 z (24 + 8 bits), so the float64
    sum is correctly rounded as well.  Every element of every masked source is compared."""
    c = PC.inputs(case)
    for s in c.segs:
        if s.mask:
            pre64 = s.c0.double()[:, None, None] * s.x.double() + s.c1.double()[:, None, None]
            assert torch.equal(R.bf16_round(s.x), s.x)          # 8-bit z: the float64 product holds all 32 bits
            assert s.c0.dtype == s.c1.dtype == torch.float32
            # TwoSum: pre64 + err is the exact value; where the double sum is 0 nothing was rounded away
            prod, c1 = s.c0.double()[:, None, None] * s.x.double(), s.c1.double()[:, None, None].expand_as(pre64)
            bb = pre64 - prod
            err = (prod - (pre64 - bb)) + (c1 - bb)
            assert bool((err[pre64 == 0] == 0).all()) and bool((err.abs() <= pre64.abs() * 2.0 ** -52).all())
            fma32 = pre64.float()
            assert torch.equal(pre64 > 0, fma32 > 0) and torch.equal(pre64 == 0, fma32 == 0)
            assert torch.equal(PC.mask64(s), fma32 > 0)


def test_case_list_holds_the_step_geometry_it_promises():
    own = {case: PC.steps_owned(case[2], case[4]) for case in PC.CASES}
    counts = lambda case: set(own[case].tolist())
    assert all(counts(c) == {0, 1} for c in PC.SMALL)                                  # total < G, one-stage start
    assert any(counts(c) == {1, 2} for c in PC.MID) and any(counts(c) == {2, 3} for c in PC.MID)
    assert any(PC.crosses_chunk(c[2], c[4]) for c in PC.MID)
    assert all(int(own[c].sum()) >= 3 * PC.G and c[4] <= 3 for c in PC.BIG) and len(PC.BIG) == 2
    assert {(c[2], c[3]) for c in PC.SMALL} >= {(64, 1), (64, 33), (192, 130)}
    assert any(c[4] == 1 for c in PC.SMALL) and any((c[3] + 63) // 64 < c[2] // 64 for c in PC.SMALL)
    for sig in PC.SIGS:                                                                # the full cross product on the small (NP, N)
        for NP, N in PC.SMALL_NPN:
            assert sum(1 for c in PC.ORDINARY_SMALL if c[0] == sig and (c[2], c[3]) == (NP, N)) == 2
        assert any(c[0] == sig for c in PC.EXACT) and any(c[0] == sig for c in PC.ZERO)
    M, srcs = PC.SIGS["dec_crop"]
    c = PC.inputs(("dec_crop", "ordinary", 64, 33, 3))
    assert R.p_range(c.segs[0], c.P)[:2] == (0, 3) and c.segs[0].L == 5 and c.segs[0].off == 1    # positions 0 and L - 1 unvisited


def _rejects(case, mut):
    """does the comparison of the GPU test reject the mutant's fp32 output on this case?"""
    c = PC.small(case)
    got = R.pw_bwd(c, torch.float32, "blocked", mut=mut)
    for k in R.outputs(c):
        if c.regime == "exact":
            if not torch.equal(got[k].double(), c.ref64[k]):
                return k
        else:
            try:
                R.close(got[k], c.ref64[k], c.yard[k], k)
            except AssertionError:
                return k
    return None


# the cases tried, most telling first; every one is in the GPU test's list
MUTANT_CASES = [("seg3", "exact", 64, 33, 3), ("enc128", "exact", 64, 33, 3), ("dec_pad", "exact", 64, 33, 3),
                ("dec_crop", "ordinary", 64, 33, 3), ("enc128", "ordinary", 192, 130, 3), ("seg3", "ordinary", 192, 130, 3),
                ("dec_pad", "ordinary", 192, 130, 3), ("plain64", "ordinary", 64, 33, 3)]


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_every_mutant_is_rejected_by_a_listed_small_case(mut):
    assert all(c in PC.SMALL for c in MUTANT_CASES)
    caught = [(PC.case_id(case), k) for case in MUTANT_CASES for k in [_rejects(case, mut)] if k]
    print("mutant %s rejected by: %s" % (mut, ", ".join("%s (%s)" % ck for ck in caught) or "NOTHING"))
    assert caught, "mutant %s passes every listed case: the case list is too weak" % mut
    by_close = [ck for ck in caught if "-ordinary-" in ck[0]]
    print("mutant %s: %s" % (mut, "also rejected by `close` against the yardstick" if by_close else
                             "rejected by bit equality in the exact regime only"))


def test_unmutated_emulation_passes_the_comparison_it_is_the_yardstick_of():
    """`permuted` is no part of the yardstick: holding it to the reference through `close` checks c and f without a GPU"""
    for case in MUTANT_CASES:
        c = PC.small(case)
        assert _rejects(case, None) is None
        if c.regime != "exact":
            perm = R.pw_bwd(c, torch.float32, "permuted")
            for k in R.outputs(c):
                R.close(perm[k], c.ref64[k], c.yard[k], "%s permuted %s" % (PC.case_id(case), k))
