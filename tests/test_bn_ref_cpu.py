"""tests/bn_ref.py is right (against torch autograd through relu(batch_norm) and conv1d in double), the comparison of
tests/test_bn_chain_gpu.py accepts the restatement in every case of its list and has teeth (each mutant is rejected exactly
where it computes other numbers), and the input conditions the GPU test relies on hold -- without a GPU."""
import pytest
import torch
import torch.nn.functional as F

import bn_cases as G
import bn_ref as R

f64 = torch.float64


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ---------------------------------------------------------------------------------------------- 1. independent reference
@pytest.mark.parametrize("regime", ["ordinary", "offset"])
def test_chain_restatement_matches_autograd_in_double(regime):
    """finalize_fwd -> relu_bwd_stats -> finalize_bwd -> dz = ca dy + cb z + cc, ALL in double (partials unrounded), is
    torch autograd through relu(F.batch_norm(z, training = True)) to 1e-12: dz, dgamma, dbeta, and the running statistics
    after one and after two steps.  The channel with a negative weight is part of it."""
    c = G.chain_inputs((5, 13, 384, 130, regime))
    N = c.N
    zl, dyl = c.z[:, :, :N].double(), c.dy[:, :, :N].double()
    rows = zl.reshape(c.C, -1)
    pf = torch.stack([rows.sum(1), (rows ** 2).sum(1)], -1)[None]                     # one part, double
    f = R.finalize_fwd(pf, c.count, c.gamma, c.beta, G.EPS, 0.1, torch.zeros(c.C), torch.ones(c.C))
    r = R.relu_bwd_stats(c.dy, c.z, f["scale"], f["shift"], f["mean"], N)
    b = R.finalize_bwd(r["parts"], c.count, c.gamma, f["mean"], f["rstd"])
    col = lambda v: v[:, None, None]
    dz = col(b["ca"]) * r["dy"][:, :, :N] + col(b["cb"]) * zl + col(b["cc"])
    ncl = lambda t: t[:, :, :N].permute(2, 0, 1).contiguous()
    a1 = G.bn_relu_autograd(ncl(c.z), c.gamma, c.beta, ncl(c.dy), f64)
    assert _rel(dz, a1[0].permute(1, 2, 0)) < 1e-12
    assert _rel(b["dgamma"], a1[1]) < 1e-12 and _rel(b["dbeta"], a1[2]) < 1e-12
    assert _rel(f["running_mean"], a1[3]) < 1e-12 and _rel(f["running_var"], a1[4]) < 1e-12
    f2 = R.finalize_fwd(pf, c.count, c.gamma, c.beta, G.EPS, 0.1, f["running_mean"], f["running_var"])
    a2 = G.bn_relu_autograd(ncl(c.z), c.gamma, c.beta, ncl(c.dy), f64, steps=2)
    assert _rel(f2["running_mean"], a2[3]) < 1e-12 and _rel(f2["running_var"], a2[4]) < 1e-12
    assert f["nbt_inc"] == 1 and bool((r["dy"][:, :, N:] == 0).all())
    # the sums the middle stage hands over are those of the masked cotangent
    assert _rel(r["s1"], r["dy"].sum((1, 2))) < 1e-12
    assert _rel(r["s2"], (r["dy"][:, :, :N] * (zl - col(f["mean"]))).sum((1, 2))) < 1e-12
    assert torch.equal(r["dy"][:, :, :N], torch.where(col(f["scale"]) * zl + col(f["shift"]) > 0, dyl, torch.zeros((), dtype=f64)))


def test_the_other_restatements_in_double():
    """conv_first's explicit (ci, k) chain is F.conv1d(padding = S // 2) + ReLU; eval_affine is F.batch_norm in eval mode;
    the affine copy is the same on (N, C, L); reduce_partials and sumsq are sums"""
    for case in ((3, 5, 2, 19, 128), (4, 5, 1, 12, 128), (4, 64, 2, 257, 128)):
        c = G.cf_inputs(case)
        assert _rel(R.conv_first(c.x, c.w, c.b, c.S, f64, "seq"), c.ref64) < 1e-12
        assert c.ref64.shape == (c.Cout, c.Lout, c.NP) and bool((c.ref64 == 0).any()) and bool((c.ref64 > 0).any())
    c = G.eval_inputs(129)
    x = torch.randn(7, 129, 3, dtype=f64)
    want = F.batch_norm(x, c.rm.double(), c.rv.double(), c.gamma.double(), c.beta.double(), False, 0.1, R.f32(G.EPS))
    assert _rel(c.ref64["scale"][None, :, None] * x + c.ref64["shift"][None, :, None], want) < 1e-12
    c = G.ffl_inputs((77, 5, 13, 1))
    want = torch.relu(c.scale.double()[None, :, None] * c.x[:, :, :77].double().permute(2, 0, 1) + c.shift.double()[None, :, None])
    assert torch.equal(c.ref64, want)
    c = G.rp_inputs((65, 17, 1))
    assert _rel(c.ref64, c.out0.double() + c.parts.double().sum(0)) < 1e-12
    assert _rel(R.sumsq(torch.arange(5.0)), torch.tensor(30.0, dtype=f64)) == 0


# ---------------------------------------------------------------------------------------------- 2. count = 1
def test_count_one_is_checked_against_the_restatement_alone():
    """count == 1 can only be checked against the restatement: torch refuses a training batch with one value per channel
    (asserted here).  The contract: mean = the value, biased variance 0 (clamped, never negative), rstd = 1 / sqrt(eps),
    and running_var takes the BIASED variance -- count / (count - 1) is not formed."""
    with pytest.raises(ValueError):
        F.batch_norm(torch.ones(1, 3, 1), torch.zeros(3), torch.ones(3), None, None, True, 0.1, 1e-5)
    v = torch.tensor([0.7, -3.0, 0.0])
    p = torch.stack([v, v * v], -1)[None]
    r = R.finalize_fwd(p, 1.0, torch.ones(3), torch.zeros(3), G.EPS, 0.1, torch.zeros(3), torch.ones(3))
    assert torch.equal(r["mean"], v.double()) and bool((r["var"] >= 0).all()) and bool((r["var"] < 1e-15).all())
    assert _rel(r["rstd"], torch.full((3,), R.f32(G.EPS) ** -0.5, dtype=f64)) < 1e-9
    assert bool(torch.isfinite(r["running_var"]).all()) and _rel(r["running_var"], torch.full((3,), 1 - R.f32(0.1), dtype=f64)) < 1e-9
    b = R.finalize_bwd(p, 1.0, torch.ones(3), r["mean"], r["rstd"])
    assert all(bool(torch.isfinite(t).all()) for t in b.values())


# ---------------------------------------------------------------------------------------------- 3. mutants
def _relu_masks_differ(c, other):
    """does another mask than the contract's pick other live elements with a non-zero cotangent?"""
    N = c.N
    z = c.z[:, :, :N].double()
    pre = z if c.sc is None else c.sc.double()[:, None, None] * z + c.sh.double()[:, None, None]
    alt = {"mask_ge": pre >= 0, "mask_raw": z > 0}[other]
    return bool(((alt != (pre > 0)) & (c.dy[:, :, :N] != 0)).any())


FAMILIES = {
    "fin_fwd": (G.FIN_CASES, G.fin_inputs, G.fin_fwd_emul, G.judge_fin_fwd),
    "fin_bwd": (G.FIN_BWD_CASES, G.fin_inputs, G.fin_bwd_emul, G.judge_fin_bwd),
    "reg": (G.REG_CASES, G.reg_inputs, G.reg_emul, G.judge_reg),
    "eval": (G.EVAL_C, G.eval_inputs, G.eval_emul, G.judge_eval),
    "relu": (G.RELU_CASES, G.relu_inputs, G.relu_emul, G.judge_relu),
    "ffl": (G.FFL_CASES, G.ffl_inputs, G.ffl_emul, G.judge_ffl),
    "cf": ([c for c in G.CF_CASES if c[4] == 128], G.cf_inputs, G.cf_emul, G.judge_cf),
    "rp": (G.RP_CASES, G.rp_inputs, G.rp_emul, G.judge_rp),
    "sq": (G.SQ_CASES, G.sq_inputs, G.sq_emul, G.judge_sq),
    "chain": (G.CHAIN_CASES, G.chain_inputs, G.chain_emul, G.judge_chain),
    "chain_ill": (G.CHAIN_ILL[:1], G.chain_inputs, G.chain_emul, G.judge_chain_ill),
}
# mutant -> family -> is it visible in this case (c = the case's inputs)?
VISIBLE = {
    "mask_ge": {"relu": lambda c: _relu_masks_differ(c, "mask_ge")},                   # needs a pre that is exactly 0
    "mask_raw": {"relu": lambda c: c.mode == "bn" and _relu_masks_differ(c, "mask_raw")},
    "count_pad": {"relu": lambda c: c.mode == "bn" and c.N < c.NP},                    # the sums alone; dy stays masked
    "no_mean": {"relu": lambda c: c.mode == "bn"},
    # count = 1: both variances are equal; count = 2^24 + 3: they differ by 6e-8 relative, inside ONE fp32 rounding
    "var_unbiased": {"fin_fwd": lambda c: c.count == 13.0 * 130.0, "reg": lambda c: True},
    "cc_sign": {"fin_bwd": lambda c: True},                                            # every channel has mean != 0
    "cb_no_rstd": {"fin_bwd": lambda c: True},
    "pad_k2": {"cf": lambda c: True},                                                  # S // 2 is 0 or 1, never K // 2 = 2
    "clip_last_tap": {"cf": lambda c: True},                                           # every shape's last position reads row Lin - 1
    "chan_div": {"ffl": lambda c: True},                                               # C >= 3 and the scales differ
    # running_var alone: needs running statistics and a count at which count / (count - 1) exceeds the fp32 roundings
    "running_var_biased": {"fin_fwd": lambda c: c.running and c.count == 13.0 * 130.0},
    "drop_parts_256": {"fin_fwd": lambda c: c.nparts > 256, "fin_bwd": lambda c: c.nparts > 256, "rp": lambda c: c.nparts > 256},
}


def test_every_mutant_has_a_table_entry():
    assert set(VISIBLE) == set(R.MUTANTS)


@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_the_comparison_accepts_the_restatement_in_every_gpu_case(fam):
    """the judge_* functions of the GPU test, fed with what a kernel that follows the contract returns (the double formula
    rounded once; the blocked fp32 order for the summing kernels), pass in every case of the GPU list"""
    cases, inputs, emul, judge = FAMILIES[fam]
    for case in cases:
        c = inputs(case)
        assert G.rejected(judge, c, emul(c)) == [], (fam, case)


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_the_comparison_rejects_mutants_where_they_are_visible(mut):
    """A subtly wrong kernel would fail: each mutant, passed through the GPU test's own comparison in place of kernel
    output, is REJECTED in every case of the GPU list in which it computes other numbers and ACCEPTED in every other:
      mask_ge         >= for >: only where a pre is exactly 0 (the channels with shift 0 and planted z = 0)
      mask_raw        [z > 0] for [sc z + sh > 0]: BatchNorm mode, wherever the two masks differ
      count_pad       frames >= N enter the sums (they hold NaN): BatchNorm mode with N < NP
      no_mean         sum dy z for sum dy (z - mean): BatchNorm mode
      var_unbiased    biased and unbiased variance swapped: count = 1690 only (equal at 1, inside a rounding at 2^24 + 3)
      cc_sign         cc = -g r m1 - g r^2 m2 mean: wherever mean != 0 -- in a block with mean ~ 0 it cancels
      cb_no_rstd      cb = -g r m2
      pad_k2          the first conv pads K // 2
      clip_last_tap   the first conv never reads row Lin - 1
      chan_div        the affine copy takes its channel as r // (L + 1)
      drop_parts_256  partial rows >= 256 ignored: nparts = 257, 600
      running_var_biased   running_var from the biased variance at count > 1, everything else right: running statistics
                      non-NULL at count = 1690 (at 2^24 + 3 the factor count / (count - 1) is inside one fp32 rounding)"""
    seen = 0
    for fam, vis in VISIBLE[mut].items():
        cases, inputs, emul, judge = FAMILIES[fam]
        for case in cases:
            c = inputs(case)
            bad = G.rejected(judge, c, emul(c, mut))
            if vis(c):
                assert bad, "%s passes in %s %s" % (mut, fam, case)
                seen += 1
            else:
                assert bad == [], (mut, fam, case, bad)
    assert seen > 0, mut


# ---------------------------------------------------------------------------------------------- 4. conditions
@pytest.mark.parametrize("case", G.RELU_CASES, ids=G.relu_id)
def test_relu_cases_have_no_mask_flips_and_the_edges_they_claim(case):
    """min |sc z + sh| >= 1e-3 over the channels with sc != 0 apart from the planted exact zeros; the fp32 and the fp64
    restatement agree on every element of the masked dy (asserted when the case is built); N covers 0 .. 3 mod 4 and NP;
    the planted zeros are live; padding frames hold NaN and come out as 0 with finite sums"""
    c = G.relu_inputs(case)
    assert c.min_pre >= 1e-3
    assert torch.equal(c.ref64["dy"].float(), c.blk["dy"]) and torch.equal(c.blk["dy"], c.seq["dy"])
    assert c.C == 1 or c.n_zero > 0
    assert bool(torch.isnan(c.dy[:, :, c.N:]).all()) and bool(torch.isnan(c.z[:, :, c.N:]).all())
    assert all(bool(torch.isfinite(c.ref64[k]).all()) for k in ("dy", "s1", "s2", "parts"))
    live = c.ref64["dy"][:, :, :c.N] != 0
    assert case[:4] == (5, 1, 128, 127) or c.C == 1 or 0.2 < float(live.double().mean()) < 0.8


def test_relu_shapes_cover_the_sweep_edges():
    assert sorted({s[3] % 4 for s in G.RELU_SHAPES}) == [0, 1, 2, 3] and any(s[2] == s[3] for s in G.RELU_SHAPES)
    assert sorted({s[1] * s[2] // 128 for s in G.RELU_SHAPES}) == [1, 32, 39, 129, 514]


@pytest.mark.parametrize("case", G.REG_CASES)
def test_conditioning_bound_is_met_with_margin_by_the_reference_emulation(case):
    """the emulated finalize (double formula on fp32 partial sums) stays below 0.5 of Bv = U (sum|p_sumsq| + 2 |mean|
    sum|p_sum|) / count against float64 of the data, in every channel -- the ill-conditioned one (|mean| / std = 100)
    included; the constant channel's variance is in [0, Bv] and its rstd is finite"""
    c = G.reg_inputs(case)
    r = R.finalize_fwd(c.pf, c.count, c.gamma, c.beta, G.EPS, 0.1)
    used = (r["var"] - c.var64).abs() / c.Bv
    print("used of Bv:", " ".join("%s %.2f" % kv for kv in zip(G.REG_CH, used.tolist())))
    assert bool((used < 0.5).all()), used
    assert bool(((r["mean"] - c.mean64).abs() < 0.5 * c.Bm).all())
    ratio = c.mean64.abs() / c.var64.sqrt().clamp_min(1e-30)
    assert 4.5 < float(ratio[1]) < 5.5 and 95 < float(ratio[2]) < 105 and float(ratio[0]) < 0.2
    assert 0.0 <= float(r["var"][3]) <= float(c.Bv[3]) and float(c.var64[3]) < 1e-12 and bool(torch.isfinite(r["rstd"]).all())
    # unclamped, the same partials can give a negative variance: the clamp is what keeps rstd at or below 1 / sqrt(eps)
    assert bool((r["rstd"] <= R.f32(G.EPS) ** -0.5 * (1 + 1e-12)).all())


def test_ill_conditioned_chain_is_further_from_fp64_than_torch_fp32_but_inside_its_bound():
    """the design limit the suite records: with the variance formed as sumsq / count - mean^2 from fp32 partial sums, the
    emulated dz at |mean| / std = 100 is tens of times further from float64 autograd than torch's own fp32 BatchNorm
    (which centres the data first), and inside the conditioning bound; at |mean| / std <= 5 the ratio is below 2"""
    out = {}
    for regime in ("ordinary", "offset", "ill"):
        c = G.chain_inputs((5, 13, 384, 130, regime))
        got = G.chain_emul(c)
        err = float((got["dz"].double() - c.ref64["dz"]).abs().max())
        e_y = float((c.yard["dz"].double() - c.ref64["dz"]).abs().max())
        out[regime] = err / e_y
        cond = float(((got["dz"].double() - c.ref64["dz"]).abs() / c.cond["dz"]).max())
        print("%s: |mean|/std %.1f  dz error %.2e  torch fp32 %.2e  ratio %.1f  of the conditioning bound %.2f" %
              (regime, c.ratio, err, e_y, out[regime], cond))
        if regime == "ill":
            assert cond < 0.5
    # the emulation gives about 407 at this shape (DESIGN.md quotes it): > 50 notices if the regime stopped being
    # ill-conditioned.  The < 2 holds for THIS shape, (5, 13, 384, 130); on the GPU the (64, 16, 256, 255) offset case
    # measured 3.1 times torch's fp32 error, which is why the GPU test holds ordinary and offset to close's c = 4, not to 2
    assert out["ordinary"] < 2 and out["offset"] < 2 and out["ill"] > 50, out
