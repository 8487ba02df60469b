"""tests/convt_ref.py is right (against torch autograd through conv_transpose1d in double), its comparison accepts both
yardsticks and each fp32 order measured by the other in every case of tests/convt_cases.py, and it has teeth (structural
mutants are rejected exactly where they compute other numbers) -- without a GPU."""
import pytest
import torch
import torch.nn.functional as F

import convt_cases as G
import convt_ref as R


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("regime", ["ordinary", "signed"])
@pytest.mark.parametrize("Lin", [1, 2, 3, 5, 9])
@pytest.mark.parametrize("K,S", G.KS)
def test_restatement_matches_autograd_in_double(K, S, Lin, regime):
    """frames are the batch axis of conv_transpose1d; its input is relu(pre) of the leaf pre = s_scale src + s_shift (dsrc
    is the gradient at the source's BatchNorm OUTPUT), the cotangent of its output the hand-written BatchNorm-backward
    affine dz = ca dy + cb z + cc, zero for frames >= N (N = 97 < NP = 128): pre.grad is the masked dsrc (torch's relu has
    gradient 0 at 0, the `>` of the contract: the signed regime has a channel whose pre is exactly 0), weight.grad dW,
    bias.grad db."""
    c = G.inputs((K, S, regime, Lin, 128, 97))
    d = torch.float64
    col = lambda v: v.to(d)[None, :, None]
    src = c.src.to(d).permute(2, 0, 1).contiguous()                                 # [NP][64][Lin]
    pre = (col(c.s_scale) * src + col(c.s_shift)).requires_grad_(True)
    W = c.W.to(d).clone().requires_grad_(True)
    b = torch.zeros(R.C, dtype=d, requires_grad=True)
    out = F.conv_transpose1d(torch.relu(pre), W, b, stride=S, padding=S // 2)
    assert out.shape == (c.NP, R.C, c.Lout)
    dz = col(c.ca) * c.dy.to(d).permute(2, 0, 1) + col(c.cb) * c.z.to(d).permute(2, 0, 1) + col(c.cc)
    dz = dz * (torch.arange(c.NP) < c.N).to(d)[:, None, None]
    (out * dz).sum().backward()
    r = R.convt_bwd(c, d)
    g = pre.grad[:c.N]
    assert _rel(r["dW"], W.grad) < 1e-12 and _rel(r["db"], b.grad) < 1e-12
    assert _rel(r["dsrc"], pre.grad.permute(1, 2, 0)) < 1e-12
    assert _rel(r["st0"], g.sum((0, 2))) < 1e-12
    assert _rel(r["st1"], (g * (src[:c.N] - col(c.s_mean))).sum((0, 2))) < 1e-12
    assert bool((r["dsrc"][:, :, c.N:] == 0).all())
    if regime == "signed":
        assert bool((r["dsrc"][G.ZERO_PRE_CH] == 0).all()) and bool((r["dsrc"][G.ALWAYS_ON_CH, :, :c.N] != 0).all())


def _rejected(items):
    out = []
    for name, got, r64, yard in items:
        try:
            R.close(got, r64, yard, name)
        except AssertionError:
            out.append(name)
    return out


def _case(case, bf16):
    return G.build(case, bf16) if G.is_big(case) else G.small(case, bf16)


@pytest.mark.parametrize("case", G.F32_CASES, ids=G.case_id)
def test_close_accepts_the_fp32_orders(case):
    """every case the GPU test runs: the builder's nudge holds (asserted there: min|pre| >= 1e-3) with about half of the
    elements active; both orders of the yardstick pass `close`; and -- what checks c and f -- two plain fp32 orders pass
    `close` with the OTHER alone as yardstick, both ways: the blocked order and the same with frames and co channels
    randomly permuted.  The blocked order also passes measured by the sequential chain alone.  The converse cannot hold
    and is not asked: one chain over all q * frames terms of a dW element is up to 37 times further from fp64 than the
    blocked sum (3 x 8290 terms), which is why the chain is part of the yardstick and not judged by c."""
    c = _case(case, False)
    if c.regime in ("ordinary", "signed", "trained"):
        assert 0.4 < c.active < 0.6, c.active
    for got, yard in ((c.blk, c.yard), (c.seq, c.yard), (c.blk, c.perm), (c.perm, c.blk), (c.blk, c.seq), (c.perm, c.yard)):
        assert _rejected([(k, got[k], c.ref64[k], yard[k]) for k in R.OUTPUTS]) == []
    if c.regime == "zero_cotangent":
        assert all(bool((c.ref64[k] == 0).all()) and bool((c.yard[k] == 0).all()) for k in R.OUTPUTS)
    if c.regime == "dead_tile":
        assert all(bool((c.yard[k][32:] == 0).all()) for k in ("dW", "dsrc", "st0", "st1"))


@pytest.mark.parametrize("case", G.B16_CASES, ids=G.case_id)
def test_close_accepts_the_bf16_emulation(case):
    """the emulation is its own yardstick, finite in every case, and it is a bf16-grade result: its error against fp64 on
    the same bf16 inputs is above the fp32 restatement's and below 2^-6 of the largest value of every output"""
    c = _case(case, True)
    assert _rejected([(k, c.yard[k], c.ref64[k], c.yard[k]) for k in R.OUTPUTS]) == []
    assert bool((R.bf16_round(c.yard["dsrc"]) == c.yard["dsrc"]).all())
    if c.regime != "zero_cotangent":
        f32 = R.convt_bwd(c, torch.float32)
        for k in ("dW", "dsrc"):
            e_y, e32 = R.bound(c.ref64[k], c.yard[k])[0], R.bound(c.ref64[k], f32[k])[0]
            assert e32 < e_y < 2.0 ** -6 * float(c.ref64[k].abs().max()), (k, e32, e_y)


# ---------------------------------------------------------------------------------------------- mutants
def visible(mut, case):
    """does the mutant compute other numbers than the restatement in this case?"""
    K, S, regime, Lin, NP, N = case
    if regime == "zero_cotangent":
        return False                     # dz = 0: every output is 0 whatever the structure
    return {
        "pad0": S == 2,                  # pad = S / 2 = 0 at stride 1
        # tap K - 1 of the last position is row Lout - 1 + pad: outside at stride 2, and Lin = 1 has no other position
        "drop_last_tap": not (S == 2 and Lin == 1),
        # K = 3, S = 2, Lin = 1: Lout = 1, the centre tap is the only one
        "tap_flip": not ((K, S) == (3, 2) and Lin == 1),
        "w_transposed": True,
        "clip_last_row": True,           # row Lout - 1 is tap K - 1 - pad of the last position
        "mask_ge": regime == "signed",   # needs a pre that is exactly 0
        "mask_raw": True,
        "no_mean": True,
        "pad_frames_counted": N < NP,
        "row_swap4": True,
    }[mut]


# the outputs a mutant may be rejected on (all five where nothing is listed)
SEEN_ON = {"no_mean": {"st1"}, "row_swap4": {"dW"}, "tap_flip": {"dsrc", "st0", "st1"}, "w_transposed": {"dsrc", "st0", "st1"},
           "mask_ge": {"dsrc", "st0", "st1"}, "mask_raw": {"dsrc", "st0", "st1"}}
MUTANT_CASES = [(c, False) for c in G.F32_CASES if not G.is_big(c)] + \
               [(c, True) for c in G.B16_CASES if c[3] == G.MID_LIN and c[4:] == G.B16_MID]


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_close_rejects_mutants_where_they_are_visible(mut):
    """A subtly wrong kernel would fail: each structural error, passed through `close` in place of kernel output (the
    blocked fp32 restatement, the bf16 emulation for the bf16 cases), is REJECTED in every case in which it computes other
    numbers and ACCEPTED in every other, so the table is exact:
      pad0                 p = q S + k: stride 2 only (pad = 0 at stride 1)
      drop_last_tap        everywhere but S = 2, Lin = 1 (the last tap of the only position is outside Lout)
      tap_flip             W[:, :, K-1-k] in the data gradient: everywhere but (3, 2), Lin = 1 (one valid tap, the centre)
      w_transposed         W[co][ci] in the data gradient
      clip_last_row        p < Lout - 1
      mask_ge              pre >= 0: only where a pre is exactly 0 (`signed`: the channel with scale 0 and shift 0)
      mask_raw             src > 0 for pre > 0
      no_mean              statistics on src instead of src - s_mean: the second statistics column alone
      pad_frames_counted   dz not zeroed for frames >= N: wherever N < NP
      row_swap4            rows r and r + 4 of dW swapped (the MFMA C-layout row map): dW alone
    Nothing is visible in `zero_cotangent`.  Every small fp32 case and the mid-shape bf16 cases of every regime."""
    for case, bf16 in MUTANT_CASES:
        c = _case(case, bf16)
        m = R.convt_bwd(c, torch.float32, mut=mut, bf16=bf16)
        bad = set(_rejected([(k, m[k], c.ref64[k], c.yard[k]) for k in R.OUTPUTS]))
        if visible(mut, case):
            assert bad, "%s passes close in %s" % (mut, G.case_id(case))
            assert bad <= SEEN_ON.get(mut, set(R.OUTPUTS)), (mut, G.case_id(case), bad)
        else:
            assert bad == set(), (mut, G.case_id(case), bad)
