"""tests/gru_ref.py is right (against torch.nn.GRU in double) and its comparison has teeth (mutants of the fp32
restatement are rejected) -- without a GPU."""
import functools

import pytest
import torch

import gru_cases as G
import gru_ref as R


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _g(seed):
    gen = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)


def test_fgru_reference_matches_nn_gru_in_double():
    """H = 64 bidirectional.  nn.GRU gets W_ih = (I | 0) / (0 | I) and b_ih = 0, so its input IS gi and an autograd leaf:
    hout, dgi = x.grad, and -- through b_hn.grad = sum dghn and W_hh.grad = sum_t dg_t h_{t-1}^T -- dghn."""
    H, L, N = 64, 7, 5
    rnd = _g(1)
    whh, bhh = rnd(2, 3 * H, H) * 0.3, rnd(2, 3 * H) * 0.1
    gi, cot = rnd(6 * H, L, N) * 2, rnd(2 * H, L, N)
    gru = torch.nn.GRU(6 * H, H, batch_first=True, bidirectional=True).double()
    eye = torch.eye(3 * H, dtype=torch.float64)
    zero = torch.zeros(3 * H, 3 * H, dtype=torch.float64)
    with torch.no_grad():
        gru.weight_ih_l0.copy_(torch.cat((eye, zero), 1)); gru.weight_ih_l0_reverse.copy_(torch.cat((zero, eye), 1))
        gru.bias_ih_l0.zero_(); gru.bias_ih_l0_reverse.zero_()
        gru.weight_hh_l0.copy_(whh[0]); gru.weight_hh_l0_reverse.copy_(whh[1])
        gru.bias_hh_l0.copy_(bhh[0]); gru.bias_hh_l0_reverse.copy_(bhh[1])
    x = gi.permute(2, 1, 0).contiguous().requires_grad_(True)          # (N, L, 6H)
    out, _ = gru(x)
    (out * cot.permute(2, 1, 0)).sum().backward()
    hout, gates = R.fgru_fwd(gi, whh, bhh)
    assert _rel(hout, out.detach().permute(2, 1, 0)) < 1e-12
    dgi, dghn = R.fgru_bwd(cot, hout, gates, whh)
    assert _rel(dgi, x.grad.permute(2, 1, 0)) < 1e-12
    for d, (w, b) in enumerate(((gru.weight_hh_l0, gru.bias_hh_l0), (gru.weight_hh_l0_reverse, gru.bias_hh_l0_reverse))):
        dg = torch.cat((dgi[d * 3 * H:d * 3 * H + 2 * H], dghn[d * H:(d + 1) * H]))        # dgh = (drp, dzp, dnp r)
        hd = hout[d * H:(d + 1) * H]
        prev = torch.zeros_like(hd)
        if d == 0:
            prev[:, 1:] = hd[:, :-1]
        else:
            prev[:, :-1] = hd[:, 1:]
        assert _rel(dg.sum((1, 2)), b.grad) < 1e-12
        assert _rel(torch.einsum("mln,kln->mk", dg, prev), w.grad) < 1e-12


def test_tgru_and_cell_reference_match_nn_gru_in_double():
    """H = 128 unidirectional, S < SP: the cotangent of nn.GRU is zero at the padded sequences, the reference's own dhs
    holds NaN there."""
    H, T, SP, S = 128, 6, 8, 5
    rnd = _g(2)
    whh, bhn = rnd(3 * H, H) * 0.3, rnd(H) * 0.1
    gi, cot = rnd(3 * H, T, SP) * 2, rnd(H, T + 1, SP)
    gru = torch.nn.GRU(3 * H, H, batch_first=True).double()
    with torch.no_grad():
        gru.weight_ih_l0.copy_(torch.eye(3 * H, dtype=torch.float64)); gru.bias_ih_l0.zero_()
        gru.weight_hh_l0.copy_(whh)
        gru.bias_hh_l0.zero_(); gru.bias_hh_l0[2 * H:].copy_(bhn)      # gi_all carries the other biases
    x = gi.permute(2, 1, 0).contiguous().requires_grad_(True)          # (SP, T, 3H)
    out, _ = gru(x)
    live = (torch.arange(SP) < S).double()
    (out * (cot[:, 1:] * live).permute(2, 1, 0)).sum().backward()
    hs, gates = R.tgru_fwd(gi, whh, bhn)
    assert bool((hs[:, 0] == 0).all()) and _rel(hs[:, 1:], out.detach().permute(2, 1, 0)) < 1e-12
    dhs = cot.clone()
    dhs[:, :, S:] = float("nan")
    dgi, dgh = R.tgru_bwd(dhs, hs, gates, whh, S)
    assert _rel(dgi, x.grad.permute(2, 1, 0)) < 1e-12
    assert bool((dgi[:, :, S:] == 0).all()) and bool((dgh[:, :, S:] == 0).all())
    assert _rel(dgh.sum((1, 2))[2 * H:], gru.bias_hh_l0.grad[2 * H:]) < 1e-12
    assert _rel(torch.einsum("mts,kts->mk", dgh, hs[:, :T]), gru.weight_hh_l0.grad) < 1e-12
    # one step of the same recurrence from full pre-activations
    t = 3
    gh = whh @ hs[:, t]
    gh[2 * H:] += bhn[:, None]
    hn, gt = R.gru_cell(gi[:, t], gh, hs[:, t])
    assert _rel(hn, hs[:, t + 1]) < 1e-14 and _rel(gt, gates[:, :, t]) < 1e-14


# ---------------------------------------------------------------------------------------------- mutants
def _fgru_L(regime):
    return 33 if regime == "long" else 16


@functools.lru_cache(maxsize=None)
def _fgru(regime):
    return G.fgru_refs(G.fgru_inputs(regime, _fgru_L(regime), 16))


@functools.lru_cache(maxsize=None)
def _tgru(regime):
    return G.tgru_refs(G.tgru_inputs(regime, 41 if regime == "long" else 9, 16, 11))


def _items(family, c, mut=None):
    """(name, candidate, ref64, ref32) of every compared tensor: the candidate is the fp32 restatement (forward, and
    backward on its own forward), with ONE deliberate error when mut is given"""
    f32 = torch.float32
    if family == "fgru":
        fw = R.fgru_fwd(c.gi, c.whh, c.bhh, f32, mut)
        bw = R.fgru_bwd(c.dhout, *c.f32, c.whh, f32, mut)
        names, gax = ("hout", "dgi", "dghn"), 1
    else:
        fw = R.tgru_fwd(c.gi, c.whh, c.bhn, f32, mut)
        bw = R.tgru_bwd(c.dhs_nan, *c.f32, c.whh, c.S, f32, mut)
        names, gax = ("hs", "dgi_all", "dgh_all"), 0
    items = [(names[0], fw[0], c.f64[0], c.f32[0])]
    items += [(G.GATE_NAMES[k], fw[1].select(gax, k), c.f64[1].select(gax, k), c.f32[1].select(gax, k)) for k in range(4)]
    items += [(names[1], bw[0], c.pair64[0], c.pair32[0]), (names[2], bw[1], c.pair64[1], c.pair32[1])]
    return items


def _rejected(items):
    out = []
    for name, got, r64, r32 in items:
        try:
            R.close(got, r64, r32, name)
        except AssertionError:
            out.append(name)
    return out


ALL = tuple(G.REGIMES)
RECURRENT = tuple(r for r in ALL if r != "no_recurrence")      # W_hh = 0 hides every error in a product with W_hh
# mutant -> (families it exists in, regimes in which `close` must reject it)
MUTANTS = {
    "bhn_outside": (("fgru", "tgru"), ALL),
    "dzp_ht": (("fgru", "tgru"), ALL),
    "rev_forwards": (("fgru",), ALL),
    "no_carry": (("fgru", "tgru"), RECURRENT),
    "dghn_dnp": (("fgru", "tgru"), ALL),
    "swap_u4": (("fgru", "tgru"), ALL),
    "k_half": (("tgru",), RECURRENT),
    "hs_off": (("tgru",), ALL),
}


@pytest.mark.parametrize("regime", ALL)
@pytest.mark.parametrize("family", ["fgru", "tgru"])
def test_close_accepts_the_fp32_restatement(family, regime):
    """the unmutated fp32 restatement is its own yardstick: 0 <= bound in every regime, and everything is finite (the
    overflow regime included)"""
    c = _fgru(regime) if family == "fgru" else _tgru(regime)
    assert _rejected(_items(family, c)) == []


@pytest.mark.parametrize("regime", ALL)
@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_close_rejects_mutants_of_the_fp32_restatement(mut, regime):
    """A subtly wrong kernel would fail: each structural error, passed through `close` in place of kernel output, is
    rejected in every regime listed with it in MUTANTS.  Which regime sees which mutant:
      bhn_outside   b_hn added outside r ( ): every regime (b_hn = 0.1 N(0,1), r < 1), through n and h
      dzp_ht        h_t for h_{t-1} in dzp: every regime, through dgi
      rev_forwards  direction 1 walked forwards: every regime (the reverse half of hout sits at mirrored positions), FGRU
      no_carry      W_hh^T dgh dropped: every regime with W_hh != 0; `no recurrence` cannot see it (the term is zero)
      dghn_dnp      dgh_n = dnp instead of dnp r: every regime, through dghn / dgh_all alone (dgi is unaffected)
      swap_u4       units u and u + 4 swapped (the MFMA C-layout row map): every regime, `no recurrence` included, where
                    nothing but the row map distinguishes units
      k_half        one K half of the TGRU product dropped: every regime with W_hh != 0, TGRU
      hs_off        h_t stored at position t instead of t + 1 (and read from there in dzp): every regime, TGRU
    Where W_hh = 0 the two W_hh mutants compute the same numbers as the restatement and must be ACCEPTED (asserted too:
    the table is exact, not a lower bound)."""
    families, regimes = MUTANTS[mut]
    assert mut in R.MUTANTS
    for family in families:
        c = _fgru(regime) if family == "fgru" else _tgru(regime)
        bad = _rejected(_items(family, c, mut))
        if regime in regimes:
            assert bad, "%s %s in the %s regime passes close" % (family, mut, regime)
        else:
            assert bad == [], (family, mut, regime, bad)
