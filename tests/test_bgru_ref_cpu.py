"""tests/bgru_ref.py without a GPU: the octet maps are bf16_gru.hip's, the fp32 restatement stored round-to-nearest-even
passes the interval comparison at every case of the GPU tables, and the comparison has teeth -- structural mutants of the
recurrence, of the rounding and of the octet plumbing, passed through it in the kernels' place, are rejected in every regime
that can see them."""
import functools

import pytest
import torch

import bgru_cases as C
import bgru_ref as B
import gru_cases as G
import gru_ref as R

H = B.H


# ---------------------------------------------------------------------------------------------- layout and rounding
def test_octet_maps_are_the_kernels_index_arithmetic():
    """every tensor map against an explicit loop over bf16_gru.hip's own index expressions: gi / dgi octet
    24 d + 8 g + u / 8, hout / dhout / dghn octet 8 d + u / 8, gates octet 32 d + 8 k + u / 8; element (octet, pos, n, u % 8)"""
    L, NP = 3, 5
    g = G._gen("octets")
    gi, hout = B.rne(G._randn(g, 6 * H, L, NP)), B.rne(G._randn(g, 2 * H, L, NP))
    gates = B.rne(G._randn(g, 2, 4, H, L, NP))
    gi16, hout16, gates16 = B.pack("gi", gi), B.pack("hout", hout), B.pack("gates", gates)
    assert gi16.shape == (48, L, NP, 8) and hout16.shape == (16, L, NP, 8) and gates16.shape == (64, L, NP, 8)
    assert gi16.dtype == torch.bfloat16 and gi16.is_contiguous()
    flat = lambda t: t.float().reshape(-1)
    at = lambda oct_, pos, n, u: ((oct_ * L + pos) * NP + n) * 8 + u % 8
    fg, fh, fs = flat(gi16), flat(hout16), flat(gates16)
    for d in range(2):
        for u in range(0, H, 7):
            for pos in range(L):
                for n in range(NP):
                    for k in range(3):
                        assert fg[at(24 * d + 8 * k + u // 8, pos, n, u)] == gi[d * 3 * H + k * H + u, pos, n]
                    for k in range(4):
                        assert fs[at(32 * d + 8 * k + u // 8, pos, n, u)] == gates[d, k, u, pos, n]
                    assert fh[at(8 * d + u // 8, pos, n, u)] == hout[d * H + u, pos, n]
    assert torch.equal(B.unpack("gi", gi16), gi) and torch.equal(B.unpack("gates", gates16), gates)
    for name in ("dgi", "dhout", "dghn"):
        src = gi if name == "dgi" else hout
        assert torch.equal(B.pack(name, src), B.pack("gi" if name == "dgi" else "hout", src))


def test_rounding_helpers():
    x = torch.tensor([1.0, 1.00390625, 1.01171875, 1.0 + 2.0 ** -8 + 2.0 ** -20, -1.00390625 - 2.0 ** -20])
    # ties go to the even mantissa: 1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6
    assert B.rne(x).tolist() == [1.0, 1.0, 1.015625, 1.0078125, -1.0078125]
    assert B.trunc(x).tolist() == [1.0, 1.0, 1.0078125, 1.0, -1.0]
    assert B.representable(B.rne(x)) and B.representable(B.trunc(x)) and not B.representable(x)
    t = torch.arange(128.0).repeat(2, 1)
    s = B.swap_frames(t)
    assert s[0, 32].item() == 1 and s[0, 1].item() == 2 and s[1, 64 + 33].item() == 64 + 3
    assert torch.equal(s.sort(-1).values, t)


def test_interval_is_the_fp32_pins_bound_rounded_outward():
    """B is gru_ref.bound; lo / hi are bf16 values, contain rne(y) for every fp32 y with |y - ref64| <= B, and exclude the
    next bf16 value beyond rne(ref64 -+ B)"""
    g = G._gen("interval")
    r64 = G._randn(g, 4096).double() * 3
    r32 = (r64 + 1e-7 * G._randn(g, 4096).double()).float()
    lo, hi, bnd, e32 = B.interval(r64, r32)
    assert (e32, bnd) == R.bound(r64, r32)[:2] and bnd == 4 * e32 + 2e-6 * float(r64.abs().max())
    assert B.representable(lo) and B.representable(hi) and bool((lo <= hi).all())
    for y in ((r64 - bnd).float(), (r64 + bnd).float(), r64.float(), r32):
        assert B.outside(B.rne(y), lo, hi) == 0.0
    ulp = lambda v: torch.maximum(v.abs(), torch.tensor(2.0 ** -126)) * 2.0 ** -7        # at least one bf16 step
    assert B.outside(hi + ulp(hi), lo, hi) == 1.0 and B.outside(lo - ulp(lo), lo, hi) == 1.0
    zero = torch.zeros(4, dtype=torch.float64)
    assert B.inside(torch.tensor([0.0, -0.0, 0.0, -0.0]), zero, zero.float(), "zeros")[2] == 1.0
    with pytest.raises(AssertionError):
        B.inside(torch.tensor([0.0, float("nan"), 0.0, 0.0]), zero, zero.float(), "nan")
    assert (R.close(r32, r64, r32, "close")[1:3]) == (e32, bnd)


# ---------------------------------------------------------------------------------------------- the stand-in passes
@pytest.mark.parametrize("case", C.CASES + [("long", 17, 128)], ids=lambda c: "-".join(str(v) for v in c))
def test_the_fp32_restatement_stored_rne_is_inside_every_interval(case):
    """forward, backward on the reference state and backward on the stand-in's own forward, at every case of the GPU
    table, through the same case functions the GPU tests call"""
    out = C.run_cases([case], fwd=B.standin_fwd, bwd=B.standin_bwd)
    assert len(out["sums"]["%s,%d,%d" % case]) == 6


# ---------------------------------------------------------------------------------------------- mutants
ALL = tuple(G.REGIMES)
# mutant -> regimes in which the interval comparison must reject it (in the others it must pass: the table is exact)
MUTANTS = {
    "bhn_outside": ALL,
    "dzp_ht": ALL,
    "rev_forwards": ALL,
    "no_carry": tuple(r for r in ALL if r != "no_recurrence"),
    "dghn_dnp": ALL,
    "swap_u4": ALL,
    "truncation": ALL,
    "h_rounded": ALL,
    "dgh_rounded": tuple(r for r in ALL if r not in ("overflow", "no_recurrence")),
    "swap_frames": ALL,
    "swap_n_gh": ALL,
    "dir1_octet0": ALL,
}


@functools.lru_cache(maxsize=None)
def _case(regime):
    c = C.case(regime, 16, 128)
    c.iso = B.bwd_refs(c.dhout, c.state, c.whh)
    return c


def _shares(c, mut):
    """{tensor: share of elements outside the interval} with the mutant in the kernels' place: forward, and backward on
    the reference state"""
    rnd = B.trunc if mut == "truncation" else B.rne
    m = None if mut == "truncation" else mut
    out = {}
    for name, got, r64, r32 in (B.fwd_items(B.standin_fwd(c.gi, c.whh, c.bhh, m, rnd), c)
                                + B.bwd_items(B.standin_bwd(c.dhout, c.state, c.whh, m, rnd), *c.iso)):
        lo, hi = B.interval(r64, r32)[:2]
        out[name] = B.outside(got, lo, hi)
    return out


@pytest.mark.parametrize("regime", ALL)
@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_interval_rejects_mutants_of_the_stand_in(mut, regime):
    """A subtly wrong kernel would fail.  Besides the six FGRU mutants of gru_ref (seen where tests/test_gru_ref_cpu.py says):
      truncation    stored values cut instead of rounded to nearest even: every regime
      h_rounded     the forward carries the ROUNDED h into the next step: every regime (`no recurrence` through z h alone)
      dgh_rounded   the backward rounds dgh in front of the carry product: not `no recurrence` (the product is zero), and
                    not reliably `overflow`, where nearly every gate derivative that feeds the product has vanished (4e-5
                    of dgi leave their interval: below the 0.1 % that counts as seen here)
      swap_frames   frames 2 c + e <-> c + 32 e inside every block of 64 (gru.hip's column map for bf16_gru.hip's)
      swap_n_gh     the n and gh planes in each other's place
      dir1_octet0   direction 1 of gi read from octet 0
    Seen means: at least 0.1 % of the elements of at least one tensor leave their interval (bgru_ref.inside fails on a
    single one).  The table is exact: in a regime that is not listed less than 0.1 % do, and where W_hh = 0 none."""
    assert mut in MUTANTS and (mut in R.MUTANTS + R.BF16_MUTANTS or mut in ("truncation", "swap_frames", "swap_n_gh",
                                                                            "dir1_octet0"))
    shares = _shares(_case(regime), mut)
    if regime in MUTANTS[mut]:
        assert max(shares.values()) >= 1e-3, (mut, regime, shares)
    else:
        assert max(shares.values()) < 1e-3, (mut, regime, shares)
        if regime == "no_recurrence":
            assert max(shares.values()) == 0.0, (mut, regime, shares)


def test_every_listed_mutant_is_in_the_table():
    assert set(MUTANTS) >= {"bhn_outside", "dzp_ht", "rev_forwards", "no_carry", "dghn_dnp", "swap_u4"}
    assert set(R.BF16_MUTANTS) <= set(MUTANTS)
