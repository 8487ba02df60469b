"""tests/frontend_ref.py is right (against torch.stft and the formulas of oracle/features_ref.py in double), its layouts
round-trip, the comparison of tests/test_frontend_pin_gpu.py accepts both fp32 orders of the restatement in every case of
its lists and has teeth (every mutant is rejected by at least one case), and the conditions the lockstep interval relies on
hold -- without a GPU."""
import pytest
import torch

import frontend_cases as G
import frontend_ref as R
from oracle import features_ref as fr

f64 = torch.float64


def _all_feature_inputs():
    for case in G.FEAT_CASES:
        yield G.feat_inputs(case)
    for case in G.FL_EDGE_CASES:
        yield G.fl_edge_inputs(case)
    for i in range(len(G.RAGGED_CASES)):
        yield G.ragged_inputs(i, 4)


# ---------------------------------------------------------------------------------------------- 1. independent reference
def test_spectrum_and_channels_match_torch_stft_and_the_oracle_formulas_in_double():
    """every utterance of every feature case: the explicit reflect map + DFT matrix equal torch.stft(center, reflect,
    rectangular window) to 1e-12 of the frame's largest bin, and the channel formulas applied to torch.stft's own spectrum
    equal oracle/features_ref.py's (norm(amp_to_db), sin / cos of the angle) to 1e-12"""
    seen = 0
    for c in _all_feature_inputs():
        off = 0
        for x in c.xs:
            spec = torch.stft(x.double(), n_fft=512, hop_length=128, window=torch.ones(512, dtype=f64), center=True,
                              pad_mode="reflect", return_complex=True).t()                     # (T, 257)
            T = spec.shape[0]
            assert T == R.nframes(x.shape[0])
            re, im = c.ref["re"][off:off + T], c.ref["im"][off:off + T]
            scale = spec.abs().max().clamp_min(1.0)
            assert float((re - spec.real).abs().max()) <= 1e-12 * scale and float((im - spec.imag).abs().max()) <= 1e-12 * scale
            mag, nm, sn, cs = R.channels(spec.real, spec.imag, f64)
            ph = torch.angle(spec)
            assert float((nm - fr.norm(fr.amp_to_db(spec.abs()))).abs().max()) <= 1e-12
            # a bin that is exactly zero has the angle of +0 by contract; torch.stft hands some of them over as -0 + 0j,
            # whose angle is pi
            nz = spec.abs() > 0
            assert bool((sn[~nz] == 0).all()) and bool((cs[~nz] == 1).all())
            assert float(((sn - torch.sin(ph)) * nz).abs().max()) <= 1e-12 and float(((cs - torch.cos(ph)) * nz).abs().max()) <= 1e-12
            assert float((mag - spec.abs()).abs().max()) <= 1e-12 * scale
            off += T
            seen += 1
    assert seen > 100


def test_features_match_the_oracle_front_end_on_a_generic_signal():
    """the whole chain (frames, spectrum, channels, PCEN) against oracle/features_ref.features_one, with and without PCEN
    (pcenfunc's training and evaluation branches compute the same values; the oracle restates them once), on signals with
    no bin near zero, to 1e-9 (sin / cos divide by the magnitude)"""
    for L in G.FEAT_L:
        x = G.signal("gauss0.1", L, "oracle")
        want = fr.features_one(x.double()[None, None], pcen=True)                              # (T, 4, 257)
        got = R.features([x], 4)
        for ch in (0, 2, 3):
            assert float((got["feat"][:, ch] - want[:, ch]).abs().max()) <= 1e-9
        assert float((R.pcen([got["mag"]], raw=True) - want[:, 1]).abs().max()) <= 1e-12
        want3 = fr.features_one(x.double()[None, None], pcen=False)
        assert float((R.features([x], 3)["feat"] - want3).abs().max()) <= 1e-9


def test_pcen_matches_the_oracle_in_double():
    """with the parameters as the oracle writes them (doubles) to 1e-12; the reference of the pin carries the fp32 values of
    the C ABI, which is the same function 1e-6 away"""
    for case in G.PCEN_CASES:
        c = G.pcen_inputs(case)
        want = torch.cat([fr.pcen_ref(m.double()[None])[0] for m in c.mags])
        scale = max(1.0, float(want.abs().max()))
        assert float((R.pcen(c.mags, raw=True) - want).abs().max()) <= 1e-12 * scale
        assert float((c.ref - want).abs().max()) <= 2e-6 * scale


def test_the_cpu_yardstick_log10_is_inside_the_ulp_count_of_the_nm_bound():
    """the device library's documented bound (2 ulp) is what the nm bound counts; the CPU yardstick's own log10 is measured
    here and lies inside it"""
    assert R.log10_ulp_cpu() <= R.LOG10_ULP


# ---------------------------------------------------------------------------------------------- 2. layouts
def test_layouts_and_offset_arrays_round_trip():
    g = G._gen("layouts")
    for N, NP in ((9, 256), (255, 256), (256, 256), (30, 512)):
        feat, mag = G._rn(g, N, 4, 257), G._rn(g, N, 257)
        for t in (feat, mag):
            x = R.to_fl(t, NP)
            assert x.shape == t.shape[1:] + (NP,)
            back, tail = R.from_fl(x, N)
            assert torch.equal(back, t) and bool((tail == 0).all())
        assert float(R.to_fl(feat, NP)[2, 5, N - 1]) == float(feat[N - 1, 2, 5])
    so, fo, po = R.ragged_offsets([257, 640, 383, 1025])
    assert so.tolist() == [0, 257, 897, 1280, 2305] and fo.tolist() == [0, 3, 9, 12, 21] and po.tolist() == [0, 2, 5, 7, 12]
    # a packed batch is its utterances one after the other
    xs = [G.signal("gauss0.1", L, "rt") for L in (257, 640, 383)]
    packed = R.features(xs, 3)
    alone = torch.cat([R.features([x], 3)["feat"] for x in xs])
    assert torch.equal(packed["frames"], torch.cat([R.features([x], 3)["frames"] for x in xs]))
    assert float((packed["feat"] - alone).abs().max()) <= 1e-9


# ---------------------------------------------------------------------------------------------- 3. the comparison
FAMILIES = (
    ("feat", lambda: [G.feat_inputs(k) for k in G.FEAT_CASES], G.feat_emul, G.judge_feat),
    ("fl-edge", lambda: [G.fl_edge_inputs(k) for k in G.FL_EDGE_CASES], lambda c, mut=None, order="fft":
        G.feat_emul(c, mut, order, fl=(256,)), G.judge_feat),
    ("ragged", lambda: [G.ragged_inputs(i, C) for i in range(len(G.RAGGED_CASES)) for C in (3, 4)], G.ragged_emul, G.judge_ragged),
    ("pcen", lambda: [G.pcen_inputs(k) for k in G.PCEN_CASES] + [G.pcen_ragged_inputs()], G.pcen_emul, G.judge_pcen),
    ("stream", lambda: [G.stream_inputs(k) for k in G.STREAM_CASES], G.stream_emul, G.judge_stream),
)


@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f[0])
def test_both_fp32_orders_of_the_restatement_pass_every_case(fam):
    _, cases, emul, judge = fam
    for c in cases():
        for order in ("dft", "fft"):
            bad = G.rejected(judge, c, emul(c, None, order))
            assert not bad, (c.tag, order, bad)


def _rejecting_case(mut):
    for name, cases, emul, judge in FAMILIES:
        for c in cases():
            if G.rejected(judge, c, emul(c, mut)):
                return c.tag
    return None


@pytest.mark.parametrize("mut", [m for m in R.MUTANTS if m not in R.EQUIVALENT])
def test_every_mutant_is_rejected_by_at_least_one_case(mut):
    assert _rejecting_case(mut) is not None, "no case rejects %s: a case is missing" % mut


def test_mutants_are_rejected_by_the_family_they_break():
    """the mutants whose home is one entry family are rejected THERE (not only by a neighbour that shares the arithmetic)"""
    home = {"ragged_pairs_across_utterances": 2, "odd_T_partner_not_zero": 0, "pcen_restart_at_256": 3, "pcen_restart_at_128": 3,
            "pcen_carried_across_utterances": 3, "pcen_bin256_unwritten": 3, "stream_ring_not_shifted": 4, "no_silent_guard": 4,
            "c3_channel_order": 0, "frames_ceil": 0}
    for mut, i in home.items():
        _, cases, emul, judge = FAMILIES[i]
        assert any(G.rejected(judge, c, emul(c, mut)) for c in cases()), mut
    # the silent-frame guard in the offline families too
    for i in (0, 2):
        _, cases, emul, judge = FAMILIES[i]
        assert any(G.rejected(judge, c, emul(c, "no_silent_guard")) for c in cases())


def test_a_floor_below_the_clamp_knee_is_an_equivalent_mutant():
    """nm is held at -1 for every mag <= 10^-3.75, so the floor 1e-6 in place of 1e-7 changes no output bit in any case (the
    floor that can be seen, 1e-3, is in the rejected list)"""
    for c in _all_feature_inputs():
        a, b = R.features(c.xs, c.C, torch.float32, "fft"), R.features(c.xs, c.C, torch.float32, "fft", "db_floor_1e-6")
        assert torch.equal(a["feat"][:, 0], b["feat"][:, 0])
    m = torch.logspace(-9, -3.76, 1000, dtype=f64)
    assert bool((R.nm_of(m) == -1).all()) and bool((R.nm_of(m, mut="db_floor_1e-6") == -1).all())


# ---------------------------------------------------------------------------------------------- 4. conditions on the inputs
def test_the_cases_hold_what_their_names_say():
    silent_even = silent_odd = 0
    for c in _all_feature_inputs():
        off = 0
        for L in c.lengths:
            T = R.nframes(L)
            z = c.silent[off:off + T]
            loud = c.ref["partner"][off:off + T].norm(dim=-1) > 1.0
            silent_even += int((z & loud)[0::2].sum())
            silent_odd += int((z & loud)[1::2].sum())
            off += T
    assert silent_even > 0 and silent_odd > 0                       # an exactly silent frame beside a loud one, on both sides
    c = G.feat_inputs((640, 3, "noise"))
    assert bool((c.ref["feat"][:, 0] == 1).any())                   # amplitude 30 reaches the upper clamp
    c = G.feat_inputs((640, 3, "quiet"))
    T = c.T
    assert bool((c.ref["feat"][:T, 0] == -1).all()) and float(c.ref["mag"][:T].max()) > 0       # 1e-9: under the floor, not zero
    c = G.feat_inputs((640, 3, "tonal"))
    tone = c.ref["mag"][2]                                          # frame 2 of L = 640 reads samples 0 .. 511: no reflection
    assert float(tone.median()) < 1e-9 * float(tone.max())          # the tone: most bins near zero
    assert {G.fl_edge_inputs(k).N for k in G.FL_EDGE_CASES} == {256, 255}


def test_the_lockstep_interval_is_a_statement_for_every_stream_that_is_not_silent():
    """(e): the float64 interval spanned by mag64 -+ d is, for every stream that is not exactly silent, narrower than a
    hundredth of the case's largest PCEN value, so a wrong smoother cannot hide inside it.  A silent stream beside a loud one
    has the interval the design allows a nearly silent frame (an error proportional to its partner's norm); its values are
    held by the exact silent checks instead."""
    for case in G.STREAM_CASES:
        c = G.stream_inputs(case)
        assert G.interval_condition(c) < 1e-2, (c.tag, G.interval_condition(c))


@pytest.mark.parametrize("L", G.SILENT_L)
def test_the_silent_frame_comparison_accepts_the_restatement_and_rejects_the_leak(L):
    """tests/test_frontend_pin_gpu.py's silent-frame test on the restatement: both fp32 orders pass, and the pair transform
    WITHOUT the guard (what the kernels computed before it) is rejected: the fp32 emulation of the leak"""
    judge = lambda c, got, quiet=False: G.judge_silent(c, got, quiet)        # noqa: E731
    for order in ("dft", "fft"):
        assert not G.rejected(judge, L, G.silent_emul(L, None, order))
    # (the matrix order multiplies a zero frame into exact zeros, which the split's P + W, P - W then cancel exactly: only
    # a transform that mixes the two halves stage by stage leaks)
    assert G.rejected(judge, L, G.silent_emul(L, "no_silent_guard", "fft"))
