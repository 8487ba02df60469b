"""tests/losstail_ref.py is right (against torch autograd through oracle/stft_loss_ref.py and
oracle/features_ref.denoise_from_output in double), the comparison of tests/test_losstail_gpu.py accepts the restatement in
every case of its lists and has teeth (each mutant is rejected exactly where it computes other numbers), and the input
conditions the GPU test relies on hold -- without a GPU."""
import math

import pytest
import torch

import convt_ref as CR
import losstail_cases as G
import losstail_ref as R
from oracle import features_ref as fr, stft_loss_ref as slr

f64 = torch.float64


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ---------------------------------------------------------------------------------------------- 1. independent reference
@pytest.mark.parametrize("shape", [(512, 50, 240, 257), (1024, 120, 601, 1500), (8, 3, 5, 37), (128, 40, 30, 200),
                                   (256, 64, 255, 129), (512, 128, 512, 640)])
def test_stft_restatement_matches_autograd_in_double(shape):
    """magnitudes, the three sums and every gradient of the restatement (explicit reflect map, explicit DFT matrix, the
    gather written as the pad's adjoint) against torch.stft + autograd in double, to 1e-12: the two gradient frame tables
    overlap-added are d S1 / dx / 2-ish and d S3 / dx exactly as the kernels define them, the coefficient form is the
    gradient of c_sc-, c_mag-weighted sums, and stft_mag_bwd is the vector-Jacobian product with a random cotangent"""
    n, hop, wl, L = shape
    c = G.stft_inputs(shape + ("noise",))
    r = c.ref64
    x = c.x.double().requires_grad_(True)
    w = torch.hann_window(wl, dtype=f64)
    xm, ym = slr.stft_mag(x, n, hop, wl, w), slr.stft_mag(c.y.double(), n, hop, wl, w)
    assert xm.shape == r["xmag"].shape and _rel(r["xmag"], xm.detach()) < 1e-12 and _rel(r["ymag"], ym) < 1e-12
    S1, S2, S3 = ((ym - xm) ** 2).sum(), (ym ** 2).sum(), (torch.log(ym) - torch.log(xm)).abs().sum()
    p = r["partials"].sum(0)
    assert abs(float(p[0] - S1)) < 1e-12 * float(S1) and abs(float(p[1] - S2)) < 1e-12 * float(S2)
    assert abs(float(p[2] - S3)) < 1e-12 * float(S3)
    g1, = torch.autograd.grad(S1, x, retain_graph=True)
    g3, = torch.autograd.grad(S3, x, retain_graph=True)
    assert _rel(2.0 * r["g_sc"], g1) < 1e-12 and _rel(r["g_mag"], g3) < 1e-12
    gc, = torch.autograd.grad(0.5 * c.coef[0].double() * S1 + c.coef[1].double() * S3, x, retain_graph=True)
    assert _rel(r["bwd_gx"], gc) < 1e-12 and _rel(r["fused_gx"], gc) < 1e-12
    gm, = torch.autograd.grad((xm * c.gmag.double()).sum(), x)
    assert _rel(r["magbwd_gx"], gm) < 1e-12
    # the whole loss of one resolution through the algebra: sc = sqrt(S1) / sqrt(S2), mag = S3 / count
    sc, mag = slr.stft_loss_one(c.x.double(), c.y.double(), n, hop, wl, w)
    cnt = float(xm.numel())
    v = R.loss_finalize(torch.zeros(1), 1.0, [r["partials"]], [cnt], 0.3, 0.8, 1.0)
    assert abs(float(v[2]) - R.f32(0.3) * float(sc)) < 1e-12 and abs(float(v[3]) - R.f32(0.8) * float(mag)) < 1e-12
    x2 = c.x.double().requires_grad_(True)
    sc2, mag2 = slr.stft_loss_one(x2, c.y.double(), n, hop, wl, w)
    (R.f32(0.3) * sc2 + R.f32(0.8) * mag2).backward()
    assert _rel(v[5] * r["g_sc"] + v[6] * r["g_mag"], x2.grad) < 1e-11


def test_x_equal_y_has_a_zero_gradient_in_torch_and_in_the_restatement():
    """the finding's reference: torch's spectral convergence and log-magnitude terms at x == y are 0 with an all-zero,
    finite gradient; the restatement gives exact zeros and a zero c_sc (not inf) at S1 == 0"""
    c = G.stft_inputs((8, 3, 5, 37, "identical"))
    x = c.x.double().requires_grad_(True)
    sc, mag = slr.stft_loss_one(x, c.x.double(), 8, 3, 5, torch.hann_window(5, dtype=f64))
    (sc + mag).backward()
    assert float(sc) == 0 and float(mag) == 0 and bool((x.grad == 0).all())
    r = c.ref64
    assert bool((r["partials"][:, 0] == 0).all()) and bool((r["partials"][:, 2] == 0).all())
    assert bool((r["fr_sc"] == 0).all()) and bool((r["fr_mag"] == 0).all())
    v = R.loss_finalize(torch.zeros(1), 1.0, [r["partials"]], [1.0], 0.5, 0.5, 1.0)
    assert bool(torch.isfinite(v).all()) and float(v[5]) == 0 and float(v[2]) == 0 and float(v[3]) == 0


@pytest.mark.parametrize("T,beta", [(2, 0.5), (3, 2.0), (4, 0.5), (5, 2.0), (9, 0.5)])
def test_mask_istft_restatement_matches_autograd_in_double(T, beta):
    """forward and the hand-written backward against autograd through features_ref.denoise_from_output (torch.istft) in
    double, away from the atan2 origin; c0 beyond +-1 is part of the inputs"""
    c = G.mask_inputs((T, beta, 1, "generic"))
    o = c.net_out.double().requires_grad_(True)
    den = fr.denoise_from_output(o, T, R.f32(beta), length=c.L)
    assert _rel(c.ref64["audio"], den.detach()) < 1e-12
    (den * c.g_audio.double()).sum().backward()
    assert bool((c.net_out[:, 0].abs() > 1).any())
    assert _rel(c.ref64["g_net"], o.grad) < 1e-12
    l1 = (den.detach() - c.clean.double()).abs().sum()
    assert abs(float(c.ref64["l1"].sum() - l1)) < 1e-12 * float(l1) and c.ref64["l1"].numel() == c.nparts


def test_mask_backward_contract_at_the_edges():
    """the contract at the points autograd cannot vouch for, checked on the restatement: zero for an exactly-zero phase pair
    (torch's atan2 backward there is NaN or 0, depending on the release), the closed interval for the clamp (torch agrees:
    asserted), finite everywhere"""
    z, w = torch.zeros(1, dtype=f64, requires_grad=True), torch.zeros(1, dtype=f64, requires_grad=True)
    torch.atan2(z, w).backward()
    assert bool((torch.isnan(z.grad) | (z.grad == 0)).all()) and bool((torch.isnan(w.grad) | (w.grad == 0)).all())
    e = torch.tensor([1.0, -1.0], dtype=f64, requires_grad=True)
    e.clamp(-1, 1).sum().backward()
    assert bool((e.grad == 1).all())
    for regime in ("zero_pairs", "c0_edge", "neg_axis"):
        c = G.mask_inputs((3, 2.0, 1, regime))
        g, o = c.ref64["g_net"], c.net_out
        assert bool(torch.isfinite(g).all()) and all(bool(torch.isfinite(v).all()) for v in c.ref64.values())
        if regime == "zero_pairs":
            zm = (o[:, 2] == 0) & (o[:, 3] == 0)
            zn = (o[:, 6] == 0) & (o[:, 7] == 0)
            assert int(zm.sum()) > 50 and int(zn.sum()) > 50 and int((zm & zn).sum()) > 20
            assert bool((g[:, 2][zm] == 0).all()) and bool((g[:, 6][zn] == 0).all()) and bool((g[:, 2][zn & ~zm] != 0).any())
        if regime == "c0_edge":
            edge = o[:, 0].abs() == 1
            assert int(edge.sum()) > 100 and bool((g[:, 0][edge] != 0).all()) and bool((g[:, 0][o[:, 0].abs() > 1] == 0).all())
        if regime == "neg_axis":
            neg = (o[:, 2] == 0) & (o[:, 3] < 0)
            assert bool(torch.signbit(o[:, 2][neg]).any()) and bool((~torch.signbit(o[:, 2][neg])).any())


# ---------------------------------------------------------------------------------------------- 2. close's constants
def test_the_two_fp32_orders_agree_through_close():
    """the torch.fft order of the restatement taken as `got` against float64 with the DFT-matrix order as the ONLY yardstick
    (the matrix product is the noisier of the two by a factor of 4 to 5, so this is the direction that can hold): convt_ref.close's
    c = 4 and f hold for this chain without a GPU, in every case and output (the STFT generator's `stable` condition; the
    first seed qualifies in all but a few cases, printed)"""
    print("seeds:", " ".join("%s=%d" % (G.stft_id(k), G.stft_inputs(k).seed) for k in G.STFT_CASES if G.stft_inputs(k).seed))
    for case in G.STFT_CASES:
        c = G.stft_inputs(case)
        for k in G.STABLE_OUT:
            CR.close(c.o_fft[k], c.ref64[k], c.o_dft[k], "%s %s" % (G.stft_id(case), k))
    for case in G.MASK_CASES[::4]:
        c = G.mask_inputs(case)
        T, beta = c.T, c.beta
        a = R.mask_istft_fwd(c.net_out, T, beta, clean=c.clean, dtype=torch.float32, order="dft")
        b = R.mask_istft_fwd(c.net_out, T, beta, clean=c.clean, dtype=torch.float32, order="fft")
        a["g_net"] = R.mask_istft_bwd(c.g_audio, c.net_out, T, beta, torch.float32, "dft")
        b["g_net"] = R.mask_istft_bwd(c.g_audio, c.net_out, T, beta, torch.float32, "fft")
        for k in c.ref64:
            CR.close(b[k], c.ref64[k], a[k], "%s %s" % (G.mask_id(case), k))


# ---------------------------------------------------------------------------------------------- 3. mutants
FAMILIES = {
    "stft": (G.STFT_CASES, G.stft_inputs, G.stft_emul, G.judge_stft),
    "gather": (G.GATHER_CASES, G.gather_inputs, G.gather_emul, G.judge_gather),
    "mask": (G.MASK_CASES, G.mask_inputs, G.mask_emul, G.judge_mask),
    "rc": (G.RC_CASES, G.rc_inputs, G.rc_emul, G.judge_rc),
    "fin": (G.FIN_CASES, G.fin_inputs, G.fin_emul, G.judge_fin),
    "l1": (G.L1_N, G.l1_inputs, G.l1_emul, G.judge_l1),
}


def _last_support_passes_the_end(c):
    return (c.F - 1) * c.hop + c.left + c.wl - 1 - c.n // 2 >= c.L


# mutant -> family -> is it visible in this case (c = the case's inputs)?
VISIBLE = {
    # the last frame's support reaches past sample L - 1 in every shape; signal 1 keeps noise there in every regime
    "reflect_right_off1": {"stft": _last_support_passes_the_end, "gather": lambda c: c.nres > 0},
    # frame 0 always starts left of sample 0 (left < n/2); signal 0 keeps noise at its start in every regime
    "no_left_reflect": {"stft": lambda c: True, "gather": lambda c: c.nres > 0},
    "frames_ceil": {"stft": lambda c: c.L % c.hop != 0},           # (the gather takes its frame count from the tables it is given)
    "win_left_ceil": {"stft": lambda c: (c.n - c.wl) % 2 == 1, "gather": lambda c: c.nres > 0},   # ... and n - wl = 423
    # exactly-zero frames have X == 0 and so no gradient either way: only 0 < px <= 1e-7 shows the branch
    # (`faint`, and the bins of the n = 8 shape that white noise leaves below the floor)
    "clamp_passes_grad": {"stft": lambda c: bool(((c.ref64["px"] > 0) & (c.ref64["px"] <= R.FLOOR)).any())},
    "mag_sign_flipped": {"stft": lambda c: c.regime != "identical"},
    "sign0_is_plus": {"stft": lambda c: c.regime in ("equal_bins", "identical")},
    "dc_weight_2": {"mask": lambda c: True},
    "nyquist_imag_kept": {"mask": lambda c: True},
    "env_uncapped": {"mask": lambda c: True},                       # the last 128 samples of every T
    "env_always_4": {"mask": lambda c: True},                       # the first 128 samples have 3 (T = 2: 2) frames
    "gather_drops_last_frame": {"stft": lambda c: True, "gather": lambda c: c.nres > 0},
    "coef_swapped": {"stft": lambda c: c.regime != "identical", "gather": lambda c: c.nres > 0},
    "l1_tail_block_dropped": {"mask": lambda c: c.with_clean and c.L % 256 != 0},
    "clamp_open_interval": {"mask": lambda c: c.regime == "c0_edge"},
}


def test_every_mutant_has_a_table_entry():
    assert set(VISIBLE) == set(R.MUTANTS)


@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_the_comparison_accepts_the_restatement_in_every_gpu_case(fam):
    """the judge_* functions of the GPU test, fed with what a kernel that follows the contract returns (the double
    restatement rounded once), pass in every case of the GPU lists"""
    cases, inputs, emul, judge = FAMILIES[fam]
    for case in cases:
        c = inputs(case)
        assert G.rejected(judge, c, emul(c)) == [], (fam, case)


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_the_comparison_rejects_mutants_where_they_are_visible(mut):
    """A subtly wrong kernel would fail: each mutant, passed through the GPU test's own comparison in place of kernel
    output, is REJECTED in every case of the GPU lists in which it computes other numbers and ACCEPTED in every other:
      reflect_right_off1   j >= L -> 2 (L - 1) - j + 1, in the staging and in the gather's fold
      no_left_reflect      j < 0 -> 0
      frames_ceil          1 + ceil(L / hop) frames: L % hop != 0 only
      win_left_ceil        left = ceil((n - wl) / 2): odd n - wl only
      clamp_passes_grad    a gradient at px <= 1e-7: only where 0 < px <= 1e-7 (`faint`)
      mag_sign_flipped     sign(log ym - log xm) for sign(log xm - log ym): wherever fr_mag is not all zero
      sign0_is_plus        sign(0) = +1: only where x == y over a frame
      dc_weight_2          the backward weighs DC and Nyquist 2 / 512
      nyquist_imag_kept    the partner frame's imaginary Nyquist part leaks into the frame
      env_uncapped         the envelope counts frames past T - 1: the last 128 samples
      env_always_4         the envelope is 4 everywhere: the first (and last) 128 samples
      gather_drops_last_frame   the last frame is never gathered
      coef_swapped         c_sc and c_mag change places
      l1_tail_block_dropped     the 128-sample tail block of L = 128 odd is not summed
      clamp_open_interval  c0 == +-1 exactly gets no gradient: `c0_edge` only"""
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
@pytest.mark.parametrize("case", G.STFT_CASES, ids=G.stft_id)
def test_stft_cases_meet_the_generator_conditions_and_have_the_edges_they_claim(case):
    """the floor and sign conditions hold with MARGIN = 16 (re-evaluated here, with the smallest ratios printed); the
    regimes contain what they are named after"""
    c = G.stft_inputs(case)
    assert G.stft_conditions(c) == []
    print("%s: seed %d, smallest margin ratio floor %.3g sign %.3g" % (G.stft_id(case), c.seed, c.min_floor, c.min_sign))
    assert c.min_floor > 1 and c.min_sign > 1 and c.F == 1 + c.L // c.hop
    r, px = c.ref64, c.ref64["px"]
    ypx = r["yre"] ** 2 + r["yim"] ** 2
    whole = lambda t: bool((t.flatten(1) if t.dim() > 1 else t).all(-1).any())      # a whole frame
    if c.regime == "silence_x":
        assert whole((px == 0).flatten(0, 1)) and not whole((ypx == 0).flatten(0, 1))
    if c.regime == "silence_y":
        assert whole((ypx == 0).flatten(0, 1)) and not whole((px == 0).flatten(0, 1))
    if c.regime == "silence_xy":
        assert whole(((px == 0) & (ypx == 0)).flatten(0, 1))
    if c.regime == "equal_bins":
        assert whole(((r["dl"] == 0) & (px > R.FLOOR)).flatten(0, 1)) and bool((r["dl"] != 0).any())
    if c.regime == "identical":
        assert bool((r["dl"] == 0).all()) and float((px > R.FLOOR).double().mean()) > 0.9 and torch.equal(c.x, c.y)
    if c.regime == "faint":
        low = (px > 0) & (px <= R.FLOOR)
        assert whole(low.flatten(0, 1)) and float((ypx > R.FLOOR)[low].double().mean()) > 0.5
    if c.regime == "noise":
        assert float((px > R.FLOOR).double().mean()) > 0.9 and (c.n == 8 or bool((px > R.FLOOR).all()))


def test_shapes_cover_the_paths():
    ns = {s[0] for s in G.STFT_SHAPES}
    assert {512, 1024, 2048} <= ns and {8, 64, 128, 256} <= ns                      # compile-time and runtime instances
    assert any(int(math.log2(s[0])) % 2 == 1 for s in G.STFT_SHAPES if s[0] < 512)   # the runtime radix-2 stage
    assert any(s[3] == s[0] // 2 + 1 for s in G.STFT_SHAPES) and any(s[2] == s[0] for s in G.STFT_SHAPES)
    assert any(s[2] % 2 == 1 for s in G.STFT_SHAPES) and any(s[1] > s[2] for s in G.STFT_SHAPES)
    assert any(s[3] % s[1] == 0 for s in G.STFT_SHAPES) and any(s[3] % s[1] != 0 for s in G.STFT_SHAPES)
    assert all(s[3] > s[0] // 2 and s[3] <= 2400 for s in G.STFT_SHAPES)
    assert {c[0] for c in G.MASK_CASES} == {2, 3, 4, 5, 9} and {c[1] for c in G.MASK_CASES} == {0.5, 2.0}
    assert {(c[0], c[2]) for c in G.MASK_CASES} == {(T, k) for T in G.MASK_T for k in (0, 1)}
    assert {c[0] for c in G.RC_CASES} == {1, 1023, 1024, 1025, 4096, 4097, 8197}
    assert {c[1] for c in G.FIN_CASES} == {0, 1, 3, 8} and any(c[2] == 0.0 for c in G.FIN_CASES) and G.SC_LAMBDA != G.MAG_LAMBDA
    assert all(G.GATHER_L > n // 2 for n, _, _ in G.GATHER_RES) and G.GATHER_L % 256 != 0
