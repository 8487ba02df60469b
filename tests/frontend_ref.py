"""Plain torch restatement of the feature front end of include/trunet_hip.h (fft.hip): trunet_stft_features, trunet_pcen,
their frames-last (`_fl`) and ragged siblings and the lockstep trunet_stream_features.  Written from the header's contracts
and the reference's dataset.py:56-76, 207-272 with explicit index maps and an explicit DFT matrix; torch.stft appears
nowhere (tests/test_frontend_ref_cpu.py holds this file to it and to oracle/features_ref.py).

    frames     T = 1 + L // 128;  frame t, tap i reads x[reflect(128 t + i - 256)],  reflect as tests/losstail_ref.py
    spectrum   rectangular window, n = 512:  X[k] = sum_i frame[i] e^{-2 pi j k i / 512},  k = 0 .. 256
    channels   mag = sqrt(re^2 + im^2);  nm = clamp(((20 log10(max(mag, 1e-7)) - 25 + 100) / 100) * 2 - 1, -1, 1);
               (sin, cos) = (im, re) / mag, and (0, 1) where mag == 0.   C = 3: (nm, sin, cos);  C = 4: (nm, -, sin, cos),
               channel 1 is left for PCEN
    layouts    dense (B T, C, 257);  frames-last [C][257][NP], frame n = b T + t in the last dimension, columns n >= N zero;
               ragged: utterances packed back to back with sample_off / frame_off / pair_off (prefix sums of L_b, T_b,
               ceil(T_b / 2))
    PCEN       M[0] = s v[0],  M[t] = (1 - s) M[t-1] + s v[t],  (v / (M + eps)^alpha + delta)^r - delta^r;  the smoother
               restarts per utterance (dense, _fl, ragged) and is carried across calls in pcen_M by the lockstep form
               (`first`: M = s v)
    lockstep   ring <- [ring[128:], chunk] (chunk None: the ring as it is), then ONE frame = the ring
    pairing    two real frames share one complex transform: frames 2i, 2i + 1 of one utterance (a lone last frame with
               zeros), streams 2i, 2i + 1 of a lockstep call.  CONTRACT: a frame whose 512 staged samples are all exactly
               zero has an exactly zero spectrum, whatever its partner holds.

dtype = float64 is the reference: every frame transformed on its own.  float32 is the yardstick, in two orders: `dft` (the
fp32 DFT-matrix product) and `fft` (torch.fft in complex64), each on the PAIR a + j b followed by the split algebra
A[k] = (Z[k] + conj Z[n-k]) / 2, B[k] = (Z[k] - conj Z[n-k]) / (2j), so the yardstick carries the partner's rounding leak
the way the kernels do; for the smoother the two orders are multiply-add and fused multiply-add.
tests/losstail_ref.py's `yardstick` keeps the worse of the two element by element.

Counted roundings (U = 2^-24), used by tests/frontend_cases.py:
  F_MAG = 14: a bin of the fp32 transform of a pair, against the exact one, beyond what the yardstick's own error E_f
      measures: 9 radix-2 stages (the kernel's radix-4 passes do the same butterflies), the split's 2 additions and its
      halving (exact, counted), the square root: 13 roundings, (r + 1) U as in tests/bn_cases.py, relative to
      ||frame||_2 + ||partner||_2 (a butterfly output is bounded by the 2-norm of what feeds it).
  nm from a given fp32 mag (`nm_raw64`): log10f 2 ulp = 4 U |l| (the HIP math API's table of maximum ulp errors of the
      device library; that documentation is not installed next to the compiler, so tests/test_frontend_ref_cpu.py also
      measures the CPU yardstick's log10: below 1 ulp), 20 l (1), - 25 (1), + 100 (1), / 100 (1), * 2 (exact), - 1 (1),
      each relative to its own result and carried through the chain.
  sin^2 + cos^2 - 1 (`UNIT_BOUND` = 10 U): mag = sqrt(re^2 + im^2) is 2.5 U relative (two squares and a sum, halved by the
      root, plus the root), each quotient one more: (cos^2 + sin^2) is within 2 (2.5 + 1) U of 1, the two squares and the
      sum add 2 U: 9 U, + 1.

`mut` names ONE deliberate error (MUTANTS); tests/test_frontend_ref_cpu.py passes each through the comparison of the GPU
test in place of kernel output.  `db_floor_1e-6` is an EQUIVALENT mutant: the clamp holds nm at -1 for every
mag <= 10^-3.75 = 1.8e-4, so a floor anywhere below that cannot change an output bit (asserted there); `db_floor_1e-3`
is the wrong floor that can be seen."""

import torch

import losstail_ref as LR

MUTANTS = ("reflect_right_off1", "no_left_reflect", "frames_ceil", "odd_T_partner_not_zero",
           "db_floor_1e-6", "db_floor_1e-3", "db_offset_20", "clamp_high_missing",
           "sin_negated", "sin_cos_swapped", "angle0_is_sin1", "nyquist_bin_dropped",
           "c3_channel_order",
           "pcen_M0_zero", "pcen_restart_at_256", "pcen_restart_at_128", "pcen_carried_across_utterances", "pcen_s_swapped",
           "pcen_eps_outside_pow", "pcen_bin256_unwritten",
           "stream_ring_not_shifted", "ragged_pairs_across_utterances", "no_silent_guard")
EQUIVALENT = ("db_floor_1e-6",)
NF, HOPF, BINS = LR.NF, LR.HOPF, LR.BINS
EPS, S, ALPHA, DELTA, RPOW = 1e-6, 0.025, 0.98, 2.0, 0.5          # dataset.py:56
U = 2.0 ** -24
F_MAG = 14 * U
UNIT_BOUND = 10 * U
LOG10_ULP = 2.0
f64, f32t = torch.float64, torch.float32
NAN = float("nan")
yardstick = LR.yardstick
f32 = LR.f32


# ---------------------------------------------------------------------------------------------- staging
def nframes(L, mut=None):
    return LR.nframes(L, HOPF, mut)


def stage(x, dtype=f64, mut=None):
    """x (L) -> frames (T, 512)"""
    idx = LR.pad_map(x.shape[-1], NF, HOPF, mut)
    return x.to(dtype)[idx].unfold(0, NF, HOPF)


def partner_frames(fr, mut=None):
    """fr (T, 512) of ONE utterance -> the frame that shares each frame's transform (zeros for a lone last frame)"""
    T = fr.shape[0]
    p = torch.zeros_like(fr)
    for t in range(T):
        q = t ^ 1
        if q < T:
            p[t] = fr[q]
        elif mut == "odd_T_partner_not_zero" and t > 0:
            p[t] = fr[t - 1]                     # the imaginary half still holds the frame before
    return p


# ---------------------------------------------------------------------------------------------- spectrum
def spectrum64(fr):
    """(..., 512) float64 frames, each on its own -> (re, im) (..., 257)"""
    return LR.spectrum(fr.to(f64), "dft")


def pair_spectrum(a, b, order, guard=True):
    """fp32: frames a, b (..., 512) as ONE complex sequence a + j b, then the split.  Returns (Are, Aim, Bre, Bim)."""
    assert a.dtype == f32t and b.dtype == f32t
    if order == "fft":
        Z = torch.fft.fft(torch.complex(a, b), dim=-1)
        k = torch.arange(BINS)
        zk, zn = Z[..., k], torch.conj(Z[..., (NF - k) % NF])
        zkx, zky, znx, zny = zk.real, zk.imag, zn.real, zn.imag
    else:
        Cm, Sm = LR.dft_matrices(NF, f32t)
        P, Q, Rr, W = a @ Cm.t(), a @ Sm.t(), b @ Cm.t(), b @ Sm.t()
        zkx, zky = P + W, Rr - Q                                   # Z[k]
        znx, zny = P - W, -(Rr + Q)                                # conj Z[n - k]
    Are, Aim = 0.5 * (zkx + znx), 0.5 * (zky + zny)
    Bre, Bim = 0.5 * (zky - zny), -0.5 * (zkx - znx)
    if guard:
        za, zb = (a == 0).all(-1, keepdim=True), (b == 0).all(-1, keepdim=True)
        zero = torch.zeros((), dtype=f32t)
        Are, Aim = torch.where(za, zero, Are), torch.where(za, zero, Aim)
        Bre, Bim = torch.where(zb, zero, Bre), torch.where(zb, zero, Bim)
    return Are, Aim, Bre, Bim


def spectra(fr, part, dtype, order, mut=None):
    """frames and their partners (N, 512) -> (re, im) (N, 257) of the frames"""
    if dtype == f64:
        return spectrum64(fr)
    return pair_spectrum(fr.to(f32t), part.to(f32t), order, guard=mut != "no_silent_guard")[:2]


# ---------------------------------------------------------------------------------------------- channels
def nm_of(mag, dtype=f64, mut=None):
    mag = mag.to(dtype)
    floor = {"db_floor_1e-6": 1e-6, "db_floor_1e-3": 1e-3}.get(mut, 1e-7)
    db = 20.0 * torch.log10(mag.clamp_min(f32(floor) if dtype == f64 else floor)) - (20.0 if mut == "db_offset_20" else 25.0)
    nm = ((db + 100.0) / 100.0) * 2.0 - 1.0
    return nm.clamp_min(-1.0) if mut == "clamp_high_missing" else nm.clamp(-1.0, 1.0)


def nm_raw64(mag):
    """(unclamped nm, its rounding bound) in float64 from fp32 magnitudes, the floor at the fp32 value of 1e-7"""
    m = mag.double().clamp_min(f32(1e-7))
    l = torch.log10(m)
    db = 20.0 * l - 25.0
    q = (db + 100.0) / 100.0
    raw = q * 2.0 - 1.0
    e_db = (2.0 * LOG10_ULP + 1.0) * U * 20.0 * l.abs() + U * db.abs()
    e_q = (e_db + U * (db + 100.0).abs()) / 100.0 + U * q.abs()
    return raw, 2.0 * e_q + U * raw.abs() + U


def channels(re, im, dtype, mut=None):
    """(re, im) (N, 257) -> mag, nm, sin, cos (N, 257)"""
    mag = torch.sqrt(re * re + im * im)
    nm = nm_of(mag, dtype, mut)
    live = mag > 0
    one, zero = torch.ones((), dtype=dtype), torch.zeros((), dtype=dtype)
    den = torch.where(live, mag, one)
    sn, cs = torch.where(live, im / den, zero), torch.where(live, re / den, one)
    if mut == "angle0_is_sin1":
        sn, cs = torch.where(live, sn, one), torch.where(live, cs, zero)
    if mut == "sin_negated":
        sn = -sn
    if mut == "sin_cos_swapped":
        sn, cs = cs, sn
    return mag, nm, sn, cs


def pack_dense(nm, sn, cs, C, mut=None):
    """(N, 257) channels -> feat (N, C, 257), what the kernel does not write left NaN"""
    feat = torch.full((nm.shape[0], C, BINS), NAN, dtype=nm.dtype)
    feat[:, 0] = nm
    if mut == "c3_channel_order" and C == 3:
        feat[:, 2] = sn                          # channel 3 of this frame is channel 0 of the next: cos is lost
    else:
        feat[:, C - 2], feat[:, C - 1] = sn, cs
    if mut == "nyquist_bin_dropped":
        feat[:, :, BINS - 1] = NAN
    return feat


def features(xs, C, dtype=f64, order="dft", mut=None, pair_across=False):
    """xs: list of utterances (L_b) fp32 -> {feat (sum T, C, 257), mag (sum T, 257), re, im, frames, partner (sum T, 512)};
    frames are paired per utterance (`pair_across`: over the packed frame index, the ragged mutant)"""
    assert order in ("dft", "fft") and (mut is None or mut in MUTANTS)
    frs = [stage(x, f64 if dtype == f64 else f32t, mut) for x in xs]
    if pair_across:
        allf = torch.cat(frs, 0)
        parts = partner_frames(allf)
    else:
        parts = torch.cat([partner_frames(f, mut) for f in frs], 0)
        allf = torch.cat(frs, 0)
    re, im = spectra(allf, parts, dtype, order, mut)
    mag, nm, sn, cs = channels(re, im, dtype, mut)
    if mut == "nyquist_bin_dropped":
        mag = mag.clone()
        mag[:, BINS - 1] = NAN
    return {"feat": pack_dense(nm, sn, cs, C, mut), "mag": mag, "re": re, "im": im, "frames": allf, "partner": parts}


# ---------------------------------------------------------------------------------------------- layouts
def to_fl(feat, NP):
    """(N, C, 257) or (N, 257) -> [C][257][NP] or [257][NP], columns n >= N zero"""
    N = feat.shape[0]
    out = torch.zeros(feat.shape[1:] + (NP,), dtype=feat.dtype)
    out[..., :N] = feat.permute(*range(1, feat.dim()), 0)
    return out


def from_fl(x, N):
    """[C][257][NP] or [257][NP] -> ((N, C, 257) or (N, 257), the columns n >= N)"""
    return x[..., :N].permute(x.dim() - 1, *range(x.dim() - 1)).contiguous(), x[..., N:]


def ragged_offsets(lengths):
    """(sample_off, frame_off, pair_off), int64 [B + 1] each"""
    so, fo, po = [0], [0], [0]
    for L in lengths:
        T = nframes(L)
        so.append(so[-1] + L)
        fo.append(fo[-1] + T)
        po.append(po[-1] + (T + 1) // 2)
    return tuple(torch.tensor(v, dtype=torch.int64) for v in (so, fo, po))


# ---------------------------------------------------------------------------------------------- PCEN
def smooth(v, M0=None, dtype=f64, order="dft", mut=None, s=S, raw=False):
    """v (T, 257) of ONE utterance -> M (T, 257).  M0 None: M[0] = s v[0]; else the carried state.  order `fft` = fused
    multiply-add (the product s v exact inside the sum), `dft` = multiply, multiply, add."""
    s_ = s if raw else f32(s)
    v = v.to(dtype)
    om = 1.0 - s_ if dtype == f64 else float(torch.tensor(1.0, dtype=f32t) - torch.tensor(s_, dtype=f32t))     # 1.f - s
    a, b = (s_, om) if mut == "pcen_s_swapped" else (om, s_)
    M = torch.empty_like(v)
    prev = None if M0 is None else M0.to(dtype)
    for t in range(v.shape[0]):
        restart = prev is None or (mut == "pcen_restart_at_256" and t == 256) or (mut == "pcen_restart_at_128" and t == 128)
        if restart:
            cur = torch.zeros_like(v[t]) if (mut == "pcen_M0_zero" and t == 0) else (s_ * v[t]).to(dtype)
        elif dtype == f32t and order == "fft":
            cur = (a * prev.double() + (b * v[t]).double()).to(f32t)          # one rounding of a M + (s v rounded)
        else:
            cur = a * prev + b * v[t]
        M[t] = cur
        prev = cur
    return M


def pcen_value(v, M, dtype=f64, mut=None, eps=EPS, alpha=ALPHA, delta=DELTA, r=RPOW, raw=False):
    if not raw:
        eps, alpha, delta, r = f32(eps), f32(alpha), f32(delta), f32(r)
    v, M = v.to(dtype), M.to(dtype)
    den = (M.pow(alpha) + eps) if mut == "pcen_eps_outside_pow" else (M + eps).pow(alpha)
    dr = torch.tensor(delta, dtype=dtype).pow(r)
    return (v / den + delta).pow(r) - dr


def pcen(mags, dtype=f64, order="dft", mut=None, raw=False):
    """mags: list of (T_b, 257) fp32, one per utterance -> (sum T, 257).  The parameters are the fp32 values the C ABI
    carries (s = 0.025f is 3.7e-10 off 0.025, which the smoother's long memory turns into 5e-7 of the output); `raw`: the
    doubles as written, for the comparison with the oracle."""
    assert mut is None or mut in MUTANTS
    outs, carry = [], None
    for v in mags:
        M = smooth(v, carry if mut == "pcen_carried_across_utterances" else None, dtype, order, mut, raw=raw)
        carry = M[-1]
        o = pcen_value(v, M, dtype, mut, raw=raw)
        if mut == "pcen_bin256_unwritten":
            o[:, BINS - 1] = NAN
        outs.append(o)
    return torch.cat(outs, 0)


# ---------------------------------------------------------------------------------------------- lockstep stream
def stream(ring0, chunks, C, dtype=f64, order="dft", mut=None):
    """ring0 (S, 512) fp32, chunks (H, S, 128) fp32: call 0 is `first` with chunk None on the ring as it is, calls 1 .. H
    shift a chunk in.  Returns {feat (H + 1, S, C, 257), ring (H + 1, S, 512) after each call, pcen_M (S, 257) after the
    last, mag, re, im (H + 1, S, 257), frames, partner (H + 1, S, 512)}"""
    assert order in ("dft", "fft") and (mut is None or mut in MUTANTS)
    S_ = ring0.shape[0]
    ring = ring0.clone()
    out = {k: [] for k in ("feat", "ring", "mag", "re", "im", "frames", "partner")}
    M = None
    for h in range(chunks.shape[0] + 1):
        if h > 0:
            ring = torch.cat([ring[:, :NF - HOPF] if mut == "stream_ring_not_shifted" else ring[:, HOPF:], chunks[h - 1]], 1)
        fr = ring.to(f64 if dtype == f64 else f32t)
        part = torch.zeros_like(fr)
        for i in range(S_):
            if (i ^ 1) < S_:
                part[i] = fr[i ^ 1]
        re, im = spectra(fr, part, dtype, order, mut)
        mag, nm, sn, cs = channels(re, im, dtype, mut)
        feat = pack_dense(nm, sn, cs, C, mut)
        if C == 4:
            Mn = torch.stack([smooth(mag[i:i + 1], None if M is None else M[i], dtype, order, mut)[0] for i in range(S_)])
            M = Mn
            feat[:, 1] = pcen_value(mag, M, dtype, mut)
            if mut == "pcen_bin256_unwritten":
                feat[:, 1, BINS - 1] = NAN
        for k, v in (("feat", feat), ("ring", ring.clone()), ("mag", mag), ("re", re), ("im", im), ("frames", fr),
                     ("partner", part)):
            out[k].append(v)
    out = {k: torch.stack(v) for k, v in out.items()}
    out["pcen_M"] = M if M is not None else torch.zeros(S_, BINS, dtype=dtype)
    return out


def log10_ulp_cpu():
    """the CPU yardstick's log10 in fp32 against float64 over the magnitudes of the front end, in ulp"""
    m = torch.logspace(-7, 4, 200001, dtype=f64).float()
    got, ref = torch.log10(m).double(), torch.log10(m.double())
    ulp = 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(1e-30))) - 23)
    return float(((got - ref).abs() / ulp).max())
